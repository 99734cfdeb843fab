"""-m gpu: one material per model (Scene.material_slots, render(list); include/zdr.h zdr_render_*_materials).  Parity with the
oracle's material table is tests/test_gpu_materials_oracle.py; these are identities with the single-texture path — the legacy slot table
renders what render(tensor) renders, a mesh split in two instances renders what it rendered whole, constant textures of any
size render alike — and on finite differences of the forward render for the second material."""
import numpy as np
import pytest
import torch

from conftest import cbox_material_np, cbox_models, fd_material_np
from gpu_util import make_scene
from zdr_amd import geometry

pytestmark = pytest.mark.gpu

W, SPP = 64, 16


def rel_l1(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def mat_a():
    return torch.from_numpy(cbox_material_np()).cuda()


@pytest.fixture(scope="module")
def small_a(mat_a):
    """A 64 x 64 version of material A: with it the cell array of a call stays below 2^16 cells (cell copies, scene.h)."""
    return torch.nn.functional.avg_pool2d(mat_a.permute(2, 0, 1)[None], 16)[0].permute(1, 2, 0).contiguous()


def split_arrays(k=None):
    """The Cornell box with cboxuv.obj's triangles in two instances, [0, k) and [k, n): same vertices, same triangle order,
    light unchanged (instance 2)."""
    a = geometry.assemble(cbox_models())
    b = a.inst_tri_begin
    n = int(b[1])
    k = n // 2 if k is None else k
    return geometry.from_arrays(a.verts, a.tris, [0, k, n, int(b[2])], np.concatenate([a.inst_xform[:1], a.inst_xform]),
                                np.concatenate([a.inst_emission[:1], a.inst_emission]))


def assert_same_image(img, ref, integrator):
    """Path and collocated: bit for bit.  Direct: to the last bits only — its material-table kernel is a separate compilation in
    which the backend contracts some multiply-adds of the shading differently (measured on cbox 64^2 spp 16: about 10 % of the
    values differ, by at most 6e-8)."""
    if integrator != "direct":
        assert torch.equal(img, ref)
        return
    d = (img - ref).abs()
    print(f"[materials] direct: {int((d > 0).sum())} of {d.numel()} values differ, max {float(d.max()):.3g}")
    assert rel_l1(img, ref) <= 1e-6 and float(d.max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


def grads(scene, mats, seed=0, cot=None):
    d = [torch.zeros_like(m) for m in mats]
    cot = torch.ones((W, W, 4), device="cuda") if cot is None else cot
    scene.render_backward_materials(cot, d, list(mats), (W, W), SPP, seed)
    return d


@pytest.mark.parametrize("accel", ["auto", "bvh"])
@pytest.mark.parametrize("integrator", ["path", "direct", "collocated"])
def test_legacy_slot_table_renders_what_one_material_renders(integrator, accel, mat_a):
    scene = make_scene(integrator, accel=accel)
    ref = scene.render_forward(mat_a, (W, W), SPP, 3)
    gref = torch.zeros_like(mat_a)
    scene.render_backward(torch.ones((W, W, 4), device="cuda"), gref, mat_a, (W, W), SPP, 3)
    scene.material_slots = [0, 0] if integrator == "collocated" else [0, None]
    img = scene.render_forward_materials([mat_a], (W, W), SPP, 3)
    assert_same_image(img, ref, integrator)
    g, = grads(scene, [mat_a], 3)
    assert rel_l1(g, gref) <= 1e-6
    assert torch.equal(scene.render(mat_a, res=(W, W), spp=SPP, seed=3), img)   # a single tensor with slots set: a one-element list
    scene.check()


@pytest.mark.parametrize("accel", ["auto", "bvh"])
@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_a_mesh_split_in_two_instances_renders_as_it_did_whole(integrator, accel, mat_a):
    whole = make_scene(integrator, accel=accel)
    ref = whole.render_forward(mat_a, (W, W), SPP, 5)
    gref = torch.zeros_like(mat_a)
    whole.render_backward(torch.ones((W, W, 4), device="cuda"), gref, mat_a, (W, W), SPP, 5)
    split = make_scene(integrator, accel=accel, arrays=split_arrays())
    split.material_slots = [0, 0, None]
    img = split.render_forward_materials([mat_a], (W, W), SPP, 5)
    assert_same_image(img, ref, integrator)
    split.material_slots = [0, 1, None]
    assert torch.equal(split.render_forward_materials([mat_a, mat_a], (W, W), SPP, 5), img)
    g0, g1 = grads(split, [mat_a, mat_a], 5)
    assert g0.abs().sum() > 0 and g1.abs().sum() > 0          # both halves of the box are shaded, by their own material
    assert rel_l1(g0 + g1, gref) <= 1e-5
    split.check()


def _const(rgbr, h, w):
    return torch.tensor(rgbr, dtype=torch.float32, device="cuda").expand(h, w, 4).contiguous()


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_constant_materials_of_any_size_render_alike_in_every_cell_mode(integrator, small_a):
    scene = make_scene(integrator, arrays=split_arrays())
    scene.material_slots = [0, 1, None]
    c = (0.6, 0.3, 0.2, 0.5)
    # material A beside a constant one: cell copies of the total
    img1 = scene.render_forward_materials([small_a, _const(c, 1, 1)], (W, W), SPP, 2)
    img16 = scene.render_forward_materials([small_a, _const(c, 16, 16)], (W, W), SPP, 2)
    assert torch.equal(img1, img16)
    _, g1 = grads(scene, [small_a, _const(c, 1, 1)], 2)
    _, g16 = grads(scene, [small_a, _const(c, 16, 16)], 2)
    assert rel_l1(g16.sum((0, 1)), g1.sum((0, 1))) <= 1e-5
    # two small constants: 4 + 9 = 13 cells (the whole cell array in LDS) against 16 + 16 = 32 (cell copies)
    c2 = (0.3, 0.7, 0.4, 0.35)
    small = [_const(c, 1, 1), _const(c2, 2, 2)]
    tiled = [_const(c, 3, 3), _const(c2, 3, 3)]
    assert torch.equal(scene.render_forward_materials(small, (W, W), SPP, 4), scene.render_forward_materials(tiled, (W, W), SPP, 4))
    gs, gt = grads(scene, small, 4), grads(scene, tiled, 4)
    for a, b in zip(gt, gs):
        assert b.abs().sum() > 0
        assert rel_l1(a.sum((0, 1)), b.sum((0, 1))) <= 1e-5
    scene.check()


def directional(scene, mats, deltas, Wd, spp, seeds, wimg, eps=0.01):
    ad, fd = [], []
    for s in range(seeds):
        d = [torch.zeros_like(m) for m in mats]
        scene.render_backward_materials(wimg, d, mats, (Wd, Wd), spp, 7000 + s)
        ad.append(sum((g.double() * dl.double()).sum().item() for g, dl in zip(d, deltas)))
        ip = scene.render_forward_materials([m + eps * dl for m, dl in zip(mats, deltas)], (Wd, Wd), spp, 3000 + s).double()
        im = scene.render_forward_materials([m - eps * dl for m, dl in zip(mats, deltas)], (Wd, Wd), spp, 3000 + s).double()
        fd.append((((ip - im) * wimg.double()).sum() / (2 * eps)).item())
    ad, fd = np.array(ad), np.array(fd)
    sigma = np.hypot(ad.std(ddof=1), fd.std(ddof=1)) / np.sqrt(seeds)
    return ad.mean(), fd.mean(), sigma


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_gradient_of_the_second_material_matches_finite_differences(integrator):
    scene = make_scene(integrator, arrays=split_arrays())
    scene.material_slots = [0, 1, None]
    a = torch.from_numpy(fd_material_np(256, 0)).cuda()
    b = torch.from_numpy(fd_material_np(256, 1)).cuda()
    g = torch.Generator(device="cuda").manual_seed(11)
    Wd = 128
    wimg = torch.rand((Wd, Wd, 4), device="cuda", generator=g) + 0.5; wimg[..., 3] = 0
    db = torch.zeros_like(b); db[..., :3] = torch.rand(b[..., :3].shape, device="cuda", generator=g)
    da = torch.zeros_like(a); da[..., :3] = torch.rand(a[..., :3].shape, device="cuda", generator=g)
    for what, deltas in (("B only", [torch.zeros_like(a), db]), ("both", [da, db])):
        ad, fd, sigma = directional(scene, [a, b], deltas, Wd, 1024, 8, wimg)
        print(f"[fd] {integrator} {what}: AD {ad:.4f} FD {fd:.4f} rel {abs(ad - fd) / abs(fd):.2e} (1 sigma {sigma / abs(fd):.2e})")
        assert abs(fd) > 0
        assert abs(ad - fd) <= 1e-3 * abs(fd) + 3 * sigma
    scene.check()


def test_autograd_fills_each_material_and_replays_the_forward_slot_table(small_a):
    scene = make_scene("path", arrays=split_arrays())
    m0 = small_a.clone().requires_grad_()
    m1 = torch.from_numpy(fd_material_np(32, 1)).cuda().requires_grad_()
    scene.render([m0, m1], res=(W, W), spp=SPP, seed=1).sum().backward()   # default mapping: [0, 1, None]
    assert m0.grad is not None and m1.grad is not None
    r0, r1 = grads(scene, [m0.detach(), m1.detach()], 1)           # (atomics reorder the sums: equal to the last digits, not bit for bit)
    assert rel_l1(m0.grad, r0) <= 1e-6 and rel_l1(m1.grad, r1) <= 1e-6
    scene.check()
    # a material without requires_grad gets no .grad
    m0.grad = None
    fixed = m1.detach().clone()
    scene.render([m0, fixed], res=(W, W), spp=SPP, seed=1).sum().backward()
    assert fixed.grad is None and rel_l1(m0.grad, r0) <= 1e-6
    scene.check()
    # material_slots changed between forward and backward: the gradient is the forward table's
    m0.grad = m1.grad = None
    scene.material_slots = [0, 1, None]
    img = scene.render([m0, m1], res=(W, W), spp=SPP, seed=1)
    scene.material_slots = [1, 0, None]
    img.sum().backward()
    assert rel_l1(m0.grad, r0) <= 1e-6 and rel_l1(m1.grad, r1) <= 1e-6
    scene.check()
