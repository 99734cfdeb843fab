"""-m gpu: the texture-space views (Scene.texel_view, texel_gather, Scene.texel_project; include/zdr.h, zdr_scene_texel_view,
zdr_texel_gather, zdr_texel_gather_backward) against the float64 reference of tests/texel_project_ref.py on the cases of
tests/texel_project_cases.py, for both accelerators wherever a ray is traced, and the properties the header states: the round trip with
the renderer's own first hits, an exact family of the gather, the clamps, what lies behind an invisible texel, the adjoint as the
transpose, texel_project of one and two views, and the argument checks.

The kernels get the case's float32 sample points, the floats the reference was given.  A texel fails when ``visible`` differs from the
float64 reference or a continuous channel is off it by more than the case's bar (4 x the float32 reference's own error, floor 4
float32 ulps of the channel's largest value); failing and uncertain texels together may be 1 % of the reached ones.  Every figure is
printed before it is asserted."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import texel_cases as TC
import texel_lighting_cases as LC
import texel_project_cases as PC
import texel_project_ref as PR
from zdr_amd import Camera, Scene, TexelProjection, TexelView, float3, texel_gather, texel_gather_backward, texel_gather_forward
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -3            # ZDR_E_* of include/zdr.h
ACCELS = ["brute", "bvh"]

_scenes = {}


def camera(name):
    fov, o, t, up = PC.CAMERAS[name]
    return Camera(fov=fov, origin=float3(*o), target=float3(*t), up=float3(*up))


def case_scene(name, accel):
    make = LC.case(PC.case(name)[0])[0]
    if (make, accel) not in _scenes:
        scene = Scene(make(), integrator="direct", accel=accel)
        assert scene.info()["accel"] == accel
        _scenes[(make, accel)] = scene
    return _scenes[(make, accel)]


def case_points(name):
    return torch.from_numpy(PC.points(name)).cuda()


def run_case(name, accel, **kw):
    _, cam, res = PC.case(name)
    out = case_scene(name, accel).texel_view_forward(case_points(name), res, camera=camera(cam), **kw)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------- the view buffer
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", list(PC.CASES))
def test_view_parity_with_the_float64_reference(name, accel):
    got = run_case(name, accel).cpu().numpy()
    ref, reached = PC.reference(name), PC.reached(name)
    unc, keep = ref["uncertain"] & reached, PC.compared(name)
    fail = PC.failing(name, got) & keep
    err = np.abs(got.astype(np.float64) - ref["data"])[keep]
    print(f"[texel view parity] {name} {accel}: reached {int(reached.sum())}, uncertain {int(unc.sum())}, failing {int(fail.sum())} "
          f"(visible differs on {int(((got[..., 0] != ref['data'][..., 0]) & keep).sum())})")
    for c, (ch, bar, margin) in enumerate(zip(PC.CHANNELS, PC.bars(name), PC.MARGINS[name]), 1):
        print(f"    {ch}: kernel vs float64 largest {err[:, c].max():.3e}; float32 reference {margin:.3e}; bar {bar:.3e}")
    assert (got[~PR.shaded(PC.points(name))] == 0).all()
    assert (got[..., 7] == 0).all()
    assert int((fail | unc).sum()) <= PC.MAX_UNCERTAIN * reached.sum(), (name, accel, int(fail.sum()), int(unc.sum()))


@pytest.mark.parametrize("accel", ACCELS)
def test_round_trip_with_the_renderers_first_hits(accel):
    """render_aovs' position and normal of every pixel, fed back as surface points: each lands in its own pixel and sees the camera"""
    w, h = 24, 16
    scene = Scene(TC.cbox_arrays(), integrator="direct", accel=accel)
    scene.camera = camera("standard")
    scene.use_tent_filter = False
    f = scene.render_aovs(torch.rand(8, 8, 4, device="cuda"), res=(w, h), spp=1, seed=0)
    pts = torch.zeros(h, w, 16, device="cuda")
    pts[..., 4:7] = f.normal; pts[..., 8:11] = f.position; pts[..., 12] = (f.coverage == 1).float()
    got = scene.texel_view_forward(pts, (w, h)).cpu().numpy()
    hit = (f.coverage == 1).cpu().numpy()
    ref = PR.view_ref(pts.cpu().numpy(), PC.CAMERAS["standard"], (w, h), LC.oracle_scene(TC.cbox_arrays))
    exempt = PC.round_trip_exempt(ref, (w, h)) & hit
    ok = (got[..., 0] == 1) & (np.floor(got[..., 2]) == np.arange(w)[None, :]) & (np.floor(got[..., 3]) == np.arange(h)[:, None])
    print(f"[texel view round trip] {accel}: hit pixels {int(hit.sum())}, exempt {int(exempt.sum())}, failing {int((hit & ~ok & ~exempt).sum())}")
    assert hit.sum() > 300 and exempt.sum() < 0.01 * hit.sum()
    assert not (hit & ~ok & ~exempt).any()
    assert (got[~hit] == 0).all()
    scene.check()


@pytest.mark.parametrize("accel", ACCELS)
def test_two_runs_give_the_same_bits_whatever_the_buffers_held(accel):
    name = "cbox_64x64_inside"
    need = N.lib().zdr_texel_view_workspace_bytes(64, 64)
    a = run_case(name, accel, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda")).clone()
    b = run_case(name, accel, out=torch.full((64, 64, 8), 7.0, device="cuda"), workspace=torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda"))
    assert torch.equal(bits(a), bits(b)) and float(a[..., 0].sum()) > 0


def test_a_nan_in_a_position_gives_eight_zeros_and_leaves_the_others_alone():
    name = "cbox_16x16_standard"
    pts = case_points(name).clone()
    ys, xs = np.nonzero(PC.reached(name))
    pts[ys[0], xs[0], 9] = float("nan"); pts[ys[1], xs[1], 4] = float("nan")
    scene, (_, cam, res) = case_scene(name, "bvh"), PC.CASES[name]
    got, clean = scene.texel_view_forward(pts, res, camera=camera(cam)), run_case(name, "bvh")
    assert (got[ys[0], xs[0]] == 0).all() and (got[ys[1], xs[1]] == 0).all()
    mask = torch.ones(16, 16, dtype=torch.bool, device="cuda"); mask[ys[0], xs[0]] = False; mask[ys[1], xs[1]] = False
    assert torch.equal(bits(got[mask]), bits(clean[mask]))
    scene.check()


def test_the_high_level_call_is_the_low_level_call_on_the_scenes_texel_buffers():
    scene = Scene(TC.cbox_arrays(), integrator="direct")
    scene.camera = camera("standard")
    material = torch.rand(16, 16, 4, device="cuda")
    texels = scene.texel_aovs(material)
    view = scene.texel_view(material, res=(24, 16))
    assert isinstance(view, TexelView) and view.data.shape == (16, 16, 8) and view.pixel.shape == (16, 16, 2) and view.res == (24, 16)
    want = scene.texel_view_forward(texels.data, (24, 16))
    assert torch.equal(bits(view.data), bits(want)) and not view.data.requires_grad
    assert torch.equal(bits(scene.texel_view(material, res=(24, 16), texels=texels).data), bits(want))
    inside = scene.texel_view(material, res=(24, 16), camera=camera("inside"))
    assert torch.equal(bits(inside.data), bits(scene.texel_view_forward(texels.data, (24, 16), camera=camera("inside")))) and not torch.equal(inside.data, want)
    for k, ch in enumerate(("visible", "cosine")):
        assert torch.equal(getattr(view, ch), view.data[..., k])
    assert torch.equal(view.depth, view.data[..., 4]) and torch.equal(view.distance, view.data[..., 5]) and torch.equal(view.scale, view.data[..., 6])
    assert torch.equal(view.weight(2.0), view.visible * view.cosine.abs() ** 2.0)
    assert (view.data[texels.reach == 0] == 0).all() and float(view.visible.sum()) > 0
    scene.check()


# ------------------------------------------------------------------------------------------- the gather
def synthetic(rng, n, res, share=0.8):
    v = np.zeros((n, 1, 8), np.float32)
    v[:, 0, 0] = rng.uniform(0, 1, n) < share
    v[:, 0, 2] = rng.uniform(0, res[0], n); v[:, 0, 3] = rng.uniform(0, res[1], n)
    return v


def test_the_exact_family_the_clamps_and_what_lies_behind_an_invisible_texel():
    rng = np.random.default_rng(3)
    w, h = 24, 16
    image = torch.from_numpy(rng.normal(size=(h, w, 4)).astype(np.float32)).cuda()
    ys, xs = np.mgrid[0:h, 0:w]
    view = np.zeros((h, w, 8), np.float32)
    view[..., 0] = 1; view[..., 2] = xs + 0.5; view[..., 3] = ys + 0.5
    assert torch.equal(bits(texel_gather_forward(image, torch.from_numpy(view).cuda())), bits(image))
    one = torch.from_numpy(rng.normal(size=(1, 1, 4)).astype(np.float32)).cuda()
    v = synthetic(rng, 300, (1, 1))
    got = texel_gather_forward(one, torch.from_numpy(v).cuda())
    on = torch.from_numpy(v[:, 0, 0] == 1).cuda()
    assert torch.equal(bits(got[on, 0]), bits(one[0, 0].expand(int(on.sum()), 4))) and (got[~on] == 0).all()
    edge = np.zeros((4, 1, 8), np.float32)
    edge[:, 0, 0] = 1; edge[:, 0, 3] = 0.5
    edge[:, 0, 2] = [0.0, 0.5, w - 0.5, np.nextafter(np.float32(w), np.float32(0))]
    got = texel_gather_forward(image, torch.from_numpy(edge).cuda())
    assert torch.equal(bits(got[:2, 0]), bits(image[0, 0].expand(2, 4))) and torch.equal(bits(got[2:, 0]), bits(image[0, w - 1].expand(2, 4)))
    poisoned = image.clone(); poisoned[3, 4] = float("nan")
    v = view.copy(); v[2:5, 3:6, 0] = 0
    v[2, 3, 2:4] = (float("nan"), 1e30)                                                    # X, Y may hold anything there
    got = texel_gather_forward(poisoned, torch.from_numpy(v).cuda())
    assert not torch.isnan(got).any() and (got[2:5, 3:6] == 0).all()
    # the same bits from two runs into a dirty output
    again = texel_gather_forward(poisoned, torch.from_numpy(v).cuda(), out=torch.full((h, w, 4), float("nan"), device="cuda"))
    assert torch.equal(bits(got), bits(again))


@pytest.mark.parametrize("name", ["cbox_64x64_standard", "cbox_64x64_inside", "cbox_64x64_inside_1x1"])
def test_gather_and_adjoint_parity_on_the_kernels_own_view_buffer(name):
    res = PC.CASES[name][2]
    view = run_case(name, "bvh")
    rng = np.random.default_rng(17)
    image, g = rng.uniform(0, 1, (res[1], res[0], 4)).astype(np.float32), rng.normal(size=(64, 64, 4)).astype(np.float32)
    v = view.cpu().numpy()
    bar, ref = PC.linear_bar(v, image, res, False)
    got = texel_gather_forward(torch.from_numpy(image).cuda(), view).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"[texel gather parity] {name}: visible {int(v[..., 0].sum())}; kernel vs float64 {err:.3e}; bar {bar:.3e}")
    assert float(np.abs(got).sum()) > 0 and err <= bar
    bar, ref = PC.linear_bar(v, g, res, True)
    d = texel_gather_backward(torch.from_numpy(g).cuda(), view, res).cpu().numpy()
    err = float(np.abs(d - ref).max())
    print(f"[texel gather adjoint parity] {name}: kernel vs float64 transpose {err:.3e}; bar {bar:.3e}; largest |d_image| {np.abs(ref).max():.3e}")
    assert err <= bar
    # it adds into what d_image holds
    base = torch.from_numpy(rng.normal(size=(res[1], res[0], 4)).astype(np.float32)).cuda()
    into = texel_gather_backward(torch.from_numpy(g).cuda(), view, res, d_image=base.clone()).cpu().numpy()
    err = float(np.abs(into - (base.cpu().numpy().astype(np.float64) + ref)).max())
    print(f"[texel gather adjoint parity] {name}: into a non-zero d_image {err:.3e}; bar {bar + 4 * PC.EPS32 * float(np.abs(into).max()):.3e}")
    assert err <= bar + PC.FLOOR_ULPS * PC.EPS32 * float(np.abs(into).max())              # (the base's own rounding: one more addition)


def test_the_gradient_passes_through_texel_gather_and_is_zero_where_nothing_taps():
    name = "cbox_64x64_standard"
    res = PC.CASES[name][2]
    view = run_case(name, "bvh")
    view[..., 0] *= (view[..., 2] < 11.0)                         # nothing visible taps the pixels x >= 12 any more
    gen = torch.Generator().manual_seed(2)
    image = torch.rand(res[1], res[0], 4, generator=gen).cuda().requires_grad_()
    y = torch.randn(64, 64, 4, generator=gen).cuda()
    out = texel_gather(image, view)
    assert out.requires_grad
    out.backward(y)
    dx = torch.randn(res[1], res[0], 4, generator=gen).cuda()
    lhs = float((texel_gather_forward(dx, view).double() * y.double()).sum())
    rhs = float((dx.double() * image.grad.double()).sum())
    print(f"[texel gather dot product] <K dx, y> = {lhs:.9e}, <dx, K^T y> = {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))
    assert (image.grad[:, 12:] == 0).all() and float(image.grad[:, :11].abs().sum()) > 0
    vg = view.clone().requires_grad_()
    assert torch.autograd.grad(texel_gather(image, vg).sum(), [image, vg], allow_unused=True)[1] is None      # the view receives none


# ------------------------------------------------------------------------------------------- texel_project
def test_texel_project_of_one_and_of_two_views():
    scene = Scene(TC.cbox_arrays(), integrator="direct")
    scene.camera = camera("standard")
    material = torch.rand(64, 64, 4, device="cuda")
    texels = scene.texel_aovs(material)
    gen = torch.Generator().manual_seed(4)
    photo = torch.rand(16, 24, 4, generator=gen).cuda().requires_grad_()
    other = torch.rand(20, 30, 4, generator=gen).cuda()
    one = scene.texel_project([(camera("standard"), photo)], material, texels=texels)
    assert isinstance(one, TexelProjection) and one.color.shape == (64, 64, 4) and one.weight.shape == (64, 64) and one.count.shape == (64, 64)
    view = scene.texel_view(material, res=(24, 16), texels=texels)
    w = view.weight()
    seen = w > 0
    want = torch.where(seen[..., None], w[..., None] * view.gather(photo) / torch.where(seen, w, torch.ones_like(w))[..., None], torch.zeros(64, 64, 4, device="cuda"))
    assert torch.equal(bits(one.color.detach()), bits(want.detach())) and torch.equal(one.weight, w) and torch.equal(one.count, view.visible)
    one.color.sum().backward()
    assert float(photo.grad.abs().sum()) > 0
    two = scene.texel_project([(camera("standard"), photo.detach()), (camera("inside"), other)], material, cosine_power=2.0, texels=texels)
    assert sorted(torch.unique(two.count).tolist()) == [0.0, 1.0, 2.0]
    assert (two.color[two.weight == 0] == 0).all() and torch.isfinite(two.color).all()
    filled = scene.texel_project([(camera("standard"), photo.detach()), (camera("inside"), other)], material, cosine_power=2.0, fill=True, texels=texels)
    keep = two.weight > 0
    assert torch.equal(bits(filled.color[keep]), bits(two.color[keep])) and float(filled.color[~keep].abs().sum()) > 0
    scene.check()


# ------------------------------------------------------------------------------------------- errors
def test_wrong_arguments_raise():
    name = "cbox_16x16_standard"
    scene, pts = case_scene(name, "brute"), case_points(name)
    L = N.lib()
    need = L.zdr_texel_view_workspace_bytes(16, 16)
    assert need >= 16 * 16 * 4 and L.zdr_texel_view_workspace_bytes(0, 16) == 0 and L.zdr_texel_view_workspace_bytes(16, -1) == 0
    with pytest.raises(ValueError):
        scene.texel_view_forward(pts[..., :4].contiguous(), (24, 16))
    with pytest.raises(ValueError):
        scene.texel_view_forward(pts.double(), (24, 16))
    with pytest.raises(ValueError):
        scene.texel_view_forward(pts, (24, 0))
    with pytest.raises(ValueError):
        scene.texel_view_forward(pts, (24, 16), out=torch.zeros(16, 16, 4, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_view_forward(pts, (24, 16), workspace=torch.zeros(need - 1, dtype=torch.uint8, device="cuda"))
    for fov in (0.0, -1.0, 3.2, float("nan"), float("inf")):
        with pytest.raises(N.ZdrError):
            scene.texel_view_forward(pts, (24, 16), camera=Camera(fov=fov, origin=float3(0, 0, 5), target=float3(0, 0, 0), up=float3(0, 1, 0)))
    view = scene.texel_view_forward(pts, (24, 16), camera=camera("standard"))
    image = torch.rand(16, 24, 4, device="cuda")
    with pytest.raises(ValueError):
        texel_gather_forward(image[..., :3].contiguous(), view)
    with pytest.raises(ValueError):
        texel_gather_forward(image.cpu(), view)
    with pytest.raises(ValueError):
        texel_gather_forward(image, view[..., :4].contiguous())
    with pytest.raises(ValueError):
        texel_gather_forward(image, view, out=torch.zeros(16, 16, 3, device="cuda"))
    with pytest.raises(ValueError):
        texel_gather_backward(torch.rand(8, 8, 4, device="cuda"), view, (24, 16))
    with pytest.raises(ValueError):
        texel_gather_backward(torch.rand(16, 16, 4, device="cuda"), view, (24, 16), d_image=torch.zeros(24, 16, 4, device="cuda"))
    with pytest.raises(ValueError):
        TexelView(view, (24, 16)).gather(torch.rand(24, 16, 4, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_project([], torch.rand(16, 16, 4, device="cuda"))
    # the C entry points themselves
    out = torch.zeros(16, 16, 8, device="cuda"); ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    from zdr_amd.render import _camera_pod

    def vparams(**kw):
        p = N.TexelViewParams()
        p.struct_size = C.sizeof(N.TexelViewParams)
        p.tex_h, p.tex_w, p.width, p.height, p.camera = 16, 16, 24, 16, _camera_pod(camera("standard"))
        for k, v in kw.items():
            if k == "fov":
                p.camera.fov = v
            else:
                setattr(p, k, v)
        return p

    def vcall(p, off=(0, 0, 0)):
        return L.zdr_scene_texel_view(scene._handle, C.byref(p), pts.data_ptr() + off[0], out.data_ptr() + off[1], ws.data_ptr() + off[2], scene._stream())
    assert vcall(vparams()) == 0
    for bad in (vparams(struct_size=4), vparams(tex_h=0), vparams(tex_w=-1), vparams(width=0), vparams(height=-3), vparams(fov=0.0), vparams(fov=3.1416),
                vparams(fov=float("nan")), vparams(fov=float("inf")), vparams(fov=-0.5)):
        assert vcall(bad) == E_INVALID
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        assert vcall(vparams(), off=off) == E_INVALID
    assert L.zdr_scene_texel_view(scene._handle, C.byref(vparams()), pts.data_ptr(), None, ws.data_ptr(), scene._stream()) == E_INVALID
    assert L.zdr_scene_texel_view(None, C.byref(vparams()), pts.data_ptr(), out.data_ptr(), ws.data_ptr(), scene._stream()) == E_INVALID
    big = torch.zeros(16 * 16 * 8 + need // 4 + 64, device="cuda")                          # out and workspace in one buffer
    assert L.zdr_scene_texel_view(scene._handle, C.byref(vparams()), pts.data_ptr(), big.data_ptr(), big.data_ptr() + 16, scene._stream()) == E_INVALID
    assert L.zdr_scene_texel_view(scene._handle, C.byref(vparams()), pts.data_ptr(), pts.data_ptr() + 64, ws.data_ptr(), scene._stream()) == E_INVALID
    assert L.zdr_scene_texel_view(scene._handle, C.byref(vparams()), pts.data_ptr(), out.data_ptr(), pts.data_ptr() + 64, scene._stream()) == E_INVALID

    def gparams(**kw):
        p = N.TexelGatherParams()
        p.struct_size = C.sizeof(N.TexelGatherParams)
        p.tex_h, p.tex_w, p.width, p.height = 16, 16, 24, 16
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    color, d_image, stream = torch.zeros(16, 16, 4, device="cuda"), torch.zeros(16, 24, 4, device="cuda"), scene._stream()
    assert L.zdr_texel_gather(C.byref(gparams()), view.data_ptr(), image.data_ptr(), color.data_ptr(), stream) == 0
    assert L.zdr_texel_gather_backward(C.byref(gparams()), view.data_ptr(), color.data_ptr(), d_image.data_ptr(), stream) == 0
    for fn, src, dst in ((L.zdr_texel_gather, image, color), (L.zdr_texel_gather_backward, color, d_image)):
        for bad in (gparams(struct_size=8), gparams(tex_h=0), gparams(width=0), gparams(height=-1)):
            assert fn(C.byref(bad), view.data_ptr(), src.data_ptr(), dst.data_ptr(), stream) == E_INVALID
        assert fn(C.byref(gparams()), view.data_ptr() + 4, src.data_ptr(), dst.data_ptr(), stream) == E_INVALID
        assert fn(C.byref(gparams()), view.data_ptr(), src.data_ptr() + 8, dst.data_ptr(), stream) == E_INVALID
        assert fn(C.byref(gparams()), view.data_ptr(), src.data_ptr(), None, stream) == E_INVALID
        assert fn(None, view.data_ptr(), src.data_ptr(), dst.data_ptr(), stream) == E_INVALID
        assert fn(C.byref(gparams()), view.data_ptr(), src.data_ptr(), src.data_ptr(), stream) == E_INVALID           # the output aliases the input
        assert fn(C.byref(gparams()), view.data_ptr(), src.data_ptr(), view.data_ptr() + 64, stream) == E_INVALID
    torch.cuda.synchronize()
    scene.check()


# ------------------------------------------------------------------------------------------- the example
def test_the_example_can_start_from_the_target():
    spec = importlib.util.spec_from_file_location("optimize_texture_project", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "optimize_texture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    losses = ex.run(iters=2, res=32, spp=4, tex=32, init_from_target=True, verbose=False)
    plain = ex.run(iters=2, res=32, spp=4, tex=32, verbose=False)
    print(f"[texel project example] first-iteration loss from the target {losses[0]:.5f}, from noise {plain[0]:.5f} (reported, not asserted)")
    assert len(losses) == 2 and np.isfinite(losses).all()
