"""-m gpu: first-hit feature buffers (Scene.render_aovs; include/zdr.h, zdr_render_aovs / zdr_render_aovs_backward).

The forward is a deterministic function of the camera samples: it is checked sample by sample against a reference built here from the
oracle's own pieces (its sampler draws, zdro_generate_ray, trace_closest, zdro_read_bsdf) and, for the hits the path kernels shade, against
zdr_path_dump.  The albedo / roughness channels are exactly linear in the materials, so the backward is checked by the adjoint identity
<g, A(m + D) - A(m)> = <A^T g, D>, which holds without any Monte Carlo noise (tests/test_gpu_envmap_grad.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from conftest import cbox_material_np, cbox_models, fd_material_np
from gpu_util import make_scene, multi_light_arrays, oracle_params
from zdr_amd import _native as N
from zdr_amd import geometry

pytestmark = pytest.mark.gpu

CH = 16


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


_PMJ = {}


def use_small_pmj_tables(scene):
    """The small PMJ02bn tables of the other gradient tests, on the scene and in the oracle (whose tables are global state)."""
    from zdr_amd import pmj02bn_tables as T
    if not _PMJ:
        _PMJ["pmj"] = T.pmj02_sets(n_sets=5, n_samples=256, seed=2)
        _PMJ["bn"] = T.blue_noise_textures(n_tex=4, res=32, seed=2)
    pmj, bn = _PMJ["pmj"], _PMJ["bn"]
    scene.sampler = "pmj02bn"
    scene.set_pmj02bn_tables(pmj, bn)
    oracle.lib().zdro_set_pmj02bn_tables(pmj.ctypes.data_as(C.POINTER(C.c_uint32)), 5, 256, bn.ctypes.data_as(C.POINTER(C.c_uint16)), 4, 32)


def build_scene(name, accel="auto", sampler="cmj", integrator="path"):
    scene = make_scene(integrator, accel=accel, arrays=multi_light_arrays() if name == "lights" else geometry.assemble(cbox_models()))
    if sampler == "pmj02bn":
        use_small_pmj_tables(scene)
    return scene


# ------------------------------------------------------------------------------------------ the reference
def tent(u):
    """camera.py:20-31 with radius 1, in float32"""
    u = u.astype(np.float32)
    one, two, half = np.float32(1.0), np.float32(2.0), np.float32(0.5)
    with np.errstate(invalid="ignore"):
        return np.where(u < half, np.sqrt(two * u) - one, one - np.sqrt(two - two * u)).astype(np.float32)


def reference(scene, mats, slots, W, H, spp, seed):
    """The (H, W, 16) buffers of include/zdr.h's table from the oracle's pieces; per sample in float64, summed in sample order."""
    A = scene._arrays
    S = oracle.OracleScene.from_arrays(A)
    kind = oracle.SAMPLER_PMJ02BN if scene.sampler == "pmj02bn" else oracle.SAMPLER_CMJ
    L = oracle.lib()
    P = oracle_params(scene, W, H, spp, seed, (1, 1), sampler=kind)
    n = W * H * spp
    xs = np.empty(n, np.int32); ys = np.empty(n, np.int32); jit = np.empty((n, 2), np.float32)
    k = 0
    for y in range(H):
        for x in range(W):
            for s in range(spp):
                xs[k], ys[k] = x, y
                jit[k] = oracle.sampler_dump(kind, x, y, seed, spp, s, nvert=1)[:2]
                k += 1
    off = jit
    if scene.use_tent_filter:
        off = np.stack([tent(jit[:, 0]) + np.float32(0.5), tent(jit[:, 1]) + np.float32(0.5)], -1).astype(np.float32)
    fx = xs.astype(np.float32) + off[:, 0]; fy = ys.astype(np.float32) + off[:, 1]
    ndx = (np.float32(2.0) / np.float32(W)) * fx - np.float32(1.0)
    ndy = ((np.float32(2.0) / np.float32(H)) * fy - np.float32(1.0)) * (np.float32(H) / np.float32(W))
    rays = np.zeros((n, 8), np.float32)
    o = (C.c_float * 3)(); d = (C.c_float * 3)()
    for k in range(n):
        L.zdro_generate_ray(C.byref(P), float(ndx[k]), float(ndy[k]), o, d)
        rays[k, 0:3] = o[:]; rays[k, 4:7] = d[:]
    rays[:, 7] = 1e30
    ip, bt = S.trace_closest(rays)
    M = A.inst_xform.reshape(-1, 4, 4).astype(np.float64)
    NM = np.stack([np.linalg.inv(m[:3, :3]).T for m in M])               # normals go through the inverse transpose (scene.h, shade record)
    mats64 = [np.ascontiguousarray(m, np.float32) for m in mats]
    out = np.zeros((H, W, CH), np.float64)
    out[..., 14:] = -1.0
    texel = (C.c_float * 4)()
    for k in range(n):
        inst, prim = int(ip[k, 0]), int(ip[k, 1])
        if inst < 0:
            continue
        u, v, t = (float(c) for c in bt[k])
        tri = A.tris[int(A.inst_tri_begin[inst]) + prim]
        a, b, c = (A.verts[i].astype(np.float64) for i in tri)
        w0 = 1.0 - u - v
        m = M[inst]
        p = m[:3, :3] @ (w0 * a[0:3] + u * b[0:3] + v * c[0:3]) + m[:3, 3]
        uv = w0 * a[3:5] + u * b[3:5] + v * c[3:5]
        ns = NM[inst] @ (w0 * a[5:8] + u * b[5:8] + v * c[5:8])
        ns /= np.linalg.norm(ns)
        slot = -1 if slots[inst] is None else int(slots[inst])
        px = out[ys[k], xs[k]]
        if slot >= 0:
            tex = mats64[slot]
            L.zdro_read_bsdf(tex.ctypes.data_as(C.POINTER(C.c_float)), tex.shape[0], tex.shape[1], float(np.float32(uv[0])), float(np.float32(uv[1])), texel)
            px[0:4] += np.array(texel[:], np.float64)
        px[4:7] += ns; px[7] += t; px[8:11] += p; px[11] += 1.0; px[12:14] += uv
        if px[14] < 0:
            px[14], px[15] = inst, slot
    out[..., :14] /= spp
    assert np.isfinite(out).all()
    return out


def assert_matches_reference(got, ref, what):
    """The project's image bar (gpu_util.image_diff_stats) for every pixel and channel, instance and slot exactly; at most 2 pixels
    may miss it: a camera sample within an ulp of a silhouette edge may land on the other side."""
    got = np.asarray(got, np.float64)
    bad = (np.abs(got[..., :14] - ref[..., :14]) > 1e-4 * (1.0 + np.abs(ref[..., :14]))).any(-1)
    bad |= (got[..., 14] != ref[..., 14]) | (got[..., 15] != ref[..., 15])
    worst = float((np.abs(got[..., :14] - ref[..., :14]) / (1.0 + np.abs(ref[..., :14])))[~bad].max())
    print(f"[aovs] {what}: {int(bad.sum())} of {bad.size} pixels miss the bar; the others are within {worst:.3g} (1 + |ref|); "
          f"coverage < 1 in {int((ref[..., 11] < 1).sum())} pixels, slot -1 first in {int(((ref[..., 15] < 0) & (ref[..., 14] >= 0)).sum())}, "
          f"instances seen {sorted(set(ref[..., 14].astype(int).ravel()) - {-1})}")
    assert int(bad.sum()) <= 2, (what, np.argwhere(bad)[:8].tolist())


_REFERENCES = {}
FORWARD_CASES = [(33, 21, 4, 3, True), (33, 21, 4, 3, False), (32, 32, 16, 6, True)]


@pytest.mark.parametrize("accel", ["brute", "bvh"])
@pytest.mark.parametrize("W,H,spp,seed,use_tent", FORWARD_CASES)
@pytest.mark.parametrize("material", ["a", "b"])
@pytest.mark.parametrize("name", ["cbox", "lights"])
def test_forward_matches_the_oracle_sample_by_sample(name, material, W, H, spp, seed, use_tent, accel):
    scene = build_scene(name, accel)
    scene.use_tent_filter = use_tent
    mat = cbox_material_np() if material == "a" else fd_material_np(64, 0)
    got = scene.render_aovs_forward(cuda(mat), (W, H), spp, seed).cpu().numpy()
    scene.check()
    slots = (0,) + (None,) * (scene.inst_count - 1)
    key = (name, material, W, H, spp, seed, use_tent)                    # the reference does not depend on the accelerator: built once
    if key not in _REFERENCES:
        _REFERENCES[key] = reference(scene, [mat], slots, W, H, spp, seed)
    ref = _REFERENCES[key]
    assert (ref[..., 11] < 1).any() and (ref[..., 15] < 0).any()         # misses and hits without a material are both in view
    if name == "lights":
        assert set(ref[..., 14].astype(int).ravel()) >= {0, 1, 2, 3, 4}  # all five instances are seen
    assert_matches_reference(got, ref, f"{name} {W}x{H} spp {spp} tent {use_tent} {accel}")


def test_forward_matches_the_oracle_with_pmj02bn():
    scene = build_scene("cbox", "brute", sampler="pmj02bn")
    mat = fd_material_np(64, 0)
    got = scene.render_aovs_forward(cuda(mat), (33, 21), 4, 3).cpu().numpy()
    scene.check()
    assert_matches_reference(got, reference(scene, [mat], (0, None), 33, 21, 4, 3), "cbox pmj02bn")


def test_forward_with_two_materials_matches_the_oracle():
    """(beyond the single-material cases: every slot of a table reads its own texture, and the slot channel says which)"""
    scene = make_scene("direct", arrays=split_arrays())
    mats = [fd_material_np(64, 0), fd_material_np(16, 1)]
    slots = (0, 1, None)
    got = scene.render_aovs_forward([cuda(m) for m in mats], (33, 21), 4, 3, slots=slots).cpu().numpy()
    scene.check()
    ref = reference(scene, mats, slots, 33, 21, 4, 3)
    assert {0.0, 1.0, -1.0} <= set(ref[..., 15].ravel())
    assert_matches_reference(got, ref, "split cbox, two materials")


def split_arrays():
    from test_gpu_materials import split_arrays as f
    return f()


# --------------------------------------------------------------------------- cross-check with the path kernels
def test_uv_and_instance_are_those_of_the_path_kernels_first_vertex():
    from path_trace import Trace, all_queries
    W = 32
    scene = build_scene("cbox")
    scene.use_tent_filter = False
    mat = cuda(cbox_material_np())
    f = scene.render_aovs_forward(mat, (W, W), 1, 4).cpu().numpy()
    q = all_queries(W, W, 1)
    tr = Trace(scene.path_dump(mat, torch.from_numpy(q).cuda(), (W, W), 1, 4).cpu().numpy())
    scene.check()
    cov = f[..., 11]
    assert np.isin(cov, (0.0, 1.0)).all()
    shaded = tr.live[:, 0]                                               # the path has at least one vertex
    assert shaded.sum() > 0.5 * q.shape[0]
    x, y = q[shaded, 0], q[shaded, 1]
    assert (cov[y, x] == 1.0).all()
    assert (f[y, x, 14] == tr.inst[shaded, 0]).all()
    assert np.abs(f[y, x, 12:14] - tr.uv[shaded, 0]).max() <= 1e-5       # a value in [0, 1] from three products: about 100 ulp


# ------------------------------------------------------------------------------------------------ adjoint
def adjoint(scene, mats, slots, W, H, spp, seed, gseed=0, g=None):
    """(lhs, rhs, gradients): <g, A(m + D) - A(m)> and <A^T g, D> in float64, g a random cotangent with all 16 channels non-zero.
    D is random and POSITIVE, like the direction of tests/test_gpu_envmap_grad.py.  The left side is a difference of two float32
    buffers: each of its W H 4 material entries (values near 0.5) carries a rounding error of about 3e-8 whatever D is, about 4e-6
    in the sum (measured: 4.1e-6 on 32 x 32).  A D of both signs is averaged away by the bilinear lookups and the 16 samples of a
    pixel — on 32 x 32, spp 16 the sum came out at -0.0109722 where the float64 reference() of this file gives -0.0109688 and the
    backward -0.0109681: the rounding of the left side alone is 3.7e-4 of such a sum — while a positive D moves every entry the
    same way and leaves sums between 2 and 3.4 in every case below, on which the identity can be read to the 1e-4 it is held to."""
    rng = np.random.default_rng(gseed)
    if g is None:
        g = rng.normal(size=(H, W, CH)).astype(np.float32)
    D = [cuda(rng.uniform(0.0, 0.1, tuple(m.shape))) for m in mats]
    kw = dict(slots=slots) if slots is not None else {}
    a1 = scene.render_aovs_forward([m + d for m, d in zip(mats, D)], (W, H), spp, seed, **kw).double().cpu().numpy()
    a0 = scene.render_aovs_forward(list(mats), (W, H), spp, seed, **kw).double().cpu().numpy()
    lhs = float((g.astype(np.float64) * (a1 - a0)).sum())
    dm = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(cuda(g), dm, list(mats), (W, H), spp, seed, **kw)
    torch.cuda.synchronize()
    rhs = float(sum((a.double() * d.double()).sum() for a, d in zip(dm, D)))
    return lhs, rhs, dm


ADJOINT_CASES = [("brute", "cmj", 32, 32, 16, 64), ("bvh", "cmj", 32, 32, 16, 64), ("brute", "pmj02bn", 32, 32, 16, 64), ("brute", "cmj", 33, 21, 4, 64),
                 ("brute", "cmj", 32, 32, 16, 1), ("brute", "cmj", 32, 32, 16, 4)]


@pytest.mark.parametrize("accel,sampler,W,H,spp,tex", ADJOINT_CASES)
def test_adjoint_identity(accel, sampler, W, H, spp, tex):
    scene = build_scene("cbox", accel, sampler)
    lhs, rhs, (dm,) = adjoint(scene, [cuda(fd_material_np(tex, 0))], None, W, H, spp, 5)
    scene.check()
    print(f"[aovs] adjoint {accel} {sampler} {W}x{H} spp {spp} texture {tex}: lhs {lhs:.9g} rhs {rhs:.9g} rel {rel(lhs, rhs):.3g}")
    assert abs(lhs) > 1e-3, lhs
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


def test_adjoint_identity_with_two_materials():
    scene = make_scene("path", arrays=split_arrays())
    mats = [cuda(fd_material_np(64, 0)), cuda(fd_material_np(16, 1))]
    lhs, rhs, dm = adjoint(scene, mats, [0, 1, None], 32, 32, 16, 5)
    scene.check()
    print(f"[aovs] adjoint two materials: lhs {lhs:.9g} rhs {rhs:.9g} rel {rel(lhs, rhs):.3g}")
    assert all(float(d.abs().sum()) > 0.0 for d in dm)
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)


def test_gradient_is_zero_where_nothing_depends_on_the_material_and_accumulates():
    W, spp, seed = 32, 16, 5
    # a material that no instance in view reads (slot 1 is given to nobody) receives exactly nothing
    scene = make_scene("path", arrays=split_arrays())
    mats = [cuda(fd_material_np(64, 0)), cuda(fd_material_np(16, 1))]
    g = np.random.default_rng(1).normal(size=(W, W, CH)).astype(np.float32)
    dm = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(cuda(g), dm, mats, (W, W), spp, seed, slots=[0, None, None])
    assert float(dm[0].abs().sum()) > 0.0 and float(dm[1].abs().max()) == 0.0
    # channels 4..15 alone carry no gradient
    g[..., :4] = 0.0
    dz = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(cuda(g), dz, mats, (W, W), spp, seed, slots=[0, 1, None])
    assert all(float(d.abs().max()) == 0.0 for d in dz)
    # += : a second call into the same tensors doubles them
    g = cuda(np.random.default_rng(2).normal(size=(W, W, CH)))
    once = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(g, once, mats, (W, W), spp, seed, slots=[0, 1, None])
    twice = [d.clone() for d in once]
    scene.render_aovs_backward(g, twice, mats, (W, W), spp, seed, slots=[0, 1, None])
    for a, b in zip(once, twice):
        torch.testing.assert_close(b, 2.0 * a, rtol=1e-5, atol=1e-6 * float(a.abs().max()))
    # a NaN cotangent counts as 0
    gn = g.clone(); gn[3, 5, 1] = float("nan")
    gz = g.clone(); gz[3, 5, :4] = 0.0
    a = [torch.zeros_like(m) for m in mats]; b = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(gn, a, mats, (W, W), spp, seed, slots=[0, 1, None])
    scene.render_aovs_backward(gz, b, mats, (W, W), spp, seed, slots=[0, 1, None])
    for x, y in zip(a, b):
        assert torch.isfinite(x).all()
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6 * float(y.abs().max()))
    scene.check()


# ----------------------------------------------------------------------------------------------- autograd
def test_autograd_is_the_low_level_backward():
    W, spp, seed = 32, 16, 7
    scene = build_scene("cbox")
    m = cuda(fd_material_np(64, 0)).requires_grad_()
    before = scene.render(m.detach(), res=(W, W), spp=spp, seed=seed)
    f = scene.render_aovs(m, res=(W, W), spp=spp, seed=seed)
    assert f.data.shape == (W, W, CH) and f.albedo.shape == (W, W, 3) and f.normal.shape == (W, W, 3) and f.position.shape == (W, W, 3)
    assert f.uv.shape == (W, W, 2) and all(getattr(f, k).shape == (W, W) for k in ("roughness", "depth", "coverage", "instance", "slot"))
    assert torch.equal(f.depth, f.data[..., 7]) and torch.equal(f.slot, f.data[..., 15])
    f.albedo.sum().backward()
    g = torch.zeros((W, W, CH), device="cuda"); g[..., :3] = 1.0
    d = torch.zeros_like(m)
    scene.render_aovs_backward(g, d, m.detach(), (W, W), spp, seed)
    assert float(d.abs().sum()) > 0.0
    torch.testing.assert_close(m.grad, d, rtol=1e-5, atol=1e-6 * float(d.abs().max()))
    # the slot upload of render_aovs does not leak into the single-material path
    assert torch.equal(scene.render(m.detach(), res=(W, W), spp=spp, seed=seed), before)
    # any integrator gives the same buffers
    other = build_scene("cbox", integrator="collocated")
    assert torch.equal(other.render_aovs(m.detach(), res=(W, W), spp=spp, seed=seed).data, f.data.detach())
    scene.check(); other.check()


def test_autograd_hands_each_material_of_a_list_its_gradient_and_replays_the_camera():
    W, spp, seed = 32, 16, 7
    scene = make_scene("path", arrays=split_arrays())
    scene.material_slots = [0, 1, None]
    mats = [cuda(fd_material_np(64, 0)).requires_grad_(), cuda(fd_material_np(16, 1)).requires_grad_()]
    cot = cuda(np.random.default_rng(3).normal(size=(W, W, CH)))
    f = scene.render_aovs(mats, res=(W, W), spp=spp, seed=seed)
    camera = scene.camera.copy()
    scene.camera.origin = type(camera.origin)(1.0, 2.0, 5.0)             # moved between forward and backward: the snapshot is replayed
    (f.data * cot).sum().backward()
    d = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(cot, d, [m.detach() for m in mats], (W, W), spp, seed, camera=camera)
    moved = [torch.zeros_like(m) for m in mats]
    scene.render_aovs_backward(cot, moved, [m.detach() for m in mats], (W, W), spp, seed)
    for m, a, b in zip(mats, d, moved):
        assert float(a.abs().sum()) > 0.0
        torch.testing.assert_close(m.grad, a, rtol=1e-5, atol=1e-6 * float(a.abs().max()))
        assert not torch.allclose(a, b, rtol=1e-3, atol=1e-6 * float(a.abs().max()))
    scene.check()


# ------------------------------------------------------------------------------------ shards and arguments
def test_shards_partition_the_buffers_and_a_rectangle_leaves_the_rest_alone():
    W, H, spp, seed = 40, 24, 4, 2
    scene = build_scene("cbox")
    m = cuda(fd_material_np(64, 0))
    whole = scene.render_aovs_forward(m, (W, H), spp, seed)
    out = torch.full((H, W, CH), 7.0, device="cuda")
    for r in range(4):
        scene.render_aovs_forward(m, (W, H), spp, seed, tile_shard=(r, 4), out=out)
    assert torch.equal(out, whole)
    out = torch.full((H, W, CH), 7.0, device="cuda")
    scene.render_aovs_forward(m, (W, H), spp, seed, rect=(3, 5, 29, 20), out=out)
    inside = torch.zeros((H, W), dtype=torch.bool, device="cuda"); inside[5:20, 3:29] = True
    assert torch.equal(out[inside], whole[inside]) and bool((out[~inside] == 7.0).all())
    # the backward honours them too: the shards' gradients add up to the whole
    g = cuda(np.random.default_rng(4).normal(size=(H, W, CH)))
    full = torch.zeros_like(m); parts = torch.zeros_like(m)
    scene.render_aovs_backward(g, full, m, (W, H), spp, seed)
    for r in range(4):
        scene.render_aovs_backward(g, parts, m, (W, H), spp, seed, tile_shard=(r, 4))
    torch.testing.assert_close(parts, full, rtol=1e-4, atol=1e-6 * float(full.abs().max()))
    scene.check()


def test_arguments_are_checked():
    W, spp = 16, 4
    scene = build_scene("cbox")
    L = N.lib()
    m = cuda(fd_material_np(16, 0))
    for bad in (torch.zeros((W, W, 4), device="cuda"), torch.zeros((W, W, CH), device="cuda", dtype=torch.float64), torch.zeros((W, W, CH))):
        with pytest.raises(ValueError, match="out must be"):
            scene.render_aovs_forward(m, (W, W), spp, 0, out=bad)
    out = torch.zeros((W, W, CH), device="cuda")
    dims = np.array([[16, 16]], np.int32)
    p = scene._params((W, W), spp, 0, (1, 1))
    scene._upload_slots((0, None))
    assert L.zdr_render_aovs(scene._handle, C.byref(p), m.data_ptr(), dims.ctypes.data, 1, out.data_ptr(), scene._stream()) == 0
    # a sample sub-range is refused: the instance channel has no partial form
    p = scene._params((W, W), spp, 0, (1, 1), samples=(0, 2))
    assert L.zdr_render_aovs(scene._handle, C.byref(p), m.data_ptr(), dims.ctypes.data, 1, out.data_ptr(), scene._stream()) == -3
    d = torch.zeros_like(m)
    assert L.zdr_render_aovs_backward(scene._handle, C.byref(p), out.data_ptr(), m.data_ptr(), dims.ctypes.data, 1, d.data_ptr(), scene._stream()) == -3
    # nmat = 0, and a slot >= nmat
    p = scene._params((W, W), spp, 0, (1, 1))
    assert L.zdr_render_aovs(scene._handle, C.byref(p), m.data_ptr(), dims.ctypes.data, 0, out.data_ptr(), scene._stream()) == -1
    assert L.zdr_render_aovs_backward(scene._handle, C.byref(p), out.data_ptr(), m.data_ptr(), dims.ctypes.data, 0, d.data_ptr(), scene._stream()) == -1
    scene._upload_slots((1, None))
    assert L.zdr_render_aovs(scene._handle, C.byref(p), m.data_ptr(), dims.ctypes.data, 1, out.data_ptr(), scene._stream()) == -1
    assert L.zdr_render_aovs_backward(scene._handle, C.byref(p), out.data_ptr(), m.data_ptr(), dims.ctypes.data, 1, d.data_ptr(), scene._stream()) == -1
    with pytest.raises(N.ZdrError, match="material slot 1"):
        scene.render_aovs_forward(m, (W, W), spp, 0, slots=(1, None))
    # a struct of another size, and null buffers
    p.struct_size += 4
    assert L.zdr_render_aovs(scene._handle, C.byref(p), m.data_ptr(), dims.ctypes.data, 1, out.data_ptr(), scene._stream()) == -1
    p.struct_size -= 4
    assert L.zdr_render_aovs(scene._handle, C.byref(p), m.data_ptr(), dims.ctypes.data, 1, None, scene._stream()) == -1
    assert L.zdr_render_aovs_backward(scene._handle, C.byref(p), None, m.data_ptr(), dims.ctypes.data, 1, d.data_ptr(), scene._stream()) == -1
    assert float(d.abs().max()) == 0.0                                    # nothing of the refused calls ran
    scene.check()
