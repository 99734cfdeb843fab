"""-m gpu: the adjoint of the bounced light (zdr_scene_texel_bounce_backward, zdr_amd/csrc/zdr_bouncegrad.hip) against the float64 reference
of tests/texel_bounce_grad_ref.py run on the hits and decisions of the kernels' own dump, and the properties include/zdr.h states: the
targets are added into and what nothing reads keeps its bits, the rule is division free, the bake is linear where it says so (a
dot-product test), sample ranges add up, both accelerators agree, the workspace needs no initialisation, the high-level call hands every
material tensor and the emissions their gradient, the call can be captured without a call before, and wrong arguments raise.

Bars.  GR.MARGINS[case] is what float32 alone costs (the float32 reference with both summation orders, measured on the CPU); a gradient
must lie within max(4 x margin, 4 float32 ulps of the case's largest entry) of float64 — the kernel may differ from one float32 evaluation
by the order of its atomics.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import texel_bounce_cases as BC
import texel_bounce_grad_ref as GR
from texel_bounce_gpu import ACCELS, case_args, case_kw, case_scene, run_dump, run_forward
from zdr_amd import Scene
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

CASES = list(BC.CASES)
NAN_A, NAN_B = 0x7FC0BEEF, 0xFFC12345       # two quiet NaNs with a payload: bits that no addition leaves alone


def cot(name):
    return torch.from_numpy(GR.cotangent(name)).cuda()


def run_backward(name, accel, *, d_out=None, mats=None, d_materials=True, d_emission=True, workspace=None, scene=None, **kw):
    """(d_materials as a list of float32 arrays or None, d_emission array or None): the low-level call on zeroed (or the given) targets"""
    scene = case_scene(name, accel) if scene is None else scene
    pts, m = case_args(name, mats)
    dm = [torch.zeros_like(t) for t in m] if d_materials is True else d_materials
    de = torch.zeros(scene.inst_count, 3, device="cuda") if d_emission is True else d_emission
    scene.texel_bounce_backward(pts, cot(name) if d_out is None else d_out, m, d_materials=dm, d_emission=de, workspace=workspace, **case_kw(name, **kw))
    torch.cuda.synchronize()
    return (None if dm is None else [t.cpu().numpy() for t in dm]), (None if de is None else de.cpu().numpy())


_refs = {}


def dump_reference(name, accel):
    """the float64 gradient on the hits and decisions of the kernels' own dump, with the read masks of the float64 AND the float32 records
    (a lookup that float32 rounding moves into the neighbouring texel reads that texel too); computed once per (case, accelerator)"""
    if (name, accel) not in _refs:
        _, dump = run_dump(name, accel)
        grad = GR.texel_bounce_grad_ref(GR.case_records(name, dump), BC.materials(name), GR.cotangent(name))
        g32 = GR.texel_bounce_grad_ref(GR.case_records(name, dump, "float32"), BC.materials(name), GR.cotangent(name))
        grad["read"] = [a | b for a, b in zip(grad["read"], g32["read"])]
        _refs[(name, accel)] = grad
    return _refs[(name, accel)]


def worst(got, want):
    return max(float(np.abs(g.astype(np.float64) - w).max()) for g, w in zip(got, want))


def check(name, dm, de, ref, label, base_m=None, base_e=None):
    bm, be = GR.bars(name, ref)
    if dm is not None:
        want = ref["d_materials"] if base_m is None else [w + b for w, b in zip(ref["d_materials"], base_m)]
        em = max(float(np.abs(g[..., :3].astype(np.float64) - w[..., :3]).max()) for g, w in zip(dm, want))
        print(f"[texel bounce grad] {label}: d_materials off by at most {em:.3e} (bar {bm:.3e}, largest entry {GR.scales(ref)[0]:.3e})")
        assert all(np.isfinite(g[..., :3]).all() for g in dm)
        assert em <= bm
    if de is not None:
        want = ref["d_emission"] if base_e is None else ref["d_emission"] + base_e
        lights = GR.light_rows(name)
        ee = float(np.abs(de[lights].astype(np.float64) - want[lights]).max()) if lights else 0.0
        print(f"[texel bounce grad] {label}: d_emission off by at most {ee:.3e} (bar {be:.3e}, largest entry {GR.scales(ref)[1]:.3e})")
        assert ee <= be


# ------------------------------------------------------------------ 1. against the reference on the dump's own hits and decisions
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_float64_reference_on_the_dumps_own_walks(name, accel):
    ref = dump_reference(name, accel)
    dm, de = run_backward(name, accel)
    check(name, dm, de, ref, f"{name} {accel}")
    for j, g in enumerate(dm):
        assert np.abs(g[..., :3]).max() > 0, f"material {j} received nothing"
        assert (g[..., 3] == 0).all()
    assert np.isfinite(de).all()
    if name == "env_k2":
        assert (de == 0).all()                                        # no mesh light
    else:
        assert np.abs(de).max() > 0
    # each target alone is the same gradient
    only_m, none_e = run_backward(name, accel, d_emission=None)
    none_m, only_e = run_backward(name, accel, d_materials=None)
    assert none_e is None and none_m is None
    check(name, only_m, only_e, ref, f"{name} {accel}, each target alone")


# ------------------------------------------------------------------------------------------------ 2. added into
@pytest.mark.parametrize("accel", ACCELS)
def test_the_targets_are_added_into_and_what_nothing_reads_keeps_its_bits(accel):
    name = "multi_k3"
    ref = dump_reference(name, accel)
    scene = case_scene(name, accel)
    rng = np.random.default_rng(3)
    lights = GR.light_rows(name)
    base_m, pre_m = [], []
    for m, read in zip(BC.materials(name), ref["read"]):
        b = rng.uniform(-2.0, 2.0, m.shape).astype(np.float32)
        b.view(np.uint32)[~read, :3] = NAN_A
        b.view(np.uint32)[..., 3] = NAN_B
        assert (~read).any() or m.shape[0] * m.shape[1] < 64          # (the small material is read everywhere)
        base_m.append(b); pre_m.append(torch.from_numpy(b.copy()).cuda())
    base_e = rng.uniform(-2.0, 2.0, (scene.inst_count, 3)).astype(np.float32)
    dark = [i for i in range(scene.inst_count) if i not in lights]
    assert dark and lights
    base_e.view(np.uint32)[dark] = NAN_A
    dm, de = run_backward(name, accel, d_materials=pre_m, d_emission=torch.from_numpy(base_e.copy()).cuda())
    for g, b, read in zip(dm, base_m, ref["read"]):
        assert np.array_equal(g.view(np.uint32)[..., 3], b.view(np.uint32)[..., 3])          # the roughness channel: never touched
        assert np.array_equal(g.view(np.uint32)[~read], b.view(np.uint32)[~read])            # texels that no vertex reads
    assert np.array_equal(de.view(np.uint32)[dark], base_e.view(np.uint32)[dark])            # rows of models that are not lights
    got = [np.where(read[..., None], g, 0.0) for g, read in zip(dm, ref["read"])]
    base = [np.where(read[..., None], b.astype(np.float64), 0.0) for b, read in zip(base_m, ref["read"])]
    check(name, got, de, ref, f"{name} {accel} on prefilled targets", base_m=base, base_e=np.where(np.isnan(base_e), 0.0, base_e).astype(np.float64))


# ------------------------------------------------------------------------------------------- 3. division free
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["cbox_k3", "multi_k3"])
def test_an_all_zero_material_gets_the_one_bounce_gradient(name, accel):
    zero = tuple(np.zeros_like(m) for m in BC.materials(name))
    dm0, de0 = run_backward(name, accel, mats=zero)
    dm1, de1 = run_backward(name, accel, bounces=1)
    bm, _ = GR.bars(name, dump_reference(name, accel))
    off = worst([a[..., :3] for a in dm0], [b[..., :3].astype(np.float64) for b in dm1])
    top = max(float(np.abs(a).max()) for a in dm0)
    print(f"[texel bounce grad] {name} {accel}: zero materials, {BC.bounces(name)} bounces against one bounce: off by at most {off:.3e} (bar {bm:.3e}); largest entry {top:.3e}")
    assert top > 0 and all(np.isfinite(a).all() for a in dm0)
    assert off <= bm
    assert (de0 == 0).all() and np.abs(de1).max() > 0                 # every beta_k is 0


# ------------------------------------------------------------------------------------ 4. linearity: a dot-product test
@pytest.mark.parametrize("accel", ACCELS)
def test_the_one_bounce_bake_is_linear_a_dot_product_test(accel):
    name = "cbox_k1"
    ref = dump_reference(name, accel)
    bm, be = GR.bars(name, ref)
    g = GR.cotangent(name).astype(np.float64)[..., :3]
    g = np.where(np.isnan(g), 0.0, g)
    n_reached = int(BC.reached(name).sum())
    m0 = BC.materials(name)
    rng = np.random.default_rng(9)
    m1 = tuple(np.concatenate([rng.uniform(0.1, 0.95, m.shape[:2] + (3,)), m[..., 3:]], -1).astype(np.float32) for m in m0)
    f0, f1 = run_forward(name, accel).astype(np.float64)[..., :3], run_forward(name, accel, mats=m1).astype(np.float64)[..., :3]
    dm, de = run_backward(name, accel)
    dmat = [(b.astype(np.float64) - a)[..., :3] for a, b in zip(m0, m1)]
    lhs = float((g * (f1 - f0)).sum())
    rhs = float(sum((d[..., :3].astype(np.float64) * x).sum() for d, x in zip(dm, dmat)))
    # Bar.  Right side: every entry of d_materials lies within bm of the truth and multiplies |m1 - m0|.  Left side: a forward texel is
    # spp x K adds over spp, each within the estimator's bar BC.bar of float64 (tests/test_gpu_texel_bounce.py), times |d_out| <= 1, in
    # two bakes.  Both scaled by the number of terms.
    n_entries = sum(x.size for x in dmat)
    bar = n_entries * bm * max(float(np.abs(x).max()) for x in dmat) + 2 * 3 * n_reached * BC.bounces(name) * BC.bar(name)
    print(f"[texel bounce grad] {name} {accel}: materials, sum d_out (F(m1) - F(m0)) = {lhs:.9e}, sum d_m (m1 - m0) = {rhs:.9e}, differ by {abs(lhs - rhs):.3e} (bar {bar:.3e})")
    assert abs(lhs - rhs) <= bar
    em = np.asarray(BC.CASES[name][0]().inst_emission, np.float64).reshape(-1, 3)
    lights = GR.light_rows(name)
    lhs_e, rhs_e = float((g * f0).sum()), float((de[lights].astype(np.float64) * em[lights]).sum())
    bar_e = 3 * len(lights) * be * float(em[lights].max()) + 3 * n_reached * BC.bounces(name) * BC.bar(name)
    print(f"[texel bounce grad] {name} {accel}: emissions, sum d_out F(E) = {lhs_e:.9e}, sum d_E E = {rhs_e:.9e}, differ by {abs(lhs_e - rhs_e):.3e} (bar {bar_e:.3e})")
    assert abs(lhs_e - rhs_e) <= bar_e


# ------------------------------------------------------------------------------------------------------ 5. ranges
@pytest.mark.parametrize("accel", ACCELS)
def test_the_gradients_of_disjoint_sample_ranges_add_up_to_the_wholes(accel):
    name = "cbox_k3"
    bm, be = GR.bars(name, dump_reference(name, accel))
    wm, we = run_backward(name, accel)
    (am, ae), (bm_, be_) = run_backward(name, accel, samples=(0, 2)), run_backward(name, accel, samples=(2, 4))
    off_m = worst([a.astype(np.float64) + b for a, b in zip(am, bm_)], [w.astype(np.float64) for w in wm])
    off_e = float(np.abs(ae.astype(np.float64) + be_ - we).max())
    print(f"[texel bounce grad] {name} {accel}: [0, 2) + [2, 4) against [0, 4): d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
    assert off_m <= bm and off_e <= be
    assert max(float(np.abs(a).max()) for a in am) > 0 and max(float(np.abs(b).max()) for b in bm_) > 0


# ------------------------------------------------------------------------------------------- 6. both accelerators
def test_bvh_and_brute_force_agree():
    name = "multi_k3"
    bm, be = GR.bars(name, dump_reference(name, "brute"))
    (am, ae), (bm_, be_) = run_backward(name, "brute"), run_backward(name, "bvh")
    off_m, off_e = worst(am, [b.astype(np.float64) for b in bm_]), float(np.abs(ae.astype(np.float64) - be_).max())
    print(f"[texel bounce grad] {name}: brute force against BVH: d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
    assert off_m <= bm and off_e <= be


# ------------------------------------------------------------------------------ 7. the workspace needs no initialisation
@pytest.mark.parametrize("accel", ACCELS)
def test_two_runs_and_two_workspaces_agree(accel):
    name = "multi_k3"
    scene = case_scene(name, accel)
    bm, be = GR.bars(name, dump_reference(name, accel))
    dims = np.ascontiguousarray(np.array([m.shape[:2] for m in BC.materials(name)], np.int32))
    H, W = BC.CASES[name][2]
    need = int(N.lib().zdr_texel_bounce_backward_workspace_bytes(scene._handle, H, W, dims.ctypes.data, dims.shape[0]))
    assert need > 16 + 4 * H * W
    runs = [run_backward(name, accel, workspace=torch.full((need,), fill, dtype=torch.uint8, device="cuda")) for fill in (0x00, 0xA5)]
    off_m = worst(runs[0][0], [b.astype(np.float64) for b in runs[1][0]])
    off_e = float(np.abs(runs[0][1].astype(np.float64) - runs[1][1]).max())
    print(f"[texel bounce grad] {name} {accel}: workspace of zeros against one of 0xA5 ({need} bytes): d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
    assert off_m <= bm and off_e <= be
    check(name, runs[1][0], runs[1][1], dump_reference(name, accel), f"{name} {accel}, workspace of 0xA5")


# ------------------------------------------------------------------------------------------ 8. the high-level call
def test_texel_bounce_of_a_list_is_differentiable_in_every_material_and_the_emissions():
    name = "multi_k3"
    scene = case_scene(name, "bvh")
    old_slots, old_em = scene.material_slots, scene.emissions
    scene.material_slots = BC.MULTI_SLOTS
    kw = dict(spp=4, bounces=2, seed=BC.SEED)
    # the run-to-run noise of the atomics, relative to the largest entry: the case's own bar over its own largest entry (the same scene
    # and materials with more samples and one more bounce: more terms per target than here)
    sm, se = GR.scales(GR.reference_grad(name))
    rel_m, rel_e = GR.bars(name)[0] / sm, GR.bars(name)[1] / se
    try:
        _, plain = case_args(name)
        texels = scene.texel_aovs(plain, 1)
        # plain tensors: no autograd node, the bits of the low-level call
        tb = scene.texel_bounce(plain, index=1, **kw)
        low = scene.texel_bounce_forward(texels.data, plain, **kw)
        torch.cuda.synchronize()
        assert not tb.data.requires_grad and tb.data.grad_fn is None and torch.equal(tb.data, low)
        # the low-level gradient of sum(irradiance)
        d_out = torch.zeros(5, 7, 4, device="cuda"); d_out[..., :3] = 1.0
        want_m, want_e = [torch.zeros_like(t) for t in plain], torch.zeros(scene.inst_count, 3, device="cuda")
        scene.texel_bounce_backward(texels.data, d_out, plain, d_materials=want_m, d_emission=want_e, **kw)
        torch.cuda.synchronize()
        tol_m, tol_e = rel_m * max(float(t.abs().max()) for t in want_m), rel_e * float(want_e.abs().max())
        assert all(float(t.abs().max()) > 0 for t in want_m) and float(want_e.abs().max()) > 0
        # materials that require grad
        mats = [t.clone().requires_grad_(True) for t in plain]
        tb = scene.texel_bounce(mats, index=1, texels=texels, **kw)
        assert tb.data.requires_grad and torch.equal(tb.data.detach(), low)
        tb.irradiance.sum().backward()
        torch.cuda.synchronize()
        for t, w in zip(mats, want_m):
            off = float((t.grad - w).abs().max())
            print(f"[texel bounce grad] high-level call, material {tuple(t.shape)}: .grad against the low-level call: {off:.3e} (tolerance {tol_m:.3e})")
            assert t.grad.shape == t.shape and off <= tol_m and (t.grad[..., 3] == 0).all()
        # emissions=, and a later set_emission_values between forward and backward
        E = torch.from_numpy(np.asarray(BC.CASES[name][0]().inst_emission, np.float32).reshape(-1, 3)).cuda().requires_grad_(True)
        mats = [t.clone().requires_grad_(True) for t in plain]
        tb = scene.texel_bounce(mats, index=1, texels=texels, emissions=E, **kw)
        assert torch.equal(tb.data.detach(), low)
        scene.set_emission_values(3.0 * E.detach())
        tb.irradiance.sum().backward()
        torch.cuda.synchronize()
        off_e = float((E.grad - want_e).abs().max())
        off_m = max(float((t.grad - w).abs().max()) for t, w in zip(mats, want_m))
        print(f"[texel bounce grad] high-level call with emissions= and a later set_emission_values: E.grad {off_e:.3e} (tolerance {tol_e:.3e}), .grad {off_m:.3e} (tolerance {tol_m:.3e})")
        assert E.grad.shape == E.shape and off_e <= tol_e and off_m <= tol_m
        # emissions alone: plain materials, only E gets a gradient
        E2 = E.detach().clone().requires_grad_(True)
        scene.texel_bounce(plain, index=1, texels=texels, emissions=E2, **kw).irradiance.sum().backward()
        torch.cuda.synchronize()
        assert float((E2.grad - want_e).abs().max()) <= tol_e
    finally:
        scene.material_slots = old_slots
        scene.update_lights(old_em)
    scene.check()


# ------------------------------------------------------------------------------------------------------ 9. capture
@pytest.mark.parametrize("accel", ACCELS)
def test_the_adjoint_can_be_captured_without_a_call_before_and_replayed(accel):
    name = "multi_k3"
    ref = dump_reference(name, accel)
    bm, be = GR.bars(name, ref)
    scene = Scene(BC.CASES[name][0](), integrator="direct", accel=accel)     # a handle of its own: nothing was launched on it before
    scene.material_slots = BC.MULTI_SLOTS                           # (the slot table is the scene's state, set before the capture)
    pts, g = torch.from_numpy(BC.points(name)).cuda(), cot(name)
    mats = BC.materials(name)
    packed = torch.cat([torch.from_numpy(m).reshape(-1, 4) for m in mats]).cuda()
    dims = [m.shape[:2] for m in mats]
    d = np.ascontiguousarray(np.array(dims, np.int32))
    H, W = pts.shape[:2]
    dpacked, d_e = torch.zeros_like(packed), torch.zeros(scene.inst_count, 3, device="cuda")
    ws = torch.full((int(N.lib().zdr_texel_bounce_backward_workspace_bytes(scene._handle, H, W, d.ctypes.data, d.shape[0])),), 0xAB, dtype=torch.uint8, device="cuda")
    kw = dict(spp=BC.CASES[name][4], bounces=BC.bounces(name), seed=BC.SEED, dims=dims)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, one launch after the other: a single chain
        scene.texel_bounce_backward(pts, g, packed, d_materials=dpacked, d_emission=d_e, workspace=ws, **kw)
    eager_m, eager_e = torch.zeros_like(packed), torch.zeros_like(d_e)
    scene.texel_bounce_backward(pts, g, packed, d_materials=eager_m, d_emission=eager_e, **kw)
    torch.cuda.synchronize()

    def split(t):
        a, out, off = t.cpu().numpy(), [], 0
        for h, w in dims:
            out.append(a[off:off + h * w].reshape(h, w, 4)); off += h * w
        return out
    check(name, split(eager_m), eager_e.cpu().numpy(), ref, f"{name} {accel} eager, packed")
    for fill in (0x11, 0xFF):
        dpacked.zero_(); d_e.zero_(); ws.fill_(fill)                # whatever the workspace held: the call clears what it reads
        graph.replay()
        torch.cuda.synchronize()
        check(name, split(dpacked), d_e.cpu().numpy(), ref, f"{name} {accel} replay after {fill:#x}")
        off_m, off_e = float((dpacked - eager_m).abs().max()), float((d_e - eager_e).abs().max())
        print(f"[texel bounce grad] {name} {accel} replay after {fill:#x} against eager: d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
        assert off_m <= bm and off_e <= be
    del graph
    scene.check()


# --------------------------------------------------------------------------------------------- 10. argument checks
def test_bad_arguments_raise():
    name = "cbox_k1"
    scene = case_scene(name, "brute")
    pts, m = case_args(name)
    g = cot(name)
    dm, de = [torch.zeros_like(m[0])], torch.zeros(scene.inst_count, 3, device="cuda")
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            scene.texel_bounce_backward(pts, g, m, spp=4, bounces=bad, d_materials=dm)
    for samples in ((2, 2), (3, 1), (0, 5)):
        with pytest.raises(ValueError):
            scene.texel_bounce_backward(pts, g, m, spp=4, samples=samples, d_materials=dm)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts[..., :8].contiguous(), g, m, spp=4, d_materials=dm)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts.reshape(-1, 16), g, m, spp=4, d_materials=dm)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts, g, m, spp=4)                                       # both targets None
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts, g[:8].contiguous(), m, spp=4, d_materials=dm)      # a wrong d_out shape
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts, g[..., :3].contiguous(), m, spp=4, d_materials=dm)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts, g, m, spp=4, d_materials=[torch.zeros(8, 8, 4, device="cuda")])   # not shaped like the materials
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts, g, m, spp=4, d_materials=dm + dm)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward(pts, g, m, spp=4, d_emission=torch.zeros(scene.inst_count + 1, 3, device="cuda"))
    # the C interface: struct_size, both targets NULL, a misaligned target
    L = N.lib()
    dims = np.array([[16, 16]], np.int32)
    ws = torch.zeros(int(L.zdr_texel_bounce_backward_workspace_bytes(scene._handle, 16, 16, dims.ctypes.data, 1)), dtype=torch.uint8, device="cuda")
    p = N.TexelBounceParams()
    p.struct_size = C.sizeof(N.TexelBounceParams)
    p.tex_h, p.tex_w, p.spp, p.seed, p.sampler, p.sample_begin, p.sample_end, p.bounces = 16, 16, 4, 0, N.SAMPLERS["cmj"], 0, 4, 1
    args = lambda dmat, dem: (scene._handle, C.byref(p), pts.data_ptr(), g.data_ptr(), m[0].data_ptr(), dims.ctypes.data, 1, dmat, dem, ws.data_ptr(), None)
    assert L.zdr_scene_texel_bounce_backward(*args(None, None)) == -1                       # ZDR_E_INVALID
    assert L.zdr_scene_texel_bounce_backward(*args(dm[0].data_ptr() + 4, None)) == -1
    assert L.zdr_scene_texel_bounce_backward(*args(None, de.data_ptr() + 2)) == -1
    assert L.zdr_scene_texel_bounce_backward(*args(dm[0].data_ptr(), de.data_ptr())) == 0
    p.struct_size = 4
    assert L.zdr_scene_texel_bounce_backward(*args(dm[0].data_ptr(), de.data_ptr())) == -1
    assert L.zdr_texel_bounce_backward_workspace_bytes(scene._handle, 0, 16, dims.ctypes.data, 1) == 0
    torch.cuda.synchronize()
    scene.check()
