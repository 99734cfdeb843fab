"""-m gpu: the adjoint of the bounced light in the environment map (zdr_scene_texel_bounce_backward_env, zdr_amd/csrc/zdr_bounceenv.hip)
against the float64 reference of tests/texel_bounce_envgrad_ref.py run on the hits and decisions of the kernels' own dump, and the
properties include/zdr.h states: the wave-level merge is exercised and counted, the map is added into and what no sample reads keeps its
bits, sample ranges add up, the workspace needs no initialisation, both accelerators agree, the bake is linear in the map (a dot-product
test against the GPU forward), one bounce under unit albedos is the lighting adjoint at the first vertices, the high-level call hands
``envmap=`` its gradient in the caller's shape, the call can be captured without a call before, and wrong arguments raise.

Bars.  ER.MARGINS[case] is what float32 alone costs (the float32 reference with both summation orders, measured on the CPU); a gradient
must lie within max(4 x margin, 4 float32 ulps of the case's largest entry) of float64 — the kernel may differ from one float32 evaluation
by the order of its atomics.  Two GPU runs are compared within two bars.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import envmap_tables as ET
import texel_bounce_cases as BC
import texel_bounce_env_cases as EC
import texel_bounce_envgrad_ref as ER
import texel_bounce_grad_ref as GR
import texel_bounce_ref as BR
import texel_lighting_ref as LR
from zdr_amd import Scene
from zdr_amd import _native as N
from zdr_amd import envmap as E

pytestmark = pytest.mark.gpu

ACCELS = ["brute", "bvh"]
CASES = list(EC.CASES)
NAN_A, NAN_B = 0x7FC0BEEF, 0xFFC12345       # two quiet NaNs with a payload: bits that no addition leaves alone
_scenes, _dumps, _refs = {}, {}, {}


def make_scene(name, accel):
    c = EC.case(name)
    scene = Scene(c["make"](), integrator="direct", accel=accel)
    if c["sampler"]:
        scene.set_pmj02bn_tables(*EC.pmj_tables(name))
    tex, prob, alias, pdf, mw, mh = EC.env(name)                  # the tables the reference uses, as they are
    N.check(N.lib().zdr_scene_set_envmap(scene._handle, tex.ctypes.data, tex.shape[0], tex.shape[1], prob.ctypes.data, alias.ctypes.data, pdf.ctypes.data, mw, mh))
    scene.env_count = 1
    scene._envmap = (tex, prob, alias, pdf)
    assert scene.info()["accel"] == accel
    return scene


def case_scene(name, accel):
    c = EC.case(name)
    key = (c["make"], c["env"], accel, c["sampler"])
    if key not in _scenes:
        _scenes[key] = make_scene(name, accel)
    return _scenes[key]


def case_args(name, mats=None):
    return torch.from_numpy(EC.points(name)).cuda(), [torch.from_numpy(m).cuda() for m in (EC.materials(name) if mats is None else mats)]


def case_kw(name, **kw):
    c = EC.case(name)
    kw.setdefault("samples", c["samples"])
    kw.setdefault("bounces", c["K"])
    return dict(spp=c["spp"], seed=EC.SEED, sampler="pmj02bn" if c["sampler"] else None, slots=c["slots"], **kw)


def cot(name):
    return torch.from_numpy(ER.cotangent(name)).cuda()


def env_bytes(name, accel):
    h, w = EC.case(name)["hw"]
    return int(N.lib().zdr_texel_bounce_backward_env_workspace_bytes(h, w))


def run_backward(name, accel, *, d_out=None, d_env=None, workspace=None, scene=None, mats=None, **kw):
    """(d_env as a float32 array, the header's three words): the low-level call on a zeroed (or the given) target"""
    scene = case_scene(name, accel) if scene is None else scene
    pts, m = case_args(name, mats)
    if d_env is None:
        d_env = torch.zeros(tuple(scene._envmap[0].shape), device="cuda")
    if workspace is None:
        workspace = torch.full((env_bytes(name, accel),), 0x5A, dtype=torch.uint8, device="cuda")
    got = scene.texel_bounce_backward_env(pts, cot(name) if d_out is None else d_out, m, d_env=d_env, workspace=workspace, **case_kw(name, **kw))
    assert got is d_env
    torch.cuda.synchronize()
    header = workspace[:16].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return d_env.cpu().numpy(), [int(v) for v in header[:3]]


def run_dump(name, accel):
    """the dump of every sample of the case, in the order of the reference's rows, parsed; computed once per (case, accelerator)"""
    if (name, accel) not in _dumps:
        pts, m = case_args(name)
        q = EC.reference(name)["queries"]
        rows = case_scene(name, accel).texel_bounce_dump(pts, m, torch.from_numpy(np.ascontiguousarray(q)), **case_kw(name))
        torch.cuda.synchronize()
        _dumps[(name, accel)] = BR.parse_dump(rows.cpu().numpy(), EC.case(name)["K"])
    return _dumps[(name, accel)]


def dump_reference(name, accel):
    """the float64 gradient on the hits and decisions of the kernels' own dump, with the read mask of the float64 AND the float32 records
    (a footprint that float32 rounding moves into the neighbouring cell reads that cell too), the records themselves, and the header the
    kernel must report for a list in row-major order; computed once per (case, accelerator)"""
    if (name, accel) not in _refs:
        dump = run_dump(name, accel)
        rec = ER.case_records(name, dump)
        grad = ER.texel_bounce_envgrad_ref(rec, EC.materials(name), ER.cotangent(name))
        g32 = ER.texel_bounce_envgrad_ref(ER.case_records(name, dump, "float32"), EC.materials(name), ER.cotangent(name))
        grad["read"] = grad["read"] | g32["read"]
        grad["rec"] = rec
        _refs[(name, accel)] = grad
    return _refs[(name, accel)]


def off_by(got, want):
    return float(np.abs(got[..., :3].astype(np.float64) - want[..., :3]).max())


def check(name, got, ref, label, base=None):
    bar = ER.bar(name, ref)
    want = ref["d_env"] if base is None else ref["d_env"] + base
    e = off_by(got, want)
    print(f"[texel bounce envgrad] {label}: d_env off by at most {e:.3e} (bar {bar:.3e}, {e / bar:.3f} of it; largest entry {ER.scale(ref):.3e})")
    assert np.isfinite(got[..., :3]).all()
    assert e <= bar


# ------------------------------------------------------------------ 1. against the reference on the dump's own hits and decisions
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_float64_reference_on_the_dumps_own_walks(name, accel):
    ref = dump_reference(name, accel)
    got, header = run_backward(name, accel)
    check(name, got, ref, f"{name} {accel}")
    assert np.abs(got[..., :3]).max() > 0
    assert (got[..., 3] == 0).all() and (got[~ref["read"]] == 0).all()
    # the header: shaded texels, accepted environment samples (the reference's count on the dump's walks), groups that went to memory
    print(f"[texel bounce envgrad] {name} {accel}: header {header}; the reference counts {ref['n_samples']} accepted environment samples")
    assert header[0] == len(ref["rec"]["ys"])
    assert header[1] == ref["n_samples"]
    assert 0 < header[2] <= header[1]


# ------------------------------------------------------------------------------------------------ 2. the merge
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["env_wave", "env_wave_ragged", "env_sky"])
def test_the_merge_is_exercised_and_counted(name, accel):
    ref = dump_reference(name, accel)
    _, header = run_backward(name, accel)
    # 25 texels: one wave compacts them, the list is row-major and the waves of the shading kernel are the reference's
    groups = ER.wave_groups(ref["rec"], name)
    want = ER.expected_groups(ref["rec"], name)
    merged_only = sum(min(g[1], EC.MERGE_ROUNDS) for g in groups)
    print(f"[texel bounce envgrad] {name} {accel}: {header[1]} accepted environment samples in {header[2]} groups (the reference: {want}; "
          f"{merged_only} of them merged cells, {want - merged_only} leftover lanes)")
    assert header[2] == want
    if name == "env_sky":
        assert want > merged_only                                     # lanes left over after the rounds went to memory themselves
    else:
        assert header[2] < header[1]                                  # lanes that share a cell were summed on chip


# ------------------------------------------------------------------------------------------------ 3. added into
@pytest.mark.parametrize("accel", ACCELS)
def test_the_map_is_added_into_and_what_no_sample_reads_keeps_its_bits(accel):
    name = "env_k2"
    ref = dump_reference(name, accel)
    read = ref["read"]
    rng = np.random.default_rng(3)
    S = ER.scale(ref)
    base = (S * rng.uniform(-1.0, 1.0, read.shape + (4,))).astype(np.float32)      # of the gradient's own size: see the bar below
    base.view(np.uint32)[~read, :3] = NAN_A
    base.view(np.uint32)[..., 3] = NAN_B
    assert (~read).any() and read.any()
    got, _ = run_backward(name, accel, d_env=torch.from_numpy(base.copy()).cuda())
    assert np.array_equal(got.view(np.uint32)[..., 3], base.view(np.uint32)[..., 3])          # alpha: never touched
    assert np.array_equal(got.view(np.uint32)[~read], base.view(np.uint32)[~read])            # texels that no footprint touches
    # Bar.  The case's bar covers sums that start at 0.  Here every add lands on a partial sum of magnitude <= |prefill| + |entry| <= 2 S
    # and rounds it by at most half an ulp, 2^-24 x 2 S; an entry receives at most as many adds as it has terms.
    want = np.where(read[..., None], base.astype(np.float64), 0.0) * np.array([1.0, 1.0, 1.0, 0.0]) + ref["d_env"]
    bar = ER.bar(name, ref) + int(ref["count"].max()) * ER.EPS32 * 2.0 * S
    e = off_by(np.where(read[..., None], got, 0.0), want)
    print(f"[texel bounce envgrad] {name} {accel} on a prefilled map: d_env off by at most {e:.3e} (bar {bar:.3e}: the case's {ER.bar(name, ref):.3e} and "
          f"{int(ref['count'].max())} adds onto sums of at most {2 * S:.3e})")
    assert e <= bar
    # the cotangent of `surface` and of the texels that are not shaded is never read: NaNs there (ER.cotangent) against zeros
    g = ER.cotangent(name)
    assert np.isnan(g[..., 3]).all() and np.isnan(g[~EC.reached(name)]).all() and (~EC.reached(name)).any()
    nan_run, _ = run_backward(name, accel)
    zero_run, _ = run_backward(name, accel, d_out=torch.from_numpy(np.nan_to_num(g, nan=0.0)).cuda())
    e = off_by(nan_run, zero_run.astype(np.float64))
    print(f"[texel bounce envgrad] {name} {accel}: NaN cotangents where nothing is read against zeros there: {e:.3e} (two bars {2 * ER.bar(name, ref):.3e})")
    assert np.isfinite(nan_run).all() and e <= 2 * ER.bar(name, ref)


# ------------------------------------------------------------------------------------------------------ 4. ranges
@pytest.mark.parametrize("accel", ACCELS)
def test_the_gradients_of_disjoint_sample_ranges_add_up_to_the_wholes(accel):
    name = "env_k2"
    bar = ER.bar(name, dump_reference(name, accel))
    whole, hw = run_backward(name, accel)
    (a, ha), (b, hb) = run_backward(name, accel, samples=(0, 2)), run_backward(name, accel, samples=(2, 4))
    e = off_by(a.astype(np.float64) + b, whole.astype(np.float64))
    print(f"[texel bounce envgrad] {name} {accel}: [0, 2) + [2, 4) against [0, 4): {e:.3e} (two bars {2 * bar:.3e}); samples {ha[1]} + {hb[1]} = {hw[1]}")
    assert e <= 2 * bar and ha[1] + hb[1] == hw[1]
    assert np.abs(a).max() > 0 and np.abs(b).max() > 0


# ------------------------------------------------------------------------------ 5. the workspace needs no initialisation
@pytest.mark.parametrize("accel", ACCELS)
def test_two_workspaces_agree(accel):
    name = "env_k3"
    ref = dump_reference(name, accel)
    need = env_bytes(name, accel)
    assert need == 16 + 4 * 144
    runs = [run_backward(name, accel, workspace=torch.full((need,), fill, dtype=torch.uint8, device="cuda")) for fill in (0x00, 0xA5)]
    e = off_by(runs[0][0], runs[1][0].astype(np.float64))
    print(f"[texel bounce envgrad] {name} {accel}: workspace of zeros against one of 0xA5 ({need} bytes): {e:.3e} (two bars {2 * ER.bar(name, ref):.3e})")
    assert e <= 2 * ER.bar(name, ref) and runs[0][1] [:2] == runs[1][1][:2]
    check(name, runs[1][0], ref, f"{name} {accel}, workspace of 0xA5")


# ------------------------------------------------------------------------------------------- 6. both accelerators
def test_bvh_and_brute_force_agree():
    name = "env_k2"
    bar = ER.bar(name, dump_reference(name, "brute"))
    (a, ha), (b, hb) = run_backward(name, "brute"), run_backward(name, "bvh")
    e = off_by(a, b.astype(np.float64))
    print(f"[texel bounce envgrad] {name}: brute force against BVH: {e:.3e} (two bars {2 * bar:.3e}); accepted environment samples {ha[1]} and {hb[1]}")
    assert e <= 2 * bar


# ------------------------------------------------------------------------------------ 7. linearity: a dot-product test
def dot_product_against_the_gpu_forward(name, accel):
    """<d_out, F(env + d) - F(env)> of two GPU bakes against <d_env, d> of the adjoint, for a case that tests/texel_bounce_cases.py shares"""
    scene = case_scene(name, accel)
    ref = dump_reference(name, accel)
    bar_g = ER.bar(name, ref)
    g = np.nan_to_num(ER.cotangent(name).astype(np.float64)[..., :3], nan=0.0)
    n_reached = int(EC.reached(name).sum())
    env0 = EC.env(name)[0]
    delta = np.zeros_like(env0)
    delta[..., :3] = np.random.default_rng(9).uniform(0.0, 1.0, env0.shape[:2] + (3,)).astype(np.float32)    # >= 0: no accepted sample turns dark
    pts, m = case_args(name)
    try:
        f0 = scene.texel_bounce_forward(pts, m, **case_kw(name)).cpu().numpy().astype(np.float64)[..., :3]
        scene.set_envmap_texture(torch.from_numpy(env0 + delta).cuda())            # the tables stay the scene's
        f1 = scene.texel_bounce_forward(pts, m, **case_kw(name)).cpu().numpy().astype(np.float64)[..., :3]
    finally:
        scene.set_envmap_texture(torch.from_numpy(env0).cuda())
        torch.cuda.synchronize()
    d_env, _ = run_backward(name, accel)
    lhs = float((g * (f1 - f0)).sum())
    rhs = float((d_env[..., :3].astype(np.float64) * delta[..., :3]).sum())
    # Bar, formed as tests/test_gpu_texel_bounce_grad.py forms its own.  Right side: every entry of d_env that a footprint touches lies
    # within bar_g of the truth and multiplies |delta| <= 1.  Left side: a forward texel is spp x K adds over spp, each within the
    # estimator's bar BC.bar of float64 (tests/test_gpu_texel_bounce.py), times |d_out| <= 1, in two bakes.
    n_entries = 3 * int(ref["read"].sum())
    bar = n_entries * bar_g * float(delta.max()) + 2 * 3 * n_reached * EC.case(name)["K"] * BC.bar(name)
    print(f"[texel bounce envgrad] {name} {accel}: sum d_out (F(env + d) - F(env)) = {lhs:.9e}, sum d_env d = {rhs:.9e}, differ by {abs(lhs - rhs):.3e} (bar {bar:.3e})")
    assert abs(rhs) > 0 and abs(lhs) > 0
    assert abs(lhs - rhs) <= bar


@pytest.mark.parametrize("accel", ACCELS)
def test_the_bake_is_linear_in_the_map_a_dot_product_test_against_the_gpu_forward(accel):
    dot_product_against_the_gpu_forward("env_k2", accel)


# ------------------------------------------------------- 8. one bounce under unit albedos is the lighting adjoint at the first vertices
@pytest.mark.parametrize("accel", ACCELS)
def test_one_bounce_under_unit_albedos_is_the_lighting_adjoint_at_the_first_vertices(accel):
    """Vertex 1 of a walk draws u_pick, u_prim, u_pt right after u_ao: floats 2..5 of the baker's sampler state for (x, y, s), the very
    draws of texel_lighting's sample s of texel (x, y) (asserted below on the references' dumps).  So with one bounce and albedo 1,
    d_env is the d_env of texel_lighting_backward run sample by sample on buffers that hold, per texel, the hit point and the shading
    normal of that sample's first vertex."""
    name = "env_k2"
    c = EC.case(name)
    scene = case_scene(name, accel)
    ref = dump_reference(name, accel)
    rec = ref["rec"]
    ys, xs, spp = rec["ys"], rec["xs"], c["spp"]
    ub = BR.draws(LR.SAMPLER_KINDS["cmj"], xs, ys, EC.SEED, spp, np.arange(spp), 1)
    ul = LR.draws(LR.SAMPLER_KINDS["cmj"], xs, ys, EC.SEED, spp, np.arange(spp))
    assert np.array_equal(ub[..., :6].view(np.uint32), ul[..., :6].view(np.uint32))              # the draws line up
    ones = tuple(np.concatenate([np.ones(m.shape[:2] + (3,), np.float32), m[..., 3:]], -1) for m in EC.materials(name))
    got, header = run_backward(name, accel, mats=ones, bounces=1)
    dump = run_dump(name, accel)
    geo = BR.Geometry(c["make"](), np.float64)
    sh = rec["shaded"][:, 0].reshape(len(ys), spp)
    inst, prim = dump["inst"][:, 0].reshape(len(ys), spp), dump["prim"][:, 0].reshape(len(ys), spp)
    uv = dump["uv"][:, 0].reshape(len(ys), spp, 2)
    want = torch.zeros(tuple(scene._envmap[0].shape), device="cuda")
    H, W = c["hw"]
    for s in range(spp):
        sel = np.nonzero(sh[:, s])[0]
        p, _, ns, _ = geo.interact(inst[sel, s], prim[sel, s], uv[sel, s, 0].astype(np.float32), uv[sel, s, 1].astype(np.float32))
        buf = np.zeros((H, W, 16), np.float32)
        buf[ys[sel], xs[sel], 4:7] = ns; buf[ys[sel], xs[sel], 8:11] = p; buf[ys[sel], xs[sel], 12] = 1.0
        scene.texel_lighting_backward(torch.from_numpy(buf).cuda(), cot(name), spp=spp, seed=EC.SEED, samples=(s, s + 1), d_env=want)
    torch.cuda.synchronize()
    bar = ER.bar(name, ref)
    e = off_by(got, want.cpu().numpy().astype(np.float64))
    print(f"[texel bounce envgrad] {name} {accel}: one bounce, unit albedos against texel_lighting_backward at the first vertices: {e:.3e} "
          f"(two bars {2 * bar:.3e}); {header[1]} accepted environment samples, largest entry {float(np.abs(got).max()):.3e}")
    assert header[1] == int(ER.accepted_env(rec)[:, 0].sum()) and np.abs(got).max() > 0
    assert e <= 2 * bar


# ------------------------------------------------------------------------------------------ 9. the high-level call
def test_texel_bounce_with_envmap_is_differentiable_in_the_map_in_the_callers_shape():
    name = "env_lit_k2"
    c = EC.case(name)
    scene = make_scene(name, "bvh")                                   # a handle of its own: the call replaces its map and its emissions
    scene.material_slots = c["slots"]
    kw = dict(spp=c["spp"], bounces=2, seed=EC.SEED)
    rel = ER.bar(name) / ER.scale(ER.reference_grad(name))            # the run-to-run noise of the atomics relative to the largest entry
    sm, se = GR.scales(GR.reference_grad(name))
    rel_m, rel_e = GR.bars(name)[0] / sm, GR.bars(name)[1] / se
    img = ET.make_map("sun_sky", (16, 32))                            # the (H, 2H, 3) image behind LC.sun_env
    _, plain = case_args(name)
    texels = scene.texel_aovs(plain, 0)
    E0 = torch.from_numpy(np.asarray(c["make"]().inst_emission, np.float32).reshape(-1, 3)).cuda()
    low = scene.texel_bounce_forward(texels.data, plain, **kw)
    d_out = torch.zeros(tuple(low.shape), device="cuda"); d_out[..., :3] = 1.0
    want_env = scene.texel_bounce_backward_env(texels.data, d_out, plain, d_env=torch.zeros(tuple(scene._envmap[0].shape), device="cuda"), **kw)
    want_m, want_e = [torch.zeros_like(t) for t in plain], torch.zeros(scene.inst_count, 3, device="cuda")
    scene.texel_bounce_backward(texels.data, d_out, plain, d_materials=want_m, d_emission=want_e, **kw)
    sky_ref = torch.from_numpy(img).cuda().requires_grad_(True)       # the low-level gradient through the preparation, in the caller's shape
    E.prepare_tensor(sky_ref).backward(want_env)
    torch.cuda.synchronize()
    assert float(want_env.abs().max()) > 0 and float(want_e.abs().max()) > 0
    tol = rel * float(want_env.abs().max()) * 2                       # the preparation sums two prepared rows into one of the caller's
    tol_m, tol_e = rel_m * max(float(t.abs().max()) for t in want_m), rel_e * float(want_e.abs().max())
    # without envmap=: no new autograd node, the bits of the low-level call
    tb = scene.texel_bounce(plain, index=0, texels=texels, **kw)
    assert tb.data.grad_fn is None and torch.equal(tb.data, low)
    # envmap= alone
    sky = torch.from_numpy(img).cuda().requires_grad_(True)
    tb = scene.texel_bounce(plain, index=0, texels=texels, envmap=sky, **kw)
    assert tb.data.requires_grad and torch.equal(tb.data.detach(), low)
    tb.irradiance.sum().backward()
    torch.cuda.synchronize()
    e = float((sky.grad - sky_ref.grad).abs().max())
    print(f"[texel bounce envgrad] high-level call, envmap= {tuple(sky.shape)}: .grad against the low-level call: {e:.3e} (tolerance {tol:.3e})")
    assert sky.grad.shape == sky.shape == (16, 32, 3) and e <= tol
    # materials, emissions and the map in one call; the scene's map and emissions change between forward and backward
    mats = [t.clone().requires_grad_(True) for t in plain]
    Eg = E0.clone().requires_grad_(True)
    sky2 = torch.from_numpy(img).cuda().requires_grad_(True)
    tb = scene.texel_bounce(mats, index=0, texels=texels, emissions=Eg, envmap=sky2, **kw)
    assert torch.equal(tb.data.detach(), low)
    scene.set_envmap_texture(3.0 * torch.from_numpy(EC.env(name)[0]).cuda())
    scene.set_emission_values(2.0 * E0)
    tb.irradiance.sum().backward()
    torch.cuda.synchronize()
    e = float((sky2.grad - sky_ref.grad).abs().max())
    e_m = max(float((t.grad - w).abs().max()) for t, w in zip(mats, want_m))
    e_e = float((Eg.grad - want_e).abs().max())
    print(f"[texel bounce envgrad] high-level call with materials, emissions= and envmap=, the scene changed before the backward: sky.grad {e:.3e} "
          f"(tolerance {tol:.3e}), .grad {e_m:.3e} (tolerance {tol_m:.3e}), E.grad {e_e:.3e} (tolerance {tol_e:.3e})")
    assert e <= tol and e_m <= tol_m and e_e <= tol_e
    # the call without envmap= gives the same material and emission gradients
    mats3 = [t.clone().requires_grad_(True) for t in plain]
    E3 = E0.clone().requires_grad_(True)
    scene.texel_bounce(mats3, index=0, texels=texels, emissions=E3, **kw).irradiance.sum().backward()
    torch.cuda.synchronize()
    assert max(float((a.grad - b.grad).abs().max()) for a, b in zip(mats, mats3)) <= tol_m and float((Eg.grad - E3.grad).abs().max()) <= tol_e
    # a scene without a map raises as texel_lighting does
    bare = Scene(c["make"](), integrator="direct")
    bare.material_slots = c["slots"]
    with pytest.raises(ValueError):
        bare.texel_bounce(plain, index=0, envmap=sky.detach(), **kw)
    with pytest.raises(ValueError):
        scene.texel_bounce(plain, index=0, texels=texels, envmap=sky.detach()[:8], **kw)      # not the map's size
    scene.check()


# ------------------------------------------------------------------------------------------------------ 10. capture
@pytest.mark.parametrize("accel", ACCELS)
def test_the_adjoint_can_be_captured_without_a_call_before_and_replayed_twice(accel):
    name = "env_k2"
    ref = dump_reference(name, accel)
    bar = ER.bar(name, ref)
    scene = make_scene(name, accel)                                   # a handle of its own: nothing was launched on it before
    scene.material_slots = EC.case(name)["slots"]                     # (the slot table is the scene's state, set before the capture)
    pts, g = torch.from_numpy(EC.points(name)).cuda(), cot(name)
    mats = EC.materials(name)
    packed = torch.cat([torch.from_numpy(m).reshape(-1, 4) for m in mats]).cuda()
    dims = [m.shape[:2] for m in mats]
    base = (ER.scale(ref) * np.random.default_rng(5).uniform(-1.0, 1.0, tuple(scene._envmap[0].shape))).astype(np.float32)   # of the gradient's own size
    d_env = torch.from_numpy(base.copy()).cuda()
    ws = torch.full((env_bytes(name, accel),), 0xAB, dtype=torch.uint8, device="cuda")
    kw = dict(spp=EC.case(name)["spp"], bounces=EC.case(name)["K"], seed=EC.SEED, dims=dims)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, one launch after the other: a single chain
        scene.texel_bounce_backward_env(pts, g, packed, d_env=d_env, workspace=ws, **kw)
    d_env.copy_(torch.from_numpy(base))                             # (the capture itself adds nothing, but the test does not rely on it)
    graph.replay()
    ws.fill_(0xFF)                                                  # whatever the workspace holds: the call clears what it reads
    graph.replay()
    torch.cuda.synchronize()
    got = d_env.cpu().numpy().astype(np.float64)
    want = base.astype(np.float64) + 2.0 * ref["d_env"]
    e = float(np.abs(got[..., :3] - want[..., :3]).max())
    print(f"[texel bounce envgrad] {name} {accel}: two replays onto a prefilled map against prefill + 2 x the reference: {e:.3e} (two bars {2 * bar:.3e})")
    assert e <= 2 * bar
    assert np.array_equal(d_env.cpu().numpy()[..., 3], base[..., 3])
    del graph
    scene.check()


# --------------------------------------------------------------------------------------------- 11. argument checks
def test_bad_arguments_raise():
    name = "env_k2"
    scene = case_scene(name, "brute")
    pts, m = case_args(name)
    g = cot(name)
    shape = tuple(scene._envmap[0].shape)
    d_env = torch.zeros(shape, device="cuda")
    kw = dict(spp=4, slots=EC.case(name)["slots"])
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            scene.texel_bounce_backward_env(pts, g, m, bounces=bad, d_env=d_env, **kw)
    for samples in ((2, 2), (3, 1), (0, 5)):
        with pytest.raises(ValueError):
            scene.texel_bounce_backward_env(pts, g, m, samples=samples, d_env=d_env, **kw)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward_env(pts, g[:8].contiguous(), m, d_env=d_env, **kw)                        # a wrong d_out shape
    with pytest.raises(ValueError):
        scene.texel_bounce_backward_env(pts, g, m, d_env=None, **kw)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward_env(pts, g, m, d_env=torch.zeros(shape[0], shape[1], 3, device="cuda"), **kw)   # a wrong shape
    with pytest.raises(ValueError):
        scene.texel_bounce_backward_env(pts, g, m, d_env=torch.zeros(shape[0] // 2, shape[1], 4, device="cuda"), **kw)
    with pytest.raises(ValueError):
        scene.texel_bounce_backward_env(pts, g, m, d_env=torch.zeros(shape), **kw)                            # on the host
    with pytest.raises(ValueError):
        scene.texel_bounce_backward_env(pts, g, m, d_env=torch.zeros(shape, device="cuda", dtype=torch.float64), **kw)
    with pytest.raises(TypeError):
        scene.texel_bounce_backward_env(pts, g, m, **kw)                                                      # d_env is required
    bare = Scene(EC.case(name)["make"](), integrator="direct", accel="brute")
    with pytest.raises(ValueError):
        bare.texel_bounce_backward_env(pts, g, m, d_env=d_env, **kw)                                          # no map
    # the C interface
    L = N.lib()
    dims = np.ascontiguousarray(np.array([t.shape[:2] for t in m], np.int32))
    packed = torch.cat([t.reshape(-1, 4) for t in m])
    H, W = EC.case(name)["hw"]
    ws = torch.zeros(int(L.zdr_texel_bounce_backward_env_workspace_bytes(H, W)) + 64, dtype=torch.uint8, device="cuda")
    p = N.TexelBounceParams()
    p.struct_size = C.sizeof(N.TexelBounceParams)
    p.tex_h, p.tex_w, p.spp, p.seed, p.sampler, p.sample_begin, p.sample_end, p.bounces = H, W, 4, 0, N.SAMPLERS["cmj"], 0, 4, 2
    scene.material_slots = EC.case(name)["slots"]
    args = lambda handle, de, w=None: (handle, C.byref(p), pts.data_ptr(), g.data_ptr(), packed.data_ptr(), dims.ctypes.data, dims.shape[0], de,
                                       ws.data_ptr() if w is None else w, None)
    INVALID = -1                                                      # ZDR_E_INVALID
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, None)) == INVALID
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, d_env.data_ptr() + 4)) == INVALID
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, ws.data_ptr())) == INVALID             # d_env overlaps the workspace
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, pts.data_ptr())) == INVALID            # d_env overlaps an input
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, d_env.data_ptr(), g.data_ptr())) == INVALID   # the workspace overlaps an input
    bare.material_slots = EC.case(name)["slots"]
    assert L.zdr_scene_texel_bounce_backward_env(*args(bare._handle, d_env.data_ptr())) == INVALID
    assert b"d_env given, but the scene has no environment map" in L.zdr_last_error()
    p.bounces = 9
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, d_env.data_ptr())) == INVALID
    p.bounces = 2
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, d_env.data_ptr())) == 0
    p.struct_size = 4
    assert L.zdr_scene_texel_bounce_backward_env(*args(scene._handle, d_env.data_ptr())) == INVALID
    assert L.zdr_texel_bounce_backward_env_workspace_bytes(0, 16) == 0
    torch.cuda.synchronize()
    scene.check()
