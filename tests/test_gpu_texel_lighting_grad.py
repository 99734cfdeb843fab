"""-m gpu: the adjoint of the texture-space lighting (Scene.texel_lighting_backward, Scene.texel_lighting(emissions=, envmap=);
include/zdr.h, zdr_scene_texel_lighting_backward) against the float64 reference of tests/texel_lighting_grad_ref.py on the cases of
tests/texel_lighting_grad_cases.py, for both accelerators, and the properties the header states: Euler's identity on the kernels' own
outputs, add-into, sample ranges add up, cotangents that are never read, the autograd route, and the argument checks.

The kernels get the case's float32 sample points and cotangent, the floats the reference was given.  An entry fails when it is off the
float64 reference by more than its bar, max(4 x the float32 reference's own error, 16 x 2^-24 x the sum of |terms| of that entry); no
entry may fail.  The sums use float atomics, so nothing is compared bit for bit.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import texel_lighting_grad_cases as GC
from zdr_amd import Scene, TexelAovs
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -3            # ZDR_E_* of include/zdr.h
EPS32 = 2.0 ** -24

_scenes = {}


def set_case_envmap(scene, env):
    """the tables the reference uses, as they are (add_envmap would build them again)"""
    tex, prob, alias, pdf, mw, mh = env()
    N.check(N.lib().zdr_scene_set_envmap(scene._handle, tex.ctypes.data, tex.shape[0], tex.shape[1], prob.ctypes.data, alias.ctypes.data, pdf.ctypes.data, mw, mh))
    scene.env_count = 1
    scene._envmap = (tex, prob, alias, pdf)


def new_scene(name, accel):
    make, env = GC.case(name)[0], GC.case(name)[4]
    scene = Scene(make(), integrator="direct", accel=accel)
    if name in GC.SAMPLERS:
        scene.set_pmj02bn_tables(*GC.pmj_tables(name))
    if env:
        set_case_envmap(scene, env)
    assert scene.info()["accel"] == accel
    return scene


def case_scene(name, accel):
    key = (GC.case(name)[0], GC.case(name)[4], accel, GC.SAMPLERS.get(name))
    if key not in _scenes:
        _scenes[key] = new_scene(name, accel)
    return _scenes[key]


def case_kw(name, **kw):
    kw.setdefault("samples", GC.RANGES.get(name))
    return dict(spp=GC.case(name)[3], seed=GC.SEED, sampler="pmj02bn" if name in GC.SAMPLERS else None, **kw)


def zeros(name, scene, target):
    return torch.zeros(scene.inst_count, 3, device="cuda") if target == "emission" else torch.zeros(tuple(scene._envmap[0].shape), device="cuda")


def run_case(name, accel, which, d_out=None, fill=None, **kw):
    """the low-level call into fresh targets (zeros, or ``fill``: a dict of prefilled tensors) -> {target: numpy}"""
    scene = case_scene(name, accel)
    tg = {t: (zeros(name, scene, t) if fill is None else fill[t].clone()) for t in which}
    g = torch.from_numpy(GC.cotangent(name)).cuda() if d_out is None else d_out
    scene.texel_lighting_backward(torch.from_numpy(GC.points(name)).cuda(), g, d_emission=tg.get("emission"), d_env=tg.get("env"), **case_kw(name, **kw))
    torch.cuda.synchronize()
    return {t: v.cpu().numpy() for t, v in tg.items()}


def check_parity(name, got, ref, tag):
    for target, g in got.items():
        fail = GC.failing(name, target, g, ref)
        want, a = GC.entries(ref, target)
        err = np.abs((g if target == "emission" else g[..., :3]).astype(np.float64) - want)
        bar = GC.bar(name, target, ref)
        print(f"[texel lighting grad parity] {tag} {target}: entries {want.size}, non-zero {int((want != 0).sum())}, failing {int(fail.sum())}; kernel vs float64 largest "
              f"{err.max():.3e} ({(err / np.maximum(bar, 1e-300)).max():.3f} of its bar); float32 reference {GC.MARGINS[name][target]:.3e}; "
              f"largest |entry| {np.abs(want).max():.4e}, largest sum |terms| {a.max():.4e}")
        assert not fail.any(), (tag, target, int(fail.sum()))
        if target == "env":
            assert (g[..., 3] == 0).all()
        else:
            assert (g[[i for i in range(g.shape[0]) if i not in GC.lights(name)]] == 0).all()


def modes(name):
    t = GC.targets(name)
    return [(x,) for x in t] + ([t] if len(t) == 2 else [])


# ------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("accel", ["brute", "bvh"])
@pytest.mark.parametrize("name", list(GC.CASES))
def test_parity_with_the_float64_reference_each_target_alone_and_both_in_one_call(name, accel):
    for which in modes(name):
        check_parity(name, run_case(name, accel, which), GC.reference(name), f"{name} {accel} {'+'.join(which)}")
    case_scene(name, accel).check()


# --------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("name", ["multi_24_spp9", "chandelier_24", "env_panel_8x8", "env_panel_lit_16"])
def test_eulers_identity_on_the_kernels_own_outputs(name):
    """F is homogeneous of degree 1 in (emissions, map) together: <d_out, F> = <d_emission, e> + <d_env, env.rgb>.  Each side is a sum of
    the same products d_out x inv_spp x w x (emission or map texel), rounded differently; 16 ulps of the sums of their absolute values."""
    scene = case_scene(name, "bvh")
    pts, g = torch.from_numpy(GC.points(name)).cuda(), GC.cotangent(name).astype(np.float64)
    kw = case_kw(name)
    F = scene.texel_lighting_forward(pts, spp=kw["spp"], seed=kw["seed"], samples=kw["samples"], sampler=kw["sampler"]).cpu().numpy().astype(np.float64)[..., :3]
    got = run_case(name, "bvh", GC.targets(name))
    lhs, total = float((g[..., :3] * F).sum()), float(np.abs(g[..., :3] * F).sum())
    rhs = 0.0
    if "emission" in got:
        e = GC.CASES[name][0]().inst_emission.astype(np.float64)
        rhs += float((got["emission"] * e).sum()); total += float(np.abs(got["emission"] * e).sum())
    if "env" in got:
        tex = GC.CASES[name][4]()[0].astype(np.float64)[..., :3]
        rhs += float((got["env"][..., :3] * tex).sum()); total += float(np.abs(got["env"][..., :3] * tex).sum())
    print(f"[texel lighting grad euler] {name}: <d_out, F> {lhs:.9e}  <d_emission, e> + <d_env, env> {rhs:.9e}  difference {abs(lhs - rhs):.3e} "
          f"= {abs(lhs - rhs) / (EPS32 * total):.2f} ulps of the absolute sums {total:.4e}")
    assert total > 0 and abs(lhs - rhs) <= 16 * EPS32 * total


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_the_targets_are_added_into_and_what_no_sample_touches_keeps_its_bits(accel):
    name = "env_panel_lit_16"
    scene, ref = case_scene(name, accel), GC.reference(name)
    rng = np.random.default_rng(3)
    fill = {"emission": torch.from_numpy(rng.standard_normal((scene.inst_count, 3)).astype(np.float32)).cuda(),
            "env": torch.from_numpy(rng.standard_normal(tuple(scene._envmap[0].shape)).astype(np.float32)).cuda()}
    got = run_case(name, accel, ("emission", "env"), fill=fill)
    f = {t: v.cpu().numpy() for t, v in fill.items()}
    others = [i for i in range(scene.inst_count) if i not in GC.lights(name)]
    assert np.array_equal(got["emission"][others].view(np.int32), f["emission"][others].view(np.int32))
    assert np.array_equal(got["env"][..., 3].view(np.int32), f["env"][..., 3].view(np.int32))
    unread = ref["n_env"] == 0
    assert unread.any() and np.array_equal(got["env"][unread].view(np.int32), f["env"][unread].view(np.int32))
    # what was added is the gradient: within the bar plus the rounding of the adds into the prefilled entry — one add per row of
    # d_emission (the gather), at most one per term for a map texel, each half an ulp of at most |prefill| + sum |terms|
    for target in ("emission", "env"):
        want, a = GC.entries(ref, target)
        cut = (lambda a: a) if target == "emission" else (lambda a: a[..., :3])
        diff = np.abs(cut(got[target]).astype(np.float64) - cut(f[target]).astype(np.float64) - want)
        adds = 1.0 if target == "emission" else ref["n_env"][..., None].astype(np.float64)
        slack = GC.bar(name, target, ref) + adds * 0.5 * np.spacing((np.abs(cut(f[target])) + a).astype(np.float32)).astype(np.float64)
        print(f"[texel lighting grad add-into] {accel} {target}: largest |result - prefill - reference| {diff.max():.3e}, {(diff / slack).max():.3f} of its bar")
        assert (diff <= slack).all()
    # a chandelier: the rows of the box, the blocker and nothing else stay
    name = "chandelier_24"
    scene = case_scene(name, accel)
    fill = {"emission": torch.from_numpy(rng.standard_normal((scene.inst_count, 3)).astype(np.float32)).cuda()}
    got = run_case(name, accel, ("emission",), fill=fill)
    others = [i for i in range(scene.inst_count) if i not in GC.lights(name)]
    assert len(others) == 2
    assert np.array_equal(got["emission"][others].view(np.int32), fill["emission"].cpu().numpy()[others].view(np.int32))
    assert (got["emission"][GC.lights(name)] != fill["emission"].cpu().numpy()[GC.lights(name)]).all()


@pytest.mark.parametrize("name,split", [("env_panel_lit_16", 1), ("multi_24_spp9", 4)])
def test_the_adjoints_of_disjoint_sample_ranges_add_up_to_the_wholes(name, split):
    spp = GC.CASES[name][3]
    whole = run_case(name, "bvh", GC.targets(name))
    a, b = run_case(name, "bvh", GC.targets(name), samples=(0, split)), run_case(name, "bvh", GC.targets(name), samples=(split, spp))
    check_parity(name, a, GC.reference(name, samples=(0, split)), f"{name} samples [0, {split})")
    for target in GC.targets(name):
        cut = (lambda x: x) if target == "emission" else (lambda x: x[..., :3])
        diff = np.abs(cut(a[target]).astype(np.float64) + cut(b[target]).astype(np.float64) - cut(whole[target]).astype(np.float64))
        bar = GC.bar(name, target)
        print(f"[texel lighting grad ranges] {name} {target}: [0, {split}) + [{split}, {spp}) against the whole: largest difference {diff.max():.3e}, "
              f"{(diff / np.maximum(bar, 1e-300)).max():.3f} of its bar")
        assert (diff <= bar).all()


def test_cotangents_that_are_never_read_reach_nothing():
    name = "env_panel_lit_16"
    rch = GC.reached(name)
    assert (~rch).any()
    g = torch.from_numpy(GC.cotangent(name)).cuda()
    g[torch.from_numpy(~rch).cuda()] = float("nan")               # all four floats of every texel that is not shaded
    g[..., 3] = float("nan")                                      # the openness' cotangent of every texel
    pts = torch.from_numpy(GC.points(name)).cuda().clone()
    ys, xs = np.nonzero(rch)
    pts[ys[0], xs[0], 9] = float("nan"); g[ys[0], xs[0]] = float("nan")     # a NaN in the position: that texel is not shaded either
    scene = case_scene(name, "bvh")
    d_e, d_env = zeros(name, scene, "emission"), zeros(name, scene, "env")
    scene.texel_lighting_backward(pts, g, d_emission=d_e, d_env=d_env, **case_kw(name))
    torch.cuda.synchronize()
    assert torch.isfinite(d_e).all() and torch.isfinite(d_env).all() and float(d_e.abs().sum()) > 0 and float(d_env.abs().sum()) > 0
    # the same call with that one texel's cotangent cleared instead
    clean = torch.from_numpy(GC.cotangent(name)).cuda(); clean[ys[0], xs[0]] = 0
    want = run_case(name, "bvh", ("emission", "env"), d_out=clean)
    for target, got in (("emission", d_e.cpu().numpy()), ("env", d_env.cpu().numpy())):
        cut = (lambda x: x) if target == "emission" else (lambda x: x[..., :3])
        assert (np.abs(cut(got).astype(np.float64) - cut(want[target])) <= GC.bar(name, target)).all(), target


# -------------------------------------------------------------------------------- the autograd route
def ones_cotangent(h, w):
    g = torch.zeros(h, w, 4, device="cuda"); g[..., :3] = 1.0
    return g


def close_positive(a, b):
    """two sums of the same positive terms in two orders: 32 float32 ulps of the sum (the terms of a ones-cotangent are all positive, so
    the sum of |terms| is the entry itself)"""
    a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
    return (np.abs(a - b) <= 32 * EPS32 * np.maximum(np.abs(a), np.abs(b))).all()


def test_autograd_in_the_emissions_is_the_low_level_call_with_the_forwards_snapshot():
    name = "chandelier_24"
    A = GC.CASES[name][0]()
    scene = new_scene(name, "bvh")                                 # a handle of its own: its emissions change
    pts = torch.from_numpy(GC.points(name)).cuda()
    texels = TexelAovs(pts)
    e0 = torch.from_numpy(A.inst_emission).cuda()
    E = (0.5 * e0).requires_grad_(True)
    out = scene.texel_lighting(None, spp=4, seed=GC.SEED, texels=texels, emissions=E)
    assert out.data.requires_grad
    assert torch.equal(out.data.detach(), scene.texel_lighting_forward(pts, spp=4, seed=GC.SEED))       # E became the scene's emissions
    scene.set_emission_values(3.0 * e0)                           # between forward and backward: must change nothing
    out.irradiance.sum().backward()
    assert E.grad is not None and tuple(E.grad.shape) == (scene.inst_count, 3)
    scene.set_emission_values(0.5 * e0)
    want = torch.zeros_like(e0)
    scene.texel_lighting_backward(pts, ones_cotangent(24, 24), spp=4, seed=GC.SEED, d_emission=want)
    torch.cuda.synchronize()
    print(f"[texel lighting grad autograd] emissions: largest |autograd - low level| {float((E.grad - want).abs().max()):.3e}, largest entry {float(want.max()):.4e}")
    assert float(want[GC.lights(name)].min()) > 0 and close_positive(E.grad, want)
    assert (E.grad[[0, 7]] == 0).all()                            # the box and the blocker
    scene.check()


def test_autograd_in_an_h_by_2h_map_returns_a_gradient_of_its_own_shape():
    import envmap_tables as ET
    name = "env_panel_8x8"
    scene = Scene(GC.CASES[name][0](), integrator="direct")
    img = np.ascontiguousarray(ET.make_map("sun_sky", (16, 32)), np.float32)
    scene.add_envmap(img)
    pts = torch.from_numpy(GC.points(name)).cuda()
    env = torch.from_numpy(img[..., :3].copy()).cuda().requires_grad_(True)
    assert tuple(env.shape) == (16, 32, 3)
    out = scene.texel_lighting(None, spp=4, seed=GC.SEED, texels=TexelAovs(pts), envmap=env)
    total = out.irradiance.sum()
    total.backward()
    assert env.grad is not None and tuple(env.grad.shape) == (16, 32, 3) and torch.isfinite(env.grad).all() and float(env.grad.abs().sum()) > 0
    # Euler through the preparation of the map, which is linear in its rgb: <grad, map> = <1, F>; all terms positive
    lhs, rhs = float((env.grad.double() * env.detach().double()).sum()), float(out.irradiance.detach().double().sum())
    print(f"[texel lighting grad autograd] map: <grad, map> {lhs:.9e}  sum of the irradiance {rhs:.9e}")
    assert rhs > 0 and abs(lhs - rhs) <= 32 * EPS32 * rhs
    scene.check()


def test_both_keywords_in_one_call_and_none_of_them():
    name = "env_panel_lit_16"
    scene = new_scene(name, "bvh")
    pts = torch.from_numpy(GC.points(name)).cuda()
    texels = TexelAovs(pts)
    E = torch.from_numpy(GC.CASES[name][0]().inst_emission).cuda().requires_grad_(True)
    env = torch.from_numpy(GC.CASES[name][4]()[0]).cuda().requires_grad_(True)          # the prepared (16, 16, 4) map itself
    out = scene.texel_lighting(None, spp=4, seed=GC.SEED, texels=texels, emissions=E, envmap=env)
    g = torch.from_numpy(GC.cotangent(name)).cuda()
    (out.data * g).sum().backward()                               # float 3 carries a cotangent too: ignored
    ref = GC.reference(name)
    check_parity(name, {"emission": E.grad.cpu().numpy(), "env": env.grad.cpu().numpy()}, ref, f"{name} autograd")
    plain = scene.texel_lighting(None, spp=4, seed=GC.SEED, texels=texels)
    assert not plain.data.requires_grad and plain.data.grad_fn is None
    assert torch.equal(plain.data.view(torch.int32), scene.texel_lighting_forward(pts, spp=4, seed=GC.SEED).view(torch.int32))
    scene.check()


# -------------------------------------------------------------------------------------------- errors
def test_wrong_arguments_raise():
    name = "env_panel_lit_16"
    scene = case_scene(name, "brute")
    pts, g = torch.from_numpy(GC.points(name)).cuda(), torch.from_numpy(GC.cotangent(name)).cuda()
    d_e, d_env = zeros(name, scene, "emission"), zeros(name, scene, "env")
    L = N.lib()
    need = L.zdr_texel_lighting_backward_workspace_bytes(scene._handle, 16, 16)
    assert need >= 16 + 16 * 16 * 4 + 256 * 3 * 4 and L.zdr_texel_lighting_backward_workspace_bytes(scene._handle, 0, 16) == 0
    assert L.zdr_texel_lighting_backward_workspace_bytes(None, 16, 16) == 0
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g, spp=4)                                                      # no target
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts[..., :4].contiguous(), g, spp=4, d_emission=d_e)
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g[..., :3].contiguous(), spp=4, d_emission=d_e)
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g.double(), spp=4, d_emission=d_e)
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g, spp=4, d_emission=torch.zeros(3, 3, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g, spp=4, d_env=torch.zeros(16, 16, 3, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g, spp=4, d_emission=d_e, workspace=torch.zeros(need - 1, dtype=torch.uint8, device="cuda"))
    for samples in ((2, 2), (3, 1), (0, 5), (-1, 2)):
        with pytest.raises(ValueError):
            scene.texel_lighting_backward(pts, g, spp=4, samples=samples, d_emission=d_e)
    with pytest.raises(ValueError):
        scene.texel_lighting_backward(pts, g, spp=4, sampler="halton", d_emission=d_e)
    no_map = case_scene("cbox_16x16", "brute")
    cpts, cg = torch.from_numpy(GC.points("cbox_16x16")).cuda(), torch.from_numpy(GC.cotangent("cbox_16x16")).cuda()
    with pytest.raises(ValueError):
        no_map.texel_lighting_backward(cpts, cg, spp=4, d_env=d_env)                                      # d_env without a map
    with pytest.raises(ValueError):
        no_map.texel_lighting(None, spp=4, texels=TexelAovs(cpts), envmap=torch.zeros(16, 32, 3, device="cuda"))
    with pytest.raises(ValueError):
        no_map.texel_lighting(None, spp=4, texels=TexelAovs(cpts), emissions=torch.zeros(5, 3, device="cuda"))
    # the C entry point itself
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    def params(**kw):
        p = N.TexelLightingParams()
        p.struct_size = C.sizeof(N.TexelLightingParams)
        p.tex_h, p.tex_w, p.spp, p.sample_begin, p.sample_end, p.seed, p.sampler, p.max_distance = 16, 16, 4, 0, 4, 0, N.SAMPLER_CMJ, 1e30
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    def call(p, s=scene, texels=pts, d_out=g, e=d_e, m=d_env, ws=ws, off=(0, 0, 0)):
        return L.zdr_scene_texel_lighting_backward(s._handle, C.byref(p), texels.data_ptr() + off[0], d_out.data_ptr() + off[1], None if e is None else e.data_ptr(),
                                                   None if m is None else m.data_ptr(), ws.data_ptr() + off[2], s._stream())
    assert call(params()) == 0 and call(params(max_distance=-1.0)) == 0                                  # max_distance plays no part
    assert call(params(), e=None, m=None) == E_INVALID                                                   # both targets NULL
    assert call(params(), s=no_map, texels=cpts, d_out=cg) == E_INVALID                                  # d_env without a map
    for bad in (params(struct_size=4), params(tex_h=0), params(spp=0), params(sample_begin=4), params(sample_end=5), params(sample_begin=2, sample_end=2), params(sampler=7)):
        assert call(bad) == E_INVALID
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        assert call(params(), off=off) == E_INVALID
    assert L.zdr_scene_texel_lighting_backward(scene._handle, C.byref(params()), pts.data_ptr(), g.data_ptr(), d_e.data_ptr(), None, g.data_ptr(), scene._stream()) == E_INVALID   # workspace on d_out
    # a scene without lights: d_emission is accepted and nothing is added
    dark = case_scene("env_panel_8x8", "brute")
    kept = torch.full((dark.inst_count, 3), 2.5, device="cuda")
    dark.texel_lighting_backward(torch.from_numpy(GC.points("env_panel_8x8")).cuda(), torch.from_numpy(GC.cotangent("env_panel_8x8")).cuda(), spp=4, seed=GC.SEED, d_emission=kept)
    torch.cuda.synchronize()
    assert (kept == 2.5).all()
    scene.check(); no_map.check(); dark.check()
