"""-m gpu: the texture-space lighting (Scene.texel_lighting; include/zdr.h, zdr_scene_texel_lighting) against the float64 reference of
tests/texel_lighting_ref.py on the cases of tests/texel_lighting_cases.py, for both accelerators, and the properties the header states:
sample ranges add up, the same bits from run to run, doubled emissions double the irradiance exactly, openness is a count over spp, the
high-level call is the low-level one on the scene's own texel buffers, and the argument checks.

The kernels get the case's float32 sample points (texel_lighting_cases.points), the floats the reference was given.  A texel fails when
its irradiance is off the float64 reference by more than the case's bar (4 x the float32 reference's own error, floor 4 float32 ulps of
the largest irradiance) or its openness differs at all; failing and uncertain texels together may be 1 % of the reached ones.  Every
figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import texel_lighting_cases as LC
from zdr_amd import Scene, TexelLighting, float3
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -3            # ZDR_E_* of include/zdr.h

_scenes = {}


def case_scene(name, accel):
    make, env = LC.case(name)[0], LC.case(name)[5]
    key = (make, env, accel, LC.SAMPLERS.get(name))
    if key not in _scenes:
        scene = Scene(make(), integrator="direct", accel=accel)
        if name in LC.SAMPLERS:                                   # a handle of its own, with the tables the reference draws from
            scene.set_pmj02bn_tables(*LC.pmj_tables(name))
        if env:                                                   # the tables the reference uses, as they are (add_envmap would build them again)
            tex, prob, alias, pdf, mw, mh = env()
            N.check(N.lib().zdr_scene_set_envmap(scene._handle, tex.ctypes.data, tex.shape[0], tex.shape[1], prob.ctypes.data, alias.ctypes.data,
                                                 pdf.ctypes.data, mw, mh))
            scene.env_count = 1
            scene._envmap = (tex, prob, alias, pdf)
        assert scene.info()["accel"] == accel
        _scenes[key] = scene
    return _scenes[key]


def case_points(name):
    return torch.from_numpy(LC.points(name)).cuda()


def run_case(name, accel, **kw):
    _, _, _, spp, max_distance, _ = LC.case(name)
    kw.setdefault("samples", LC.RANGES.get(name))
    out = case_scene(name, accel).texel_lighting_forward(case_points(name), spp=spp, seed=LC.SEED, max_distance=max_distance,
                                                         sampler="pmj02bn" if name in LC.SAMPLERS else None, **kw)
    torch.cuda.synchronize()
    return out


def check_parity(name, got, ref, tag):
    reached, unc = LC.reached(name), ref["uncertain"] & LC.reached(name)
    fail = LC.failing(name, got, ref) & reached
    err = np.abs(got[..., :3].astype(np.float64) - ref["data"][..., :3]).max(-1)
    keep = reached & ~unc
    print(f"[texel lighting parity] {tag}: reached {int(reached.sum())}, uncertain {int(unc.sum())}, failing {int(fail.sum())} "
          f"(openness differs on {int(((got[..., 3] != ref['data'][..., 3].astype(np.float32)) & reached).sum())}); irradiance: kernel vs float64 "
          f"largest {err[keep].max():.3e}, 99th percentile {np.percentile(err[keep], 99):.3e}; float32 reference {LC.MARGINS[name]:.3e}; bar {LC.bar(name):.3e}; "
          f"largest irradiance {LC.scale(name):.4e}")
    assert (got[~reached] == 0).all()
    assert (fail | unc).sum() <= LC.MAX_UNCERTAIN * reached.sum(), (tag, int(fail.sum()), int(unc.sum()), int(reached.sum()))


# ------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("accel", ["brute", "bvh"])
@pytest.mark.parametrize("name", [n for n in LC.CASES if n not in LC.SAMPLERS])
def test_parity_with_the_float64_reference(name, accel):
    check_parity(name, run_case(name, accel).cpu().numpy(), LC.reference(name), f"{name} {accel}")


@pytest.mark.parametrize("accel", ["brute", "bvh"])
@pytest.mark.parametrize("name", list(LC.SAMPLERS))
def test_parity_with_the_pmj02bn_sampler(name, accel):
    """with tables of several sets, and with one set of exactly spp samples where the last lanes of a texel run out of samples"""
    check_parity(name, run_case(name, accel).cpu().numpy(), LC.reference(name), f"{name} {accel}")
    case_scene(name, accel).check()


def test_parity_of_a_single_sample_on_one_lane_per_texel():
    """a range of one sample: one lane per texel, the route of the large textures"""
    name = "multi_24_spp9"
    check_parity(name, run_case(name, "bvh", samples=(4, 5)).cpu().numpy(), LC.reference(name, samples=(4, 5)), f"{name} bvh samples [4, 5)")


# --------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_disjoint_sample_ranges_add_up_to_the_whole(accel):
    name = "cbox_64x64"
    whole = run_case(name, accel).cpu().numpy().astype(np.float64)
    parts = run_case(name, accel, samples=(0, 2)).cpu().numpy().astype(np.float64) + run_case(name, accel, samples=(2, 4)).cpu().numpy().astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(whole), np.abs(parts)).astype(np.float32)).astype(np.float64)
    off = np.abs(whole - parts) / ulp
    print(f"[texel lighting ranges] {accel}: [0, 2) + [2, 4) against [0, 4): largest difference {off.max():.2f} ulps of the larger value")
    assert (off <= 4.0).all()
    assert np.array_equal(whole[..., 3], parts[..., 3])               # counts over spp: quarters are exact


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_two_runs_give_the_same_bits(accel):
    name = "multi_24_spp9"
    scene, pts = case_scene(name, accel), case_points(name)
    need = N.lib().zdr_texel_lighting_workspace_bytes(24, 24)
    a = scene.texel_lighting_forward(pts, spp=9, seed=LC.SEED, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda")).clone()
    b = scene.texel_lighting_forward(pts, spp=9, seed=LC.SEED, out=torch.full((24, 24, 4), 7.0, device="cuda"),
                                     workspace=torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(a[..., :3].sum()) > 0


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_doubled_emissions_double_the_irradiance_bit_for_bit(accel):
    name = "multi_24_spp4"
    A = LC.CASES[name][0]()
    scene = Scene(A, integrator="direct", accel=accel)              # a handle of its own: its lights change
    pts = case_points(name)
    once = scene.texel_lighting_forward(pts, spp=4, seed=LC.SEED).clone()
    scene.update_lights([float3(*(2.0 * float(c) for c in e)) for e in A.inst_emission])
    twice = scene.texel_lighting_forward(pts, spp=4, seed=LC.SEED)
    torch.cuda.synchronize()
    assert float(once[..., :3].sum()) > 0
    assert torch.equal((2.0 * once[..., :3]).view(torch.int32), twice[..., :3].contiguous().view(torch.int32))
    assert torch.equal(once[..., 3], twice[..., 3])
    scene.check()


@pytest.mark.parametrize("name", ["multi_24_spp9", "cbox_16x16_ao"])
def test_openness_is_a_count_over_spp(name):
    spp = LC.CASES[name][3]
    got = run_case(name, "bvh").cpu().numpy()[..., 3]
    assert (got >= 0).all() and (got <= 1).all()
    k = np.rint(got.astype(np.float64) * spp)
    assert np.array_equal(got, (k / spp).astype(np.float32))
    assert len(np.unique(k)) > 2


def test_the_high_level_call_is_the_low_level_call_on_the_scenes_texel_buffers():
    name = "multi_24_spp4"
    scene = Scene(LC.CASES[name][0](), integrator="direct")
    scene.material_slots = list(LC.MULTI_SLOTS)
    material = torch.rand(24, 24, 4, device="cuda")
    texels = scene.texel_aovs(material)
    got = scene.texel_lighting(material, spp=4, seed=3)
    assert isinstance(got, TexelLighting) and got.data.shape == (24, 24, 4) and got.irradiance.shape == (24, 24, 3) and got.openness.shape == (24, 24)
    want = scene.texel_lighting_forward(texels.data, spp=4, seed=3)
    assert torch.equal(got.data, want)
    assert torch.equal(scene.texel_lighting(material, spp=4, seed=3, texels=texels).data, want)
    assert torch.equal(scene.texel_lighting(material, spp=4, seed=3, samples=(1, 3), max_distance=0.5).data,
                       scene.texel_lighting_forward(texels.data, spp=4, seed=3, samples=(1, 3), max_distance=0.5))
    assert (got.data[texels.reach == 0] == 0).all() and float(got.irradiance.sum()) > 0 and not got.data.requires_grad
    # the kernels' own sample points against the reference's: the same lighting up to what the points differ by
    ref = LC.reference(name)["data"]
    mine = scene.texel_lighting_forward(texels.data, spp=4, seed=LC.SEED).cpu().numpy()
    same = np.abs(mine - ref).max(-1) <= 1e-3 * LC.scale(name)
    print(f"[texel lighting] kernel sample points against the reference's: {int((~same).sum())} of {same.size} texels differ by more than 1e-3 of the largest irradiance")
    assert (~same).sum() <= 0.02 * same.size
    scene.check()


def test_a_nan_in_position_or_normal_gives_four_zeros():
    name = "cbox_16x16"
    pts = case_points(name).clone()
    ys, xs = np.nonzero(LC.reached(name))
    pts[ys[0], xs[0], 9] = float("nan"); pts[ys[1], xs[1], 4] = float("nan")
    got = case_scene(name, "bvh").texel_lighting_forward(pts, spp=4, seed=LC.SEED)
    clean = run_case(name, "bvh")
    assert (got[ys[0], xs[0]] == 0).all() and (got[ys[1], xs[1]] == 0).all()
    mask = torch.ones(16, 16, dtype=torch.bool, device="cuda"); mask[ys[0], xs[0]] = False; mask[ys[1], xs[1]] = False
    assert torch.equal(got[mask], clean[mask])
    case_scene(name, "bvh").check()


# -------------------------------------------------------------------------------------------- errors
def test_wrong_arguments_raise():
    name = "cbox_16x16"
    scene, pts = case_scene(name, "brute"), case_points(name)
    need = N.lib().zdr_texel_lighting_workspace_bytes(16, 16)
    assert need >= 16 * 16 * 4 and N.lib().zdr_texel_lighting_workspace_bytes(0, 16) == 0 and N.lib().zdr_texel_lighting_workspace_bytes(16, -1) == 0
    with pytest.raises(ValueError):
        scene.texel_lighting_forward(pts[..., :4].contiguous(), spp=4)                      # not 16 channels
    with pytest.raises(ValueError):
        scene.texel_lighting_forward(pts.double(), spp=4)
    with pytest.raises(ValueError):
        scene.texel_lighting_forward(pts, spp=4, out=torch.zeros(16, 16, 3, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_lighting_forward(pts, spp=4, workspace=torch.zeros(need - 1, dtype=torch.uint8, device="cuda"))
    for samples in ((2, 2), (3, 1), (0, 5), (-1, 2)):
        with pytest.raises(ValueError):
            scene.texel_lighting_forward(pts, spp=4, samples=samples)
    with pytest.raises(ValueError):
        scene.texel_lighting_forward(pts, spp=4, sampler="halton")
    with pytest.raises(ValueError):
        scene.texel_lighting_forward(pts, spp=0)                                            # no range is a subrange of [0, 0)
    with pytest.raises(N.ZdrError):
        scene.texel_lighting_forward(pts, spp=4, max_distance=0.0)
    # the C entry point itself
    L = N.lib()
    out = torch.zeros(16, 16, 4, device="cuda"); ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    def params(**kw):
        p = N.TexelLightingParams()
        p.struct_size = C.sizeof(N.TexelLightingParams)
        p.tex_h, p.tex_w, p.spp, p.sample_begin, p.sample_end, p.seed, p.sampler, p.max_distance = 16, 16, 4, 0, 4, 0, N.SAMPLER_CMJ, 1e30
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    def call(p, texels=pts, out=out, ws=ws, off=(0, 0, 0)):
        return L.zdr_scene_texel_lighting(scene._handle, C.byref(p), texels.data_ptr() + off[0], out.data_ptr() + off[1], ws.data_ptr() + off[2], scene._stream())
    assert call(params()) == 0
    for bad in (params(struct_size=4), params(tex_h=0), params(spp=0), params(sample_begin=4), params(sample_end=5), params(sample_begin=2, sample_end=2),
                params(sampler=7), params(max_distance=float("nan")), params(max_distance=-1.0)):
        assert call(bad) == E_INVALID
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        assert call(params(), off=off) == E_INVALID
    assert L.zdr_scene_texel_lighting(scene._handle, C.byref(params()), pts.data_ptr(), None, ws.data_ptr(), scene._stream()) == E_INVALID
    big = torch.zeros(16 * 16 * 4 + need // 4 + 64, device="cuda")                          # out and workspace in one buffer
    assert L.zdr_scene_texel_lighting(scene._handle, C.byref(params()), pts.data_ptr(), big.data_ptr(), big.data_ptr() + 16, scene._stream()) == E_INVALID
    assert L.zdr_scene_texel_lighting(scene._handle, C.byref(params()), pts.data_ptr(), pts.data_ptr() + 64, ws.data_ptr(), scene._stream()) == E_INVALID
    fresh = Scene(LC.CASES[name][0](), integrator="direct")                                 # pmj02bn without tables
    assert L.zdr_scene_texel_lighting(fresh._handle, C.byref(params(sampler=N.SAMPLER_PMJ02BN)), pts.data_ptr(), out.data_ptr(), ws.data_ptr(), fresh._stream()) == E_UNSUPPORTED
    torch.cuda.synchronize()
    scene.check()
