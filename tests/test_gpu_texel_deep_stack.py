"""-m gpu: the six texture-space kernel families that cast rays through BvhAccel on a BVH that needs more traversal-stack entries than
they keep in LDS — the shaft of tests/texel_deep_cases.py, 24 entries against ZDR_BVH_LDS_STACK = 12 — run through the machinery and with
the bars of each family's own tests.  tests/test_texel_deep_stack_host.py holds the conditions under which the cases' segments leave the
LDS part; no other texel test runs the one-entry-at-a-time push of BvhAccel::consume, its patched pop, or a launch with lds_stack = 12.

Which test reaches which launch function on a scene with bvh_stack_entries > 12:
  texel_lighting_forward (zdr_bake.hip)             test_lighting_and_openness_on_the_shaft
  texel_lighting_backward (zdr_bakegrad.hip)        test_the_lighting_adjoint_on_the_shaft
  texel_bounce_forward, texel_bounce_dump           test_the_bounce_forward_and_its_dump_on_the_shaft
  (zdr_bounce.hip)
  texel_bounce_backward (zdr_bouncegrad.hip)        test_the_bounce_adjoint_on_the_shaft, and with the record block of eight bounces behind
                                                    the 12-entry stacks test_eight_bounces_of_records_behind_a_twelve_entry_stack
  texel_bounce_backward_env (zdr_bounceenv.hip)     test_the_bounce_adjoint_in_the_map_on_the_shaft,
                                                    test_the_bake_on_the_shaft_is_linear_in_the_map
  texel_view_forward (zdr_project.hip)              test_the_view_down_the_shaft
Each checks parity with the float64 reference by the family's own bar, agreement of the free-running walks where the family dumps them
(what catches a dropped or duplicated stack entry: a comparison on the dump's own hits cannot), BVH against brute force on the same
scene, and scene.check() after the calls: no ZDR_DEVERR_BVH_BUDGET.  The launch functions expose no query for the dynamic LDS they ask
for, so the run at eight bounces checks parity only.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import test_gpu_texel_bake_edges as EDGES
import test_gpu_texel_bounce as FWD
import test_gpu_texel_bounce_envgrad as ENVG
import test_gpu_texel_bounce_grad as ADJ
import test_gpu_texel_lighting as LIGHT
import test_gpu_texel_lighting_grad as LADJ
import test_gpu_texel_project as VIEW
import texel_bounce_cases as BC
import texel_bounce_env_cases as EC
import texel_bounce_envgrad_ref as ER
import texel_bounce_grad_ref as GR
import texel_bounce_ref as BR
import texel_deep_cases as DC
import texel_lighting_cases as LC
import texel_lighting_grad_cases as GC
import texel_project_cases as PC
from texel_bounce_gpu import ACCELS, case_scene, run_dump, run_forward

pytestmark = pytest.mark.gpu

LANES = 8        # 144 texels, 8 samples: one lane per sample (zdr_bounce_lanes_shift)


def deep(scene, accel):
    """the handle's tree is the one the host test measured: more entries than the LDS part holds; and nothing raised a device error"""
    info = scene.info()
    if accel == "bvh":
        assert info["accel"] == "bvh" and info["bvh_stack_entries"] > DC.LDS_STACK, info
        assert info["bvh_stack_entries"] == DC.host_bvh(scene_make(scene))[2]
    scene.check()


def scene_make(scene):
    for make in (DC.shaft_arrays, DC.shaft_open_arrays):
        if scene._arrays is make():
            return make
    raise AssertionError("not a scene of tests/texel_deep_cases.py")


# ------------------------------------------------------------------------------------------------ texel_bounce_forward, texel_bounce_dump
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["shaft_k3", "shaft_pmj02bn_k3", "shaft_env_k3"])
def test_the_bounce_forward_and_its_dump_on_the_shaft(name, accel):
    """the estimator on the dump's own hits within max(4 x MARGINS, 4 ulps), the free-running walks against the float64 reference's at
    MIN_WALK_AGREEMENT, the buffer as the sum of the dump bit for bit"""
    EDGES.forward_statements(name, accel, LANES)
    q, dump = run_dump(name, accel)
    ref = BC.reference(name)
    accepted, want = int(((dump["flags"] & BR.F_ADDED) != 0).sum()), int(((ref["flags"] & BR.F_ADDED) != 0).sum())
    print(f"[deep stack] {name} {accel}: accepted light samples {accepted} (the free-running reference: {want}); vertices {int(dump['nvert'].sum())} ({int(ref['nvert'].sum())})")
    assert accepted > 0
    deep(case_scene(name, accel), accel)


@pytest.mark.parametrize("name", ["shaft_k3", "shaft_env_k3"])
def test_bvh_and_brute_force_agree_on_the_bounce_forward(name):
    (q, a), (_, b) = run_dump(name, "brute"), run_dump(name, "bvh")
    same = BR.signature_equal(a, b)
    fa, fb = run_forward(name, "brute"), run_forward(name, "bvh")
    err = np.abs(fa[..., :3].astype(np.float64) - fb[..., :3]).max()
    print(f"[deep stack] {name}: brute force against BVH: signatures agree on {int(same.sum())} of {same.size} samples; irradiance differs by at most {err:.3e} "
          f"over all texels (the estimator's bar: {BC.bar(name):.3e})")
    assert same.sum() >= (1 - 2 * (1 - BC.MIN_WALK_AGREEMENT) - 2 * BC.MAX_SET_ASIDE) * same.size   # each agrees with the reference on 99 %, flags on 99 %
    assert np.array_equal(fa[..., 3], fb[..., 3])
    assert err <= BC.bar(name)
    deep(case_scene(name, "bvh"), "bvh")


# ------------------------------------------------------------------------------------------------ texel_bounce_backward
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["shaft_k3", "shaft_env_lit_k3"])
def test_the_bounce_adjoint_on_the_shaft(name, accel):
    """materials and emissions within their bars of the float64 reference on the dump's own walks; rec_offset = 12 x 64 with the BVH"""
    ref, dm, de = EDGES.adjoint_parity(name, accel)
    assert np.abs(de[2]).min() > 0 and (de[:2] == 0).all()           # the cap's row, and nothing else
    deep(case_scene(name, accel), accel)


@pytest.mark.parametrize("accel", ACCELS)
def test_eight_bounces_of_records_behind_a_twelve_entry_stack(accel):
    """K = 8: the largest record block, (12 x 64 + 8 x ZDR_BGRAD_FIELDS x 64) x 4 bytes of dynamic LDS with the BVH.  The walks first."""
    name = "shaft_k8"
    FWD.test_the_walk_against_the_free_running_reference(name, accel)
    q, dump = run_dump(name, accel)
    reach = int((dump["nvert"] == 8).sum())
    accepted = ((dump["flags"] & BR.F_ADDED) != 0).sum(0)
    print(f"[deep stack] {name} {accel}: {reach} of {dump['nvert'].size} dumped samples reach vertex 8; accepted per vertex index {accepted.tolist()}")
    assert reach >= 0.10 * dump["nvert"].size
    EDGES.adjoint_parity(name, accel)
    deep(case_scene(name, accel), accel)


@pytest.mark.parametrize("name", ["shaft_k3", "shaft_k8"])
def test_bvh_and_brute_force_agree_on_the_bounce_adjoint(name):
    bm, be = GR.bars(name, ADJ.dump_reference(name, "brute"))
    (am, ae), (bm_, be_) = ADJ.run_backward(name, "brute"), ADJ.run_backward(name, "bvh")
    off_m, off_e = ADJ.worst(am, [b.astype(np.float64) for b in bm_]), float(np.abs(ae.astype(np.float64) - be_).max())
    print(f"[deep stack] {name}: brute force against BVH: d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
    assert off_m <= bm and off_e <= be
    deep(case_scene(name, "bvh"), "bvh")


# ------------------------------------------------------------------------------------------------ texel_bounce_backward_env
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", list(DC.BOUNCE_ENV))
def test_the_bounce_adjoint_in_the_map_on_the_shaft(name, accel):
    """BenvRays keeps the whole stack of 24 entries in LDS: d_env within its bar of the float64 reference on the dump's own walks, the
    header's counts those of the reference, and the dump's walks those of the free-running reference"""
    ref = ENVG.dump_reference(name, accel)
    got, header = ENVG.run_backward(name, accel)
    ENVG.check(name, got, ref, f"{name} {accel}")
    print(f"[deep stack] {name} {accel}: header {header}; the reference counts {ref['n_samples']} accepted environment samples")
    assert np.abs(got[..., :3]).max() > 0
    assert (got[..., 3] == 0).all() and (got[~ref["read"]] == 0).all()
    assert header[0] == len(ref["rec"]["ys"]) and header[1] == ref["n_samples"] and 0 < header[2] <= header[1]
    dump, free = ENVG.run_dump(name, accel), EC.reference(name)
    agree = BR.triangles_equal(free, dump)
    print(f"[deep stack] {name} {accel}: nvert and triangles agree with the free-running reference on {int(agree.sum())} of {agree.size} samples")
    assert agree.sum() >= BC.MIN_WALK_AGREEMENT * agree.size
    deep(ENVG.case_scene(name, accel), accel)


@pytest.mark.parametrize("name", list(DC.BOUNCE_ENV))
def test_bvh_and_brute_force_agree_on_the_adjoint_in_the_map(name):
    bar = ER.bar(name, ENVG.dump_reference(name, "brute"))
    (a, ha), (b, hb) = ENVG.run_backward(name, "brute"), ENVG.run_backward(name, "bvh")
    e = ENVG.off_by(a, b.astype(np.float64))
    print(f"[deep stack] {name}: brute force against BVH: {e:.3e} (two bars {2 * bar:.3e}); header {ha} and {hb}")
    assert e <= 2 * bar
    assert ha[:2] == hb[:2]                                           # shaded texels and accepted environment samples
    deep(ENVG.case_scene(name, "bvh"), "bvh")


@pytest.mark.parametrize("accel", ACCELS)
def test_the_bake_on_the_shaft_is_linear_in_the_map(accel):
    """the dot-product test of tests/test_gpu_texel_bounce_envgrad.py against the GPU forward, on the shaft"""
    name = "shaft_env_k3"
    ENVG.dot_product_against_the_gpu_forward(name, accel)
    deep(ENVG.case_scene(name, accel), accel)


# ------------------------------------------------------------------------------------------------ texel_lighting_forward
def test_lighting_and_openness_on_the_shaft():
    """irradiance within the bar and openness equal for both accelerators; and BVH against brute force within two bars"""
    name = "shaft_16_ao"
    got = {}
    for accel in ACCELS:
        got[accel] = LIGHT.run_case(name, accel).cpu().numpy()
        LIGHT.check_parity(name, got[accel], LC.reference(name), f"{name} {accel}")
        deep(LIGHT.case_scene(name, accel), accel)
    rch = LC.reached(name)
    d = np.abs(got["brute"][..., :3].astype(np.float64) - got["bvh"][..., :3]).max(-1)
    off = (d > 2 * LC.bar(name)) | (got["brute"][..., 3] != got["bvh"][..., 3])
    print(f"[deep stack] {name}: brute force against BVH: irradiance differs by at most {d[rch].max():.3e} (two bars {2 * LC.bar(name):.3e}); texels off or with "
          f"another openness {int((off & rch).sum())} of {int(rch.sum())}; lit texels {int((got['bvh'][..., :3].sum(-1) > 0).sum())}, mean openness {got['bvh'][..., 3][rch].mean():.3f}")
    assert (off & rch).sum() <= LC.MAX_UNCERTAIN * rch.sum()
    assert (got["bvh"][..., :3].sum(-1)[rch] > 0).any() and (got["bvh"][..., 3][rch] > 0).any() and (got["bvh"][..., 3][rch] == 0).any()


# ------------------------------------------------------------------------------------------------ texel_lighting_backward
@pytest.mark.parametrize("name", list(DC.LIGHTING_GRAD))
def test_the_lighting_adjoint_on_the_shaft(name):
    """the emissions' and the map's gradient within their bars for both accelerators, each target alone and both in one call; and BVH
    against brute force within two bars per entry"""
    got = {}
    for accel in ACCELS:
        for which in LADJ.modes(name):
            got[accel] = LADJ.run_case(name, accel, which)
            LADJ.check_parity(name, got[accel], GC.reference(name), f"{name} {accel} {'+'.join(which)}")
        deep(LADJ.case_scene(name, accel), accel)
    for target in GC.targets(name):                                   # (the last mode holds every target of the case)
        cut = (lambda a: a) if target == "emission" else (lambda a: a[..., :3])
        d = np.abs(cut(got["brute"][target]).astype(np.float64) - cut(got["bvh"][target]))
        bar = GC.bar(name, target)
        print(f"[deep stack] {name} {target}: brute force against BVH: largest difference {d.max():.3e}, {(d / np.maximum(2 * bar, 1e-300)).max():.3f} of two bars")
        assert (d <= 2 * bar).all() and np.abs(got["bvh"][target]).max() > 0


# ------------------------------------------------------------------------------------------------ texel_view_forward
def test_the_view_down_the_shaft():
    """visible equal and every channel within its bar for both accelerators; and BVH against brute force: visible equal, two bars"""
    name = "shaft_open_16_above"
    ref, reached = PC.reference(name), PC.reached(name)
    got = {}
    for accel in ACCELS:
        VIEW.test_view_parity_with_the_float64_reference(name, accel)
        got[accel] = VIEW.run_case(name, accel).cpu().numpy()
        deep(VIEW.case_scene(name, accel), accel)
    vis = int(((got["bvh"][..., 0] == 1) & reached).sum())
    off = got["brute"][..., 0] != got["bvh"][..., 0]
    for c, bar in zip(range(1, 7), PC.bars(name)):
        off |= ~(np.abs(got["brute"][..., c].astype(np.float64) - got["bvh"][..., c]) <= 2 * bar)
    print(f"[deep stack] {name}: visible texels {vis} of {int(reached.sum())} (the reference: {PC.classes(name)[3]}); brute force against BVH: texels with another "
          f"visibility or a channel off by more than two bars {int((off & reached).sum())}")
    assert (off & reached).sum() <= PC.MAX_UNCERTAIN * reached.sum()
    assert abs(vis - PC.classes(name)[3]) <= PC.MAX_UNCERTAIN * reached.sum()
