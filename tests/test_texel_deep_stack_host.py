"""No GPU: the conditions the cases on the shaft rest on (tests/texel_deep_cases.py; the GPU tests are
tests/test_gpu_texel_deep_stack.py), checked on the float64 references alone with the walk's mirror (tests/test_bvh_emulation.py, traverse)
over the host builder's records: a case that is meant to push the kernels' traversal stacks past their LDS part must do so on the
reference's own segments, or the GPU test proves nothing.  Conditions, not measurements:

1. the builder's stack_entries is > 12 (ZDR_BVH_LDS_STACK) and <= ZDR_BVH_STACK for both variants of the scene;
2. at least 25 % of the closest-hit segments that leave the texels (vertex 0 of the bounce families, the openness segments of
   texel_lighting) keep more than 12 entries pending;
3. at least 50 % of the shadow / visibility segments of positive length that leave the texels keep more than 12 pending (texel_lighting,
   its adjoint, texel_view);
4. bounce families: at least 20 shadow segments from vertices k >= 1 exceed 12;
5. no segment's pending set reaches stack_entries - 4: the premise of BenvRays (zdr_bounceenv.hip), whose whole stack lives in LDS and
   whose ``deep`` is never reached, on real rays;
6. the caps of the bounce cases (MAX_SET_ASIDE, MIN_WALK_AGREEMENT, MAX_FRAGILE) hold on the float32 against the float64 references;
7. the margins are the measurement (float32 reference against float64 reference, never a GPU result), and profiles/texel_deep_stack.txt
   holds them;
8. the cases are what tests/texel_deep_cases.py says: light is accepted, both materials get a gradient, the map and the cap are both
   sampled where both are present, the view sees the floor down the shaft.
Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import texel_bounce_cases as BC
import texel_bounce_env_cases as EC
import texel_bounce_envgrad_ref as ER
import texel_bounce_grad_ref as GR
import texel_bounce_ref as BR
import texel_deep_cases as DC
import texel_lighting_cases as LC
import texel_lighting_grad_cases as GC
import texel_project_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = DC.LDS_STACK
MIN_LOBE_SHARE = 0.25
MIN_SHADOW_SHARE = 0.50
MIN_LATER_SHADOWS = 20
BOUNCE = list(DC.BOUNCE)


def _define(header, name):
    text = open(os.path.join(ROOT, "zdr_amd", "csrc", header)).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


def profile():
    return open(os.path.join(ROOT, "profiles", "texel_deep_stack.txt")).read()


def all_segments(name):
    """every pending set the reference's segments of a case reach, whatever the family"""
    if name in DC.BOUNCE:
        s = DC.bounce_segments(name)
        return np.concatenate(s["lobe"] + s["shadow"])
    if name in DC.LIGHTING:
        return np.concatenate(list(DC.lighting_segments(name).values()))
    if name in DC.LIGHTING_GRAD:
        return DC.lighting_grad_segments(name)["shadow"]
    return DC.view_segments(name)["shadow"]


# ------------------------------------------------------------------------------------------------ 1. the tree
@pytest.mark.parametrize("make", [DC.shaft_arrays, DC.shaft_open_arrays], ids=["shaft", "shaft_open"])
def test_the_builder_asks_for_more_stack_entries_than_the_lds_part_holds(make):
    nodes, isect, entries = DC.host_bvh(make)
    A = make()
    print(f"[deep stack] {make.__name__}: {isect.shape[0]} triangles in {A.ninst} instances, {nodes.shape[0]} nodes, stack entries {entries}; "
          f"ZDR_BVH_LDS_STACK {_define('scene.h', 'ZDR_BVH_LDS_STACK')}, ZDR_BVH_STACK {_define('scene.h', 'ZDR_BVH_STACK')}")
    assert _define("scene.h", "ZDR_BVH_LDS_STACK") == LDS
    assert LDS < entries <= _define("scene.h", "ZDR_BVH_STACK")
    assert isect.shape[0] == A.tris.shape[0] == 12 + DC.TOWER + (2 if make is DC.shaft_arrays else 0)
    assert list(np.diff(A.inst_tri_begin)) == [12, DC.TOWER] + ([2] if make is DC.shaft_arrays else [])
    assert [bool((e > 0).any()) for e in A.inst_emission] == [False, False] + ([True] if make is DC.shaft_arrays else [])


# ------------------------------------------------------------------------------------------------ 2. to 5. the segments
@pytest.mark.parametrize("name", BOUNCE)
def test_the_walks_of_the_bounce_cases_leave_the_lds_part(name):
    s = DC.bounce_segments(name)
    entries = DC.host_bvh(BC.case(name)[0])[2]
    lobe0, later = DC.share(s["lobe"][0]), DC.share(np.concatenate(s["shadow"][1:]))
    top = int(all_segments(name).max())
    print(f"[deep stack] {name}: closest-hit segments of vertex 0: {lobe0[0]} of {lobe0[1]} exceed {LDS} ({lobe0[0] / lobe0[1]:.3f}); shadow segments from vertices "
          f"k >= 1: {later[0]} of {later[1]} exceed {LDS}; largest pending set of any segment {top} (stack entries {entries})")
    assert lobe0[1] == BC.reference(name)["nvert"].size
    assert lobe0[0] >= MIN_LOBE_SHARE * lobe0[1]
    assert later[0] >= MIN_LATER_SHADOWS
    assert LDS < top < entries - 4


@pytest.mark.parametrize("name", list(DC.LIGHTING))
def test_the_segments_of_the_lighting_case_leave_the_lds_part(name):
    s = DC.lighting_segments(name)
    entries = DC.host_bvh(LC.case(name)[0])[2]
    lobe, shadow = DC.share(s["lobe"]), DC.share(s["shadow"])
    max_distance = LC.case(name)[4]
    print(f"[deep stack] {name}: openness segments (max_distance {max_distance}): {lobe[0]} of {lobe[1]} exceed {LDS} ({lobe[0] / lobe[1]:.3f}); shadow segments: "
          f"{shadow[0]} of {shadow[1]} ({shadow[0] / shadow[1]:.3f}); largest pending set {max(lobe[2], shadow[2])} (stack entries {entries})")
    assert max_distance > DC.GAP + DC.SPACING * DC.TOWER + DC.RISE    # longer than the shaft: an openness ray up the shaft ends on the cap
    assert lobe[1] == int(LC.reached(name).sum()) * LC.case(name)[3]
    assert lobe[0] >= MIN_LOBE_SHARE * lobe[1]
    assert shadow[1] > 0 and shadow[0] >= MIN_SHADOW_SHARE * shadow[1]
    assert LDS < max(lobe[2], shadow[2]) < entries - 4


@pytest.mark.parametrize("name", list(DC.LIGHTING_GRAD))
def test_the_segments_of_the_lighting_adjoints_cases_leave_the_lds_part(name):
    shadow = DC.share(DC.lighting_grad_segments(name)["shadow"])
    entries = DC.host_bvh(GC.case(name)[0])[2]
    print(f"[deep stack] {name}: shadow segments: {shadow[0]} of {shadow[1]} exceed {LDS} ({shadow[0] / shadow[1]:.3f}); largest pending set {shadow[2]} (stack entries {entries})")
    assert shadow[1] > 0 and shadow[0] >= MIN_SHADOW_SHARE * shadow[1]
    assert LDS < shadow[2] < entries - 4


@pytest.mark.parametrize("name", list(DC.VIEW))
def test_the_visibility_segments_of_the_view_leave_the_lds_part(name):
    vis = DC.share(DC.view_segments(name)["shadow"])
    entries = DC.host_bvh(LC.case(PC.case(name)[0])[0])[2]
    c = PC.classes(name)
    print(f"[deep stack] {name}: visibility segments: {vis[0]} of {vis[1]} exceed {LDS} ({vis[0] / vis[1]:.3f}); largest pending set {vis[2]} (stack entries {entries}); "
          f"reached {c[0]}, behind {c[1]}, outside {c[2]}, visible {c[3]}, occluded {c[4]}, seen from behind {c[5]}, uncertain {c[6]}")
    assert PC.case(name)[2] == (64, 64)
    assert vis[1] == c[0] - c[1] - c[2] and vis[0] >= MIN_SHADOW_SHARE * vis[1]
    assert LDS < vis[2] < entries - 4
    # the camera looks down the shaft: every texel lies in front of it and inside its image, the open half is seen, the tower hides the other
    assert c[1] == 0 and c[2] == 0 and c[3] >= 0.4 * c[0] and c[4] >= 0.4 * c[0]
    assert c[6] <= PC.MAX_UNCERTAIN_REF * c[0]


# ------------------------------------------------------------------------------------------------ 6. the caps of the bounce cases
@pytest.mark.parametrize("name", BOUNCE)
def test_the_caps_of_the_bounce_cases_hold_on_the_shaft(name):
    a, b = BC.reference(name), BC.reference(name, "float32")
    same, walk = BR.signature_equal(a, b), BR.triangles_equal(a, b)
    print(f"[deep stack] {name}: float32 against float64 reference: signatures agree on {int(same.sum())} of {same.size}, nvert and triangles on {int(walk.sum())}")
    assert same.size <= 20000
    assert same.sum() >= (1 - BC.MAX_SET_ASIDE) * same.size
    assert walk.sum() >= BC.MIN_WALK_AGREEMENT * walk.size
    for pattern in range(4):
        changed, total = BC.perturbed_signature_changes(name, pattern)
        print(f"[deep stack] {name}, sign pattern {pattern}: {changed} of {total} samples change signature under +-{BC.BARY_EPS:g}")
        assert changed <= BC.MAX_FRAGILE * total, (name, pattern, changed, total)


# ------------------------------------------------------------------------------------------------ 7. the margins
@pytest.mark.parametrize("name", BOUNCE)
def test_the_bounce_margins_are_the_measurement(name):
    e, same, total = BC.margin(name)
    (em, ee), (sm, se) = GR.margin(name)
    pm, pe = GR.MARGINS[name]
    print(f"[deep stack] {name}: float32 against float64, largest error of an add {e:.3e} over {same} of {total} samples (table {BC.MARGINS[name]:.3e}); "
          f"adjoint: d_materials {em:.3e} (table {pm:.3e}, largest entry {sm:.3e}), d_emission {ee:.3e} (table {pe:.3e}, largest entry {se:.3e})")
    assert e <= BC.MARGINS[name] <= 1.02 * e + 1e-12                  # the constant IS the measurement, rounded up
    assert em <= pm <= 1.02 * em + 1e-12 and ee <= pe <= 1.02 * ee + 1e-12
    assert sm > 0 and (se > 0) == bool(GR.light_rows(name))
    line = [l for l in profile().splitlines() if re.match(r"\s+%s\s+samples" % re.escape(name), l)]
    assert line and f"{e:.3e}" in line[0], (name, line)
    line = [l for l in profile().splitlines() if re.match(r"\s+%s\s+terms" % re.escape(name), l)]
    assert line and f"{em:.3e}" in line[0] and f"{ee:.3e}" in line[0], (name, line)


@pytest.mark.parametrize("name", list(DC.BOUNCE_ENV))
def test_the_map_adjoints_margins_are_the_measurement(name):
    e, s = ER.margin(name)
    print(f"[deep stack] {name}: float32 margin of d_env {e:.3e} (table {ER.margin_of(name):.3e}, largest entry {s:.3e})")
    assert e <= ER.margin_of(name) <= 1.02 * e + 1e-12 and s > 0
    line = [l for l in profile().splitlines() if re.match(r"\s+%s\s+walks" % re.escape(name), l)]
    assert line and f"{e:.3e}" in line[0], (name, line)


@pytest.mark.parametrize("name", list(DC.LIGHTING))
def test_the_lighting_margin_is_the_measurement(name):
    ref = LC.reference(name)
    rch = LC.reached(name)
    e = LC.error(name, LC.reference(name, "float32")["data"])
    uncertain = int((rch & ref["uncertain"]).sum())
    print(f"[deep stack] {name}: float32 vs float64 irradiance {e:.3e} (table {LC.MARGINS[name]:.3e}); uncertain texels {uncertain} of {int(rch.sum())}; "
          f"lit texels {int((ref['lit'] > 0).sum())}, mean openness {float(ref['data'][..., 3][rch].mean()):.3f}")
    assert uncertain <= LC.MAX_UNCERTAIN * rch.sum()
    assert e <= LC.MARGINS[name] <= 1.02 * e + 1e-12
    assert f"{e:.3e}" in [l for l in profile().splitlines() if re.match(r"\s+%s\s+reached" % re.escape(name), l)][0]
    # both outputs carry information: lit and unlit texels, open and closed ones
    opn = ref["data"][..., 3][rch]
    assert (ref["lit"][rch] > 0).any() and (ref["lit"][rch] == 0).any() and (opn == 0).any() and (opn > 0).any()


@pytest.mark.parametrize("name", list(DC.LIGHTING_GRAD))
def test_the_lighting_adjoints_margins_are_the_measurement(name):
    ref, r32 = GC.reference(name), GC.reference(name, "float32")
    rch = GC.reached(name)
    uncertain = int((rch & ref["uncertain"]).sum())
    assert sorted(GC.MARGINS[name]) == sorted(GC.targets(name))
    assert uncertain <= GC.MAX_UNCERTAIN * rch.sum()
    row = [l for l in profile().splitlines() if re.match(r"\s+%s\s+reached" % re.escape(name), l)][0]
    for target in GC.targets(name):
        e = GC.error(name, target, GC.entries(r32, target)[0])
        print(f"[deep stack] {name} {target}: float32 vs float64 {e:.3e}; table {GC.MARGINS[name][target]:.3e}; uncertain texels {uncertain} of {int(rch.sum())}")
        assert e <= GC.MARGINS[name][target] <= 1.02 * e + 1e-12
        assert np.abs(GC.entries(ref, target)[0]).max() > 0 and f"{e:.3e}" in row


@pytest.mark.parametrize("name", list(DC.VIEW))
def test_the_views_margins_are_the_measurement(name):
    e = PC.errors(name, PC.reference(name, "float32")["data"])
    print(f"[deep stack] {name}: float32 vs float64 per channel {['%.3e' % x for x in e]}; table {['%.3e' % x for x in PC.MARGINS[name]]}")
    for x, m in zip(e, PC.MARGINS[name]):
        assert x <= m <= 1.02 * x + 1e-12
    row = [l for l in profile().splitlines() if re.match(r"\s+cosine \d", l)][0]                  # (the host's row: the kernels' rows read "cosine: kernel vs ...")
    assert all(f"{x:.3e}" in row for x in e)


# ------------------------------------------------------------------------------------------------ 8. the cases are what they say
@pytest.mark.parametrize("name", BOUNCE)
def test_the_bounce_cases_accept_light_and_both_materials_get_a_gradient(name):
    make, slots, hw, second, spp, K, env, _ = BC.case(name)
    ref, rec, grad = BC.reference(name), GR.reference_records(name), GR.reference_grad(name)
    accepted = ((ref["flags"] & BR.F_ADDED) != 0).sum(0)
    on_tower = int(((ref["inst"] == 1) & ((ref["flags"] & BR.F_SHADED) != 0)).sum())
    on_floor = int(((ref["inst"] == 0) & ((ref["flags"] & BR.F_SHADED) != 0)).sum())
    print(f"[deep stack] {name}: {ref['nvert'].size} samples, accepted light samples per vertex index {accepted.tolist()}; shaded vertices on the tower {on_tower}, on the floor {on_floor}; "
          f"largest |d_materials| per material {[float(np.abs(d).max()) for d in grad['d_materials']]}")
    assert hw[0] <= 16 and hw[1] <= 16 and 4 <= spp <= 8 and K in (3, 8)
    assert [m.shape[:2] for m in BC.materials(name)] == [hw, second] and second != hw
    assert accepted.sum() >= 20 and on_tower >= 100 and on_floor >= 100
    assert all(np.abs(d[..., :3]).max() > 0 for d in grad["d_materials"])
    if K == 8:
        assert int((ref["nvert"] == 8).sum()) >= 0.10 * ref["nvert"].size      # the whole record block is written
    if env is not None:
        mesh, sky = int((rec["added"] & (rec["light"] >= 0)).sum()), int((rec["added"] & (rec["light"] < 0)).sum())
        print(f"[deep stack] {name}: accepted samples from the cap {mesh}, from the map {sky}")
        assert sky >= 20 and (mesh >= 10) == (make is DC.shaft_arrays)
        assert np.abs(ER.reference_grad(name)["d_env"]).max() > 0
        assert EC.case(name)["shared"] == name and EC.case(name)["make"] is make


def test_the_sampler_and_the_tables_of_the_cases():
    assert list(DC.BOUNCE_SAMPLERS) == ["shaft_pmj02bn_k3"] and BC.SAMPLERS["shaft_pmj02bn_k3"] == (5, 256)
    assert not set(DC.BOUNCE) & (set(BC.CASES) | set(BC.EDGE_CASES)) and not set(DC.BOUNCE_ENV) & set(EC.CASES)
    assert not (set(DC.LIGHTING) | set(DC.LIGHTING_POINTS)) & set(LC.CASES) and not set(DC.LIGHTING_GRAD) & (set(GC.CASES) | set(GC.EDGE_CASES))
    assert not set(DC.VIEW) & set(PC.CASES)
    a, b = BC.reference("shaft_k3"), BC.reference("shaft_pmj02bn_k3")
    assert not np.array_equal(a["uv"], b["uv"])                       # another sampler, other walks
    assert GC.targets("shaft_16") == ("emission",) and GC.targets("shaft_env_lit_16") == ("emission", "env")
