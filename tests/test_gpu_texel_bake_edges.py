"""-m gpu: the bounced-light bake, its adjoint and the adjoint of the texture-space lighting (zdr_bounce.hip, zdr_bouncegrad.hip,
zdr_bakegrad.hip) at the edges of their launch shapes — the cases of BC.EDGE_CASES (tests/texel_bounce_cases.py) and GC.EDGE_CASES
(tests/texel_lighting_grad_cases.py), run through the machinery of tests/test_gpu_texel_bounce.py, tests/test_gpu_texel_bounce_grad.py and
tests/test_gpu_texel_lighting_grad.py with their bars.  tests/test_texel_bake_edges_host.py holds the conditions under which a case
crosses the branch it is meant for.

a. hall: 43 lights; a light with list index >= 32 leaves the adjoints' on-chip table and adds into the accumulator row directly.
b. cbox_k8: eight bounces, the documented maximum — the vertex records behind the BVH stacks, 55 sampler dimensions.
c. cbox_wave: a whole wave per texel, one lane per texel, and 32 lanes in two trips of which the second is ragged.
d. cbox_wide: more shade workgroups than accumulator rows and than copies of the material's cells: both modulos wrap.
e. tiny_*: material tables of 4, 28, 30 and 12 + 6 staging cells: the LDS cell array, its limit, the queue, and a non-zero m.cell.
f. cbox_k3_nan: a NaN position and a NaN normal in two waves of the compactions.
g. env_lit_k2: an environment map and a mesh light in one light list: a map sample reports no light to the hook.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import many_lights as ML
import test_gpu_texel_bounce as FWD
import test_gpu_texel_bounce_grad as ADJ
import test_gpu_texel_lighting_grad as LADJ
import texel_bounce_cases as BC
import texel_bounce_grad_ref as GR
import texel_bounce_ref as BR
import texel_lighting_grad_cases as GC
from texel_bounce_gpu import ACCELS, case_scene, run_dump, run_forward
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

NAN_A, NAN_B = ADJ.NAN_A, ADJ.NAN_B
GUARD = 4096


def forward_statements(name, accel, lanes):
    """the statements of tests/test_gpu_texel_bounce.py for one case: the shading of the dump's own hits within the case's bar, the walk
    against the free-running reference, and the buffer as the sum of the dumped adds, bit for bit, with ``lanes`` lanes per texel"""
    FWD.test_the_shading_of_the_dumps_own_hits(name, accel)
    FWD.test_the_walk_against_the_free_running_reference(name, accel)
    FWD.test_the_buffer_is_the_sum_of_the_dump_bit_for_bit(name, accel)
    q, dump = run_dump(name, accel)
    assert FWD.sum_of_dump(name, q, dump)[1] == lanes


def adjoint_parity(name, accel):
    """the kernel's gradient within the case's bars of the float64 reference on the dump's own walks, both targets in one call"""
    ref = ADJ.dump_reference(name, accel)
    dm, de = ADJ.run_backward(name, accel)
    ADJ.check(name, dm, de, ref, f"{name} {accel}")
    for j, g in enumerate(dm):
        assert np.abs(g[..., :3]).max() > 0, f"material {j} received nothing"
        assert (g[..., 3] == 0).all()
    assert np.isfinite(de).all()
    return ref, dm, de


def workspace_runs(name, accel, against_reference=True):
    """the call on a workspace of exactly the advertised size, filled with 0x00 and with 0xA5, each followed by GUARD bytes that must
    keep their bits: both results within the bars of each other and (``against_reference``) of the reference"""
    scene = case_scene(name, accel)
    ref = ADJ.dump_reference(name, accel)
    bm, be = GR.bars(name, ref)
    dims = np.ascontiguousarray(np.array([m.shape[:2] for m in BC.materials(name)], np.int32))
    H, W = BC.case(name)[2]
    need = int(N.lib().zdr_texel_bounce_backward_workspace_bytes(scene._handle, H, W, dims.ctypes.data, dims.shape[0]))
    assert need % 16 == 0 and need > 16 + 4 * H * W
    runs = []
    for fill in (0x00, 0xA5):
        buf = torch.full((need + GUARD,), fill, dtype=torch.uint8, device="cuda")
        buf[need:] = 0x5A
        runs.append(ADJ.run_backward(name, accel, workspace=buf[:need]))
        assert bool((buf[need:] == 0x5A).all()), f"{name} {accel}: the call wrote behind the {need} bytes of its workspace"
    off_m = ADJ.worst(runs[0][0], [b.astype(np.float64) for b in runs[1][0]])
    off_e = float(np.abs(runs[0][1].astype(np.float64) - runs[1][1]).max())
    print(f"[bake edges] {name} {accel}: workspace of zeros against one of 0xA5 ({need} bytes): d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
    assert off_m <= bm and off_e <= be
    if against_reference:
        ADJ.check(name, runs[1][0], runs[1][1], ref, f"{name} {accel}, workspace of 0xA5")
    scene.check()


# ------------------------------------------------------------------------------------------------ a. hall
@pytest.mark.parametrize("accel", ACCELS)
def test_lights_beyond_the_on_chip_table_in_the_bounce_adjoint(accel):
    name = "hall_k2"
    ref, dm, de = adjoint_parity(name, accel)
    lights = GR.light_rows(name)
    beyond = lights[ML.TEXEL_LDS_LIGHTS:]
    _, be = GR.bars(name, ref)
    err = np.abs(de[lights].astype(np.float64) - ref["d_emission"][lights]).max(1)
    print(f"[bake edges] {name} {accel}: {len(lights)} lights; largest error of a row with list index < 32: {err[:32].max():.3e}, >= 32: {err[32:].max():.3e} (bar {be:.3e}); "
          f"smallest |row| beyond the table {np.abs(de[beyond]).sum(1).min():.4f}")
    assert len(beyond) == 11 and (err <= be).all()                    # every light's row
    assert (np.abs(de[beyond]).sum(1) > 0).all() and (de[0] == 0).all()
    # the same gradient without the material target
    none_m, only_e = ADJ.run_backward(name, accel, d_materials=None)
    assert none_m is None
    ADJ.check(name, None, only_e, ref, f"{name} {accel}, d_materials=None")
    workspace_runs(name, accel)


@pytest.mark.parametrize("accel", ACCELS)
def test_lights_beyond_the_on_chip_table_in_the_lighting_adjoint(accel):
    name = "hall_16"
    got = LADJ.run_case(name, accel, ("emission",))
    LADJ.check_parity(name, got, GC.reference(name), f"{name} {accel}")
    beyond = GC.lights(name)[ML.TEXEL_LDS_LIGHTS:]
    assert len(beyond) == 11 and (np.abs(got["emission"][beyond]).sum(1) > 0).all()
    LADJ.case_scene(name, accel).check()


# ------------------------------------------------------------------------------------------------ b. cbox_k8
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["cbox_k8", "cbox_k8_pmj02bn"])
def test_eight_bounces_forward_dump_and_adjoint(name, accel):
    forward_statements(name, accel, 4)
    q, dump = run_dump(name, accel)
    reach = int((dump["nvert"] == 8).sum())
    accepted = ((dump["flags"] & BR.F_ADDED) != 0).sum(0)
    print(f"[bake edges] {name} {accel}: {reach} of {dump['nvert'].size} dumped samples reach vertex 8; accepted per vertex index {accepted.tolist()}")
    assert reach >= 0.10 * dump["nvert"].size and (accepted > 0).all()
    adjoint_parity(name, accel)
    case_scene(name, accel).check()


@pytest.mark.parametrize("accel", ACCELS)
def test_an_all_zero_material_gets_the_one_bounce_gradient_at_eight_bounces(accel):
    name = "cbox_k8"
    zero = tuple(np.zeros_like(m) for m in BC.materials(name))
    dm0, de0 = ADJ.run_backward(name, accel, mats=zero)
    dm1, de1 = ADJ.run_backward(name, accel, bounces=1)
    bm, _ = GR.bars(name, ADJ.dump_reference(name, accel))
    off = ADJ.worst([a[..., :3] for a in dm0], [b[..., :3].astype(np.float64) for b in dm1])
    top = max(float(np.abs(a).max()) for a in dm0)
    print(f"[bake edges] {name} {accel}: zero materials, 8 bounces against one bounce: off by at most {off:.3e} (bar {bm:.3e}); largest entry {top:.3e}")
    assert top > 0 and all(np.isfinite(a).all() for a in dm0)
    assert off <= bm
    assert (de0 == 0).all() and np.abs(de1).max() > 0                 # every beta_k is 0


# ------------------------------------------------------------------------------------------------ c. cbox_wave
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name,lanes", [("cbox_wave", 64), ("cbox_wave_one", 1), ("cbox_wave_ragged", 32)])
def test_a_whole_wave_one_lane_and_a_ragged_trip_per_texel(name, lanes, accel):
    forward_statements(name, accel, lanes)
    adjoint_parity(name, accel)


@pytest.mark.parametrize("accel", ACCELS)
def test_the_adjoints_of_ranges_with_four_lane_counts_add_up_to_the_whole(accel):
    name = "cbox_wave"
    bm, be = GR.bars(name, ADJ.dump_reference(name, accel))
    wm, we = ADJ.run_backward(name, accel)
    sm, se = [np.zeros(m.shape, np.float64) for m in wm], np.zeros(we.shape, np.float64)
    for rng in ((0, 1), (1, 3), (3, 40), (40, 64)):
        pm, pe = ADJ.run_backward(name, accel, samples=rng)
        assert max(float(np.abs(a).max()) for a in pm) > 0
        sm, se = [s + a for s, a in zip(sm, pm)], se + pe
    off_m, off_e = ADJ.worst(wm, sm), float(np.abs(we.astype(np.float64) - se).max())
    print(f"[bake edges] {name} {accel}: [0, 1) + [1, 3) + [3, 40) + [40, 64) against [0, 64): d_materials {off_m:.3e} (bar {bm:.3e}), d_emission {off_e:.3e} (bar {be:.3e})")
    assert off_m <= bm and off_e <= be


# ------------------------------------------------------------------------------------------------ d. cbox_wide
@pytest.mark.parametrize("accel", ACCELS)
def test_accumulator_rows_and_cell_copies_wrap_in_the_bounce_adjoint(accel):
    """This case found a disagreement between the bake and its adjoint.  With brute force one of the 19,520 samples (texel (33, 20),
    sample 15) has a light sample at its first vertex whose shadow ray leaves the wall at a grazing angle (c / pdf = 4.35e-05); the
    forward accepts it, and k_bgrad_shade<BruteAccel>, whose compilation rounded it.p.x unlike every kernel of zdr_bounce.hip, rejected it:
    texel (18, 54) of d_materials was off by 1.677e-05 against this bar of 1.520e-05.  bgrad_interact (zdr_bouncegrad.hip) now spells
    the forward's rounding out; measured since: 3.657e-06, and 3.756e-06 with the BVH."""
    name = "cbox_wide"
    ref = ADJ.dump_reference(name, accel)
    # the emission rows first (the accumulator's modulo), then the workspace (what holds for brute force too runs before what does not)
    none_m, only_e = ADJ.run_backward(name, accel, d_materials=None)
    assert none_m is None
    ADJ.check(name, None, only_e, ref, f"{name} {accel}, d_materials=None")
    workspace_runs(name, accel, against_reference=False)
    adjoint_parity(name, accel)
    only_m, none_e = ADJ.run_backward(name, accel, d_emission=None)
    assert none_e is None
    ADJ.check(name, only_m, None, ref, f"{name} {accel}, d_emission=None")


@pytest.mark.parametrize("accel", ACCELS)
def test_accumulator_rows_wrap_in_the_lighting_adjoint(accel):
    name = "cbox_wide_40"
    LADJ.check_parity(name, LADJ.run_case(name, accel, ("emission",)), GC.reference(name), f"{name} {accel}")
    LADJ.case_scene(name, accel).check()


# ------------------------------------------------------------------------------------------------ e. tiny tables
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", ["tiny_1x1", "tiny_3x6", "tiny_4x5", "tiny_multi"])
def test_material_tables_about_the_lds_cell_limit(name, accel):
    ref = ADJ.dump_reference(name, accel)
    scene = case_scene(name, accel)
    # into targets whose roughness channel holds a NaN with a payload: it keeps its bits
    pre = []
    for m in BC.materials(name):
        b = np.zeros(m.shape, np.float32)
        b.view(np.uint32)[..., 3] = NAN_B
        pre.append(torch.from_numpy(b).cuda())
    dm, de = ADJ.run_backward(name, accel, d_materials=pre)
    for g in dm:
        assert (g.view(np.uint32)[..., 3] == NAN_B).all()
        assert (np.abs(g[..., :3]).reshape(-1, 3).sum(1) > 0).all()  # every texel of these few is read
    ADJ.check(name, dm, de, ref, f"{name} {accel}")
    workspace_runs(name, accel)


@pytest.mark.parametrize("accel", ACCELS)
def test_the_1x1_gradient_is_the_sum_of_the_16x16_gradient_of_the_same_walks(accel):
    """d/dc of the bake with the constant c everywhere is the sum over the texels of the gradient at the constant material; the walks do
    not depend on the materials (zdr_bouncegrad.hip), so both calls run the same walks"""
    one, big = "tiny_1x1", "cbox_k3"
    (m1,) = BC.materials(one)
    const = (np.ascontiguousarray(np.broadcast_to(m1, BC.materials(big)[0].shape)),)
    (d1,), _ = ADJ.run_backward(one, accel)
    (d16,), _ = ADJ.run_backward(big, accel, mats=const)
    _, dump = run_dump(big, accel)
    ref16 = GR.texel_bounce_grad_ref(GR.case_records(big, dump), const, GR.cotangent(big))
    bar1, bar16 = GR.bars(one, ADJ.dump_reference(one, accel))[0], GR.bars(big, ref16)[0]
    a, b = d1[0, 0, :3].astype(np.float64), d16[..., :3].astype(np.float64).sum((0, 1))
    off16 = float(np.abs(d16[..., :3] - ref16["d_materials"][0][..., :3]).max())
    print(f"[bake edges] {accel}: d_materials of the 1 x 1 material {a}, the constant 16 x 16 material's summed over its texels {b}: differ by {np.abs(a - b).max():.3e} "
          f"(bars {bar1:.3e} + {bar16:.3e}); the 16 x 16 gradient against its reference {off16:.3e}")
    assert off16 <= bar16
    assert np.abs(a - b).max() <= bar1 + bar16


# ------------------------------------------------------------------------------------------------ f. NaN sample points
@pytest.mark.parametrize("accel", ACCELS)
def test_nan_sample_points_are_skipped_by_both_compactions(accel):
    name, clean = "cbox_k3_nan", "cbox_k3"
    (ya, xa, _), (yb, xb, _) = BC.nan_texels(name)
    got, base = run_forward(name, accel), run_forward(clean, accel)
    assert (got[[ya, yb], [xa, xb]] == 0).all() and (base[[ya, yb], [xa, xb], :3] > 0).any()
    other = np.ones(got.shape[:2], bool)
    other[[ya, yb], [xa, xb]] = False
    diff = int((got.view(np.uint32)[other] != base.view(np.uint32)[other]).any(-1).sum())
    print(f"[bake edges] {name} {accel}: the two NaN texels are zeros; other texels whose bits differ from the run without the NaNs: {diff}")
    assert diff == 0
    # the adjoint: NaNs with a payload in all four cotangents of both texels; the reference has no sample of either
    g = GR.cotangent(name).copy()
    g.view(np.uint32)[[ya, yb], [xa, xb]] = np.array([[NAN_A], [NAN_B]], np.uint32)
    ref = ADJ.dump_reference(name, accel)
    dm, de = ADJ.run_backward(name, accel, d_out=torch.from_numpy(g).cuda())
    assert all(np.isfinite(d).all() for d in dm) and np.isfinite(de).all()
    ADJ.check(name, dm, de, ref, f"{name} {accel}")
    assert ref["n_terms"] < ADJ.dump_reference(clean, accel)["n_terms"]
    case_scene(name, accel).check()


# ------------------------------------------------------------------------------------------------ g. env_lit_k2
@pytest.mark.parametrize("accel", ACCELS)
def test_an_environment_map_and_a_mesh_light_in_one_light_list(accel):
    name = "env_lit_k2"
    forward_statements(name, accel, 4)
    ref, dm, de = adjoint_parity(name, accel)
    _, dump = run_dump(name, accel)
    rec = GR.case_records(name, dump)
    mesh, env = int((rec["added"] & (rec["light"] >= 0)).sum()), int((rec["added"] & (rec["light"] < 0)).sum())
    _, be = GR.bars(name, ref)
    err = float(np.abs(de[1].astype(np.float64) - ref["d_emission"][1]).max())
    print(f"[bake edges] {name} {accel}: accepted samples from the mesh light {mesh}, from the map {env}; the light's row {de[1]} off by {err:.3e} (bar {be:.3e})")
    assert mesh >= 0.10 * (mesh + env) and env >= 0.10 * (mesh + env)
    assert err <= be and np.abs(de[1]).min() > 0 and (de[0] == 0).all()
    case_scene(name, accel).check()
