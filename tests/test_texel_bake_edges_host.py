"""No GPU: the conditions the edge cases of the texture-space bakes rest on (BC.EDGE_CASES of tests/texel_bounce_cases.py, GC.EDGE_CASES
of tests/texel_lighting_grad_cases.py; the GPU tests are tests/test_gpu_texel_bake_edges.py), checked on the float64 references alone: a
case that is meant to cross a branch of the kernels must cross it in the reference's own walks, or the GPU test proves nothing.

1. hall: the lights with list index >= 32 (past the adjoints' on-chip table) carry at least 5 % of sum |d_emission| and none of them is 0,
   for the bounce adjoint and for the lighting adjoint.
2. cbox_k8: at least 10 % of the samples reach the eighth vertex, and a light sample is accepted at every vertex index.
3. cbox_wave: the lanes rule of csrc/bounce.h, restated here, gives a whole wave, one lane and 32 lanes in two trips.
4. cbox_wide: more live shade workgroups than accumulator rows (256) and than copies of the 64 x 64 material's cells.
5. tiny_*: 4, 28, 30 and 12 + 6 staging cells about ZDR_LDS_CELLS = 28.
6. cbox_k3_nan: the two NaN texels lie in different waves of the compaction.
7. env_lit_k2: environment samples and mesh-light samples are each at least 10 % of the accepted samples.
8. The margins tables are the measurement, the caps of the old cases hold unchanged, and the evaluator and the complex step pin the
   reference's gradient on the new shapes too.
Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest

import many_lights as ML
import texel_bounce_cases as BC
import texel_bounce_grad_ref as GR
import texel_bounce_ref as BR
import texel_lighting_grad_cases as GC
from zdr_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIGHTS = ML.TEXEL_LDS_LIGHTS     # ZDR_BGRAD_LDS_LIGHTS = ZDR_LGRAD_LDS_LIGHTS
ACC_ROWS = 256                       # ZDR_BGRAD_COPIES = ZDR_LGRAD_COPIES
LDS_CELLS = 28                       # ZDR_LDS_CELLS
MAX_LANES = 64                       # ZDR_BOUNCE_MAX_LANES
EDGES = list(BC.EDGE_CASES)


def lanes_shift(ntexels, nsamples):
    """zdr_bounce_lanes_shift (csrc/bounce.h), restated"""
    want, cap, shift = (262144 + ntexels - 1) // ntexels, min(nsamples, MAX_LANES), 0
    while (2 << shift) <= cap and (1 << shift) < want:
        shift += 1
    return shift


def cell_copies(cells):
    """cell_copies_for (zdr_api.cpp): the copies of a lone material's staging cells"""
    return min(1024, (1 << 20) // cells) if cells < (1 << 16) else 1


def cells(name):
    return [(h + 1) * (w + 1) for h, w in BC.material_sizes(name)]


# ------------------------------------------------------------------------------------------------ 1. hall
def test_the_halls_lights_past_the_table_carry_a_share_of_both_adjoints():
    arrays = ML.hall_arrays()
    lights = GR.light_rows("hall_k2")
    assert arrays.ninst == 44 and lights == list(range(1, 44)) and lights == GC.lights("hall_16")
    assert BC.case("hall_k2")[1].count(0) == 1 and len(BC.case("hall_k2")[1]) == 44
    for label, d in (("bounce adjoint", GR.reference_grad("hall_k2")["d_emission"]), ("lighting adjoint", GC.reference("hall_16")["d_emission"])):
        rows = np.abs(d[lights]).sum(1)
        share = rows[LDS_LIGHTS:].sum() / rows.sum()
        print(f"[bake edges] hall, {label}: {len(lights)} lights, those with list index >= {LDS_LIGHTS} carry {share:.3f} of sum |d_emission|; "
              f"their smallest row sum {rows[LDS_LIGHTS:].min():.4f}, the largest of all {rows.max():.4f}")
        assert len(lights) - LDS_LIGHTS == 11
        assert share >= 0.05 and (rows[LDS_LIGHTS:] > 0).all()
        assert (np.abs(d[lights]) > 0).all()


# ------------------------------------------------------------------------------------------------ 2. cbox_k8
@pytest.mark.parametrize("name", ["cbox_k8", "cbox_k8_pmj02bn"])
def test_walks_reach_the_eighth_vertex_and_every_vertex_index_accepts_light(name):
    ref = BC.reference(name)
    assert BC.bounces(name) == 8 == _native_max_bounces()
    reach = int((ref["nvert"] == 8).sum())
    accepted = ((ref["flags"] & BR.F_ADDED) != 0).sum(0)
    print(f"[bake edges] {name}: {reach} of {ref['nvert'].size} samples reach vertex 8; accepted light samples per vertex index {accepted.tolist()}; "
          f"sampler dimensions per sample {2 + 7 * 8 - 3}")
    assert reach >= 0.10 * ref["nvert"].size
    assert (accepted > 0).all()
    if name in BC.SAMPLERS:
        assert 2 + 7 * 8 - 3 > BC.SAMPLERS[name][0]                  # far more dimensions than the seeded tables have sets


def _native_max_bounces():
    header = open(os.path.join(ROOT, "zdr_amd", "csrc", "bounce.h")).read()
    return int(re.search(r"#define ZDR_BOUNCE_MAX_BOUNCES (\d+)", header).group(1))


# ------------------------------------------------------------------------------------------------ 3. lanes
def test_the_lanes_rule_gives_a_whole_wave_one_lane_and_a_ragged_second_trip():
    L = _native.lib()
    H, W = BC.case("cbox_wave")[2]
    got = {}
    for name in ("cbox_wave", "cbox_wave_one", "cbox_wave_ragged"):
        begin, end = BC.RANGES.get(name) or (0, BC.case(name)[4])
        got[name] = lanes_shift(H * W, end - begin)
        print(f"[bake edges] {name}: {H} x {W} texels, samples [{begin}, {end}): shift {got[name]}, {(end - begin + (1 << got[name]) - 1) >> got[name]} trips")
        assert L.zdr_texel_bounce_lanes_shift(H, W, begin, end) == got[name]
    assert got == {"cbox_wave": 6, "cbox_wave_one": 0, "cbox_wave_ragged": 5}
    assert 32 < 37 < 64                                              # two trips of 32 lanes, 5 samples in the second
    for (h, w, b, e) in ((24, 24, 0, 9), (16, 16, 1, 4), (1024, 1024, 0, 16), (40, 40, 0, 16), (8, 8, 1, 3), (8, 8, 40, 64)):
        assert L.zdr_texel_bounce_lanes_shift(h, w, b, e) == lanes_shift(h * w, e - b)
    # the adjoint's ranges of cbox_wave: 1, 2, 37 and 24 samples
    assert [lanes_shift(64, n) for n in (1, 2, 37, 24)] == [0, 1, 5, 4]


# ------------------------------------------------------------------------------------------------ 4. cbox_wide
def test_the_wide_case_has_more_workgroups_than_rows_and_than_copies():
    name = "cbox_wide"
    H, W = BC.case(name)[2]
    spp = BC.case(name)[4]
    reach = int(BC.reached(name).sum())
    shift = lanes_shift(H * W, spp)
    groups = (reach << shift) // 64
    (one,) = cells(name)
    copies = cell_copies(one)
    print(f"[bake edges] {name}: {reach} reached texels x {1 << shift} lanes / 64 = {groups} live shade workgroups; accumulator rows {ACC_ROWS}; "
          f"a {BC.material_sizes(name)[0]} material has {one} cells, {copies} copies")
    assert BC.reference(name)["nvert"].size == reach * spp <= 20000
    assert groups > ACC_ROWS and groups > copies > 1 and one > LDS_CELLS
    # the lighting adjoint on the same points: its lanes rule is the same (csrc/bake.h)
    assert GC.case("cbox_wide_40")[2:4] == ((H, W), spp) and np.array_equal(GC.points("cbox_wide_40"), BC.points(name))
    # and every workgroup beyond row 255 has something to add: texels at the list's end are lit
    d = GR.reference_grad(name)
    assert np.abs(d["d_emission"]).max() > 0 and np.abs(d["d_materials"][0]).max() > 0


# ------------------------------------------------------------------------------------------------ 5. tiny tables
def test_the_tiny_tables_lie_about_the_lds_limit():
    got = {name: cells(name) for name in ("tiny_1x1", "tiny_3x6", "tiny_4x5", "tiny_multi")}
    print(f"[bake edges] staging cells of the tiny tables: {got} (the LDS path holds at most {LDS_CELLS})")
    assert got == {"tiny_1x1": [4], "tiny_3x6": [28], "tiny_4x5": [30], "tiny_multi": [12, 6]}
    assert sum(got["tiny_3x6"]) == LDS_CELLS < sum(got["tiny_4x5"]) and sum(got["tiny_multi"]) <= LDS_CELLS
    assert cell_copies(30) == 1024
    for name in got:
        grad = GR.reference_grad(name)
        for j, d in enumerate(grad["d_materials"]):
            assert (np.abs(d[..., :3]).reshape(-1, 3).sum(1) > 0).all(), f"{name}: a texel of material {j} gets no gradient"
            assert (d[..., 3] == 0).all()
    # vertices land on both materials of the two-material table
    rec = GR.reference_records("tiny_multi")
    assert (rec["slot"][rec["shaded"]] == 0).sum() > 10 and (rec["slot"][rec["shaded"]] == 1).sum() > 10


def test_the_1x1_gradient_is_the_sum_of_the_16x16_gradient_of_a_constant_material():
    """d/dc of the bake with the constant c everywhere = the sum over the texels of the gradient at the constant material: the walks do not
    depend on the materials, so both run on the same records"""
    (m1,) = BC.materials("tiny_1x1")
    const = (np.ascontiguousarray(np.broadcast_to(m1, (16, 16, 4))),)
    a = GR.reference_grad("tiny_1x1")["d_materials"][0][0, 0, :3]
    b = GR.texel_bounce_grad_ref(GR.reference_records("cbox_k3"), const, GR.cotangent("cbox_k3"))["d_materials"][0][..., :3].sum((0, 1))
    print(f"[bake edges] tiny_1x1: d_materials {a}, the sum over the texels of the constant 16 x 16 material's {b}")
    assert np.array_equal(BC.points("tiny_1x1"), BC.points("cbox_k3")) and np.array_equal(GR.cotangent("tiny_1x1"), GR.cotangent("cbox_k3"), equal_nan=True)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


# ------------------------------------------------------------------------------------------------ 6. NaN points
def test_the_nan_points_lie_in_two_waves_of_the_compaction():
    name = "cbox_k3_nan"
    (ya, xa, fa), (yb, xb, fb) = BC.nan_texels(name)
    W = BC.case(name)[2][1]
    ta, tb = ya * W + xa, yb * W + xb
    clean = BC.points("cbox_k3")
    print(f"[bake edges] {name}: NaN in float {fa} of texel {ta} and in float {fb} of texel {tb}")
    assert 8 <= fa < 11 and 4 <= fb < 7                              # a position, a normal
    assert abs(ta - tb) >= 64 and ta // 64 != tb // 64
    assert clean[ya, xa, 12] == 1 and clean[yb, xb, 12] == 1
    pts = BC.points(name)
    assert np.isnan(pts).sum() == 2 and np.isnan(pts[ya, xa, fa]) and np.isnan(pts[yb, xb, fb])
    assert BC.reference(name)["nvert"].size == BC.reference("cbox_k3")["nvert"].size - 2 * BC.case(name)[4]
    # the samples of the other texels are those of the clean case
    q, qc = BC.reference(name)["queries"], BC.reference("cbox_k3")["queries"]
    keep = ~(((qc[:, 0] == xa) & (qc[:, 1] == ya)) | ((qc[:, 0] == xb) & (qc[:, 1] == yb)))
    assert np.array_equal(q, qc[keep]) and np.array_equal(BC.reference(name)["add"], BC.reference("cbox_k3")["add"][keep])
    assert (BC.reference(name)["data"][[ya, yb], [xa, xb]] == 0).all()


# ------------------------------------------------------------------------------------------------ 7. env_lit_k2
def test_environment_and_mesh_light_samples_are_both_accepted():
    name = "env_lit_k2"
    rec = GR.reference_records(name)
    mesh, env = int((rec["added"] & (rec["light"] >= 0)).sum()), int((rec["added"] & (rec["light"] < 0)).sum())
    print(f"[bake edges] {name}: accepted samples from the mesh light {mesh}, from the environment map {env}")
    assert mesh + env == int(rec["added"].sum()) > 0
    assert mesh >= 0.10 * (mesh + env) and env >= 0.10 * (mesh + env)
    assert GR.light_rows(name) == [1] and np.abs(GR.reference_grad(name)["d_emission"][1]).min() > 0


# ------------------------------------------------------------------------------------------------ 8. the references on the new shapes
@pytest.mark.parametrize("name", EDGES)
def test_the_bounce_margins_are_the_measurement(name):
    e, same, total = BC.margin(name)
    print(f"[bake edges] {name}: float32 against float64, largest error of an add {e:.3e} over {same} of {total} samples; table {BC.MARGINS[name]:.3e}")
    assert total <= 20000
    assert same >= (1 - BC.MAX_SET_ASIDE) * total
    assert e <= BC.MARGINS[name] <= 1.02 * e + 1e-12                  # the constant IS the measurement, rounded up
    line = [l for l in open(os.path.join(ROOT, "profiles", "texel_bounce_margins.txt")) if re.match(r"\s+%s\s+samples" % re.escape(name), l)]
    assert line and f"{e:.3e}" in line[0], (name, line)


@pytest.mark.parametrize("name", EDGES)
def test_the_bounce_adjoints_margins_are_the_measurement(name):
    (em, ee), (sm, se) = GR.margin(name)
    print(f"[bake edges] {name}: float32 margin d_materials {em:.3e} (largest entry {sm:.3e}), d_emission {ee:.3e} (largest entry {se:.3e})")
    pm, pe = GR.MARGINS[name]
    assert em <= pm <= 1.02 * em + 1e-12, (em, pm)
    assert ee <= pe <= 1.02 * ee + 1e-12, (ee, pe)
    assert sm > 0 and se > 0


@pytest.mark.parametrize("name", list(GC.EDGE_CASES))
def test_the_lighting_adjoints_margins_are_the_measurement(name):
    ref, r32 = GC.reference(name), GC.reference(name, "float32")
    rch = GC.reached(name)
    uncertain = int((rch & ref["uncertain"]).sum())
    e = GC.error(name, "emission", GC.entries(r32, "emission")[0])
    print(f"[bake edges] {name}: float32 vs float64 {e:.3e}; margin {GC.MARGINS[name]['emission']}; uncertain texels {uncertain} of {int(rch.sum())}")
    assert GC.targets(name) == ("emission",) and sorted(GC.MARGINS[name]) == ["emission"]
    assert uncertain <= GC.MAX_UNCERTAIN * rch.sum()
    assert e <= GC.MARGINS[name]["emission"] <= 1.02 * e + 1e-12


@pytest.mark.parametrize("name", EDGES)
def test_few_walks_change_when_every_barycentric_moves_by_the_ray_tests_error(name):
    for pattern in range(4):
        changed, total = BC.perturbed_signature_changes(name, pattern)
        print(f"[bake edges] {name}, sign pattern {pattern}: {changed} of {total} samples change signature under +-{BC.BARY_EPS:g}")
        assert changed <= BC.MAX_FRAGILE * total, (name, pattern, changed, total)


@pytest.mark.parametrize("name", ["hall_k2", "cbox_k8", "tiny_multi", "env_lit_k2"])
def test_the_evaluator_reproduces_the_bake_and_the_emission_gradient_is_its_complex_step(name):
    ref, rec, mats = BC.reference(name), GR.reference_records(name), BC.materials(name)
    out = GR.bake_eval(rec, mats)
    err, top = float(np.abs(out - ref["data"][..., :3]).max()), float(np.abs(ref["data"][..., :3]).max())
    print(f"[bake edges] {name}: evaluator against the reference's bake: {err:.3e} of {top:.3e}")
    assert top > 0 and err <= 1e-12 * top
    g = GR.cotangent(name).astype(np.float64)[..., :3]
    g = np.where(np.isnan(g), 0.0, g)
    grad = GR.reference_grad(name)
    em = np.asarray(BC.case(name)[0]().inst_emission, np.float64).reshape(-1, 3)
    etop, worst = float(np.abs(grad["d_emission"]).max()), 0.0
    for i in GR.light_rows(name):
        for ch in range(3):
            step = em.astype(np.complex128)
            step[i, ch] += 1e-20j
            d = float((GR.bake_eval(rec, [np.asarray(m, np.float64) for m in mats], step).imag * g).sum() / 1e-20)
            worst = max(worst, abs(d - grad["d_emission"][i, ch]))
    print(f"[bake edges] {name}: d_emission against the complex step: {worst:.3e} of {etop:.3e}")
    assert etop > 0 and worst <= 1e-9 * etop
