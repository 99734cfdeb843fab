"""No GPU: the float64 reference of the bounced light (tests/texel_bounce_ref.py) held to account on its own, since the kernels are held
to it — an independent check of its physics against a deterministic area quadrature, the properties the header states (prefix, zero
material, sample ranges), the statement about the Cornell box's ceiling that motivates the feature, the margins table of
tests/texel_bounce_cases.py against the measurement, and the condition behind the GPU test's 1 % cap: how few walks change when every
barycentric moves by the largest float32 error the ray tests have measured."""
import os
import re

import numpy as np
import pytest

import texel_bounce_cases as BC
import texel_bounce_ref as BR
import texel_lighting_cases as LC
import texel_lighting_ref as LR
from zdr_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------- physics
def cbox_texels():
    """three texels of the Cornell case, each the most interior of its kind: on the ceiling (normal -y), on a wall (|n.x| = 1), on the floor"""
    pts = BC.points("cbox_k1")
    n, p, reach = pts[..., 4:7], pts[..., 8:11], pts[..., 12] == 1
    reach = reach & (BC.reference("cbox_k1")["data"][..., 3] > 0.5)   # (not one under a box: most of its hemisphere lands on a surface's front)
    floor_y = p[..., 1][reach].min()
    kinds = {"ceiling": reach & (n[..., 1] < -0.99), "wall": reach & (np.abs(n[..., 0]) > 0.99), "floor": reach & (n[..., 1] > 0.99) & (p[..., 1] < floor_y + 0.3)}      # (below the boxes' tops)
    out = {}
    for kind, mask in kinds.items():
        assert mask.any(), kind
        ys, xs = np.nonzero(mask)
        c = p[ys, xs].mean(0)
        k = int(np.argmin(((p[ys, xs] - c) ** 2).sum(1)))
        out[kind] = (int(ys[k]), int(xs[k]))
    return out


def quadrature(name, texel, n):
    """int albedo(y) / pi E_direct(y) cos_x cos_y / r^2 V dA over the triangles of the models with a material, each cut into n x n
    sub-triangles and sampled at their centroids: a deterministic rule.  E_direct(y): tests/texel_lighting_ref.py at y with 16 samples
    (every point has a pixel of its own, so the estimates are independent: their noise is part of the rule's error and, like it,
    shrinks with n); V: OracleScene.trace_any."""
    make, slots = BC.CASES[name][0], BC.CASES[name][1]
    arrays, osc = make(), LC.oracle_scene(make)
    geo = BR.Geometry(arrays, np.float64)
    pts = BC.points(name)
    x, nx = pts[texel][8:11].astype(np.float64), pts[texel][4:7].astype(np.float64)
    slot_of_inst = np.array([-1 if k is None else k for k in slots])
    inst_of_tri = np.repeat(np.arange(arrays.ninst), np.diff(arrays.inst_tri_begin))
    tris = np.nonzero(slot_of_inst[inst_of_tri] >= 0)[0]
    # centroids of the n^2 sub-triangles in barycentrics (u, v) of corners 1 and 2
    uv = []
    for i in range(n):
        for j in range(n - i):
            uv.append(((i + 1 / 3) / n, (j + 1 / 3) / n))
            if j < n - i - 1:
                uv.append(((i + 2 / 3) / n, (j + 2 / 3) / n))
    uv = np.array(uv)
    assert uv.shape[0] == n * n
    g = np.repeat(tris, uv.shape[0]); u = np.tile(uv[:, 0], tris.shape[0]); v = np.tile(uv[:, 1], tris.shape[0])
    inst, prim = inst_of_tri[g], g - np.asarray(arrays.inst_tri_begin)[inst_of_tri[g]]
    y, yuv, yns, yng = geo.interact(inst, prim, u, v)
    area = 0.5 * np.linalg.norm(np.cross(geo.P[g, 1] - geo.P[g, 0], geo.P[g, 2] - geo.P[g, 0]), axis=1) / uv.shape[0]
    d = y - x
    r = np.linalg.norm(d, axis=1)
    w = d / r[:, None]
    cos_x, cos_y, cos_s = (w * nx).sum(1), -(w * yng).sum(1), -(w * yns).sum(1)
    keep = (cos_x > 0) & ~(cos_y < 1e-4) & ~(cos_s < 1e-4)
    idx = np.nonzero(keep)[0]
    vis = ~LR.trace_any(osc, np.repeat(x[None], idx.size, 0), w[idx], 1e-4, r[idx] * (1 - 1e-3))
    idx = idx[vis]
    fake = np.zeros((1, idx.size, 16), np.float32)
    fake[0, :, 4:7] = yns[idx]; fake[0, :, 8:11] = y[idx]; fake[0, :, 12] = 1
    e_direct = LR.texel_lighting_ref(arrays, osc, fake, spp=16, seed=3)["data"][0, :, :3]
    total = np.zeros(3)
    for m, mat in enumerate(BC.materials(name)):
        sel = slot_of_inst[inst[idx]] == m
        if sel.any():
            k = idx[sel]
            alb = BR.read_bsdf(mat, yuv[k], np.float64)
            total += ((alb / np.pi) * e_direct[sel] * (cos_x[k] * cos_y[k] / r[k] ** 2 * area[k])[:, None]).sum(0)
    return total


def test_one_bounce_agrees_with_an_area_quadrature_of_the_radiosity_integral():
    name, spp = "cbox_k1", 4096
    texels = cbox_texels()
    pts = BC.points(name).copy()
    only = np.zeros(pts.shape[:2], bool)
    for t in texels.values():
        only[t] = True
    pts[..., 12] = np.where(only, pts[..., 12], 0)                   # the reference walks these three texels alone
    make, slots = BC.CASES[name][0], BC.CASES[name][1]
    ref = BR.texel_bounce_ref(make(), LC.oracle_scene(make), pts, BC.materials(name), slots, spp=spp, bounces=1, seed=BC.SEED)
    q = ref["queries"]
    for kind, (ty, tx) in texels.items():
        rows = (q[:, 0] == tx) & (q[:, 1] == ty)
        per = ref["add"][rows, 0]
        assert per.shape[0] == spp
        mc, se = per.mean(0), per.std(0, ddof=1) / np.sqrt(spp)
        fine, coarse = quadrature(name, (ty, tx), 12), quadrature(name, (ty, tx), 6)
        qerr = np.abs(fine - coarse)
        print(f"[texel bounce physics] {kind} texel ({tx}, {ty}): Monte Carlo {mc} +- {se} (spp {spp}); quadrature {fine} (half the grid: {coarse})")
        assert np.allclose(mc, ref["data"][ty, tx, :3], rtol=1e-9, atol=1e-12)
        assert (fine > 0).all()
        assert (np.abs(mc - fine) <= 4 * se + qerr).all(), (kind, mc, fine, se, qerr)


def test_the_interaction_is_the_oracles():
    """surface_interact of the reference (float32) against the oracle's copy, at the hits of the Cornell walks"""
    ref = BC.reference("cbox_k3", "float32")
    make = BC.CASES["cbox_k3"][0]
    have = np.arange(3)[None, :] < ref["nvert"][:, None]
    inst, prim, uv = ref["inst"][have], ref["prim"][have], ref["uv"][have]
    rows = np.zeros((inst.shape[0], 16), np.float32)
    rows[:, 0] = inst.astype(np.int32).view(np.float32); rows[:, 1] = prim.astype(np.int32).view(np.float32); rows[:, 2:4] = uv
    o = LC.oracle_scene(make).light_rows("interact", rows)
    p, tuv, ns, ng = BR.Geometry(make(), np.float32).interact(inst, prim, uv[:, 0], uv[:, 1])
    mine = np.concatenate([p, tuv, ns, ng], 1)
    err = np.abs(mine.astype(np.float64) - o[:, :11]).max()
    print(f"[texel bounce interact] {inst.shape[0]} hits: largest difference to the oracle's surface_interact {err:.3e}")
    assert err < 2e-5


# ---------------------------------------------------------------------------- properties
def test_the_prefix_property():
    k3, k1 = BC.reference("cbox_k3"), BC.reference("cbox_k1")
    k2 = BC.run_reference("cbox_k3", K=2)
    assert np.array_equal(k3["add"][:, 0], k1["add"][:, 0]) and np.array_equal(k3["add"][:, :2], k2["add"])
    assert np.array_equal(k3["beta"][:, 0], k1["beta"][:, 0]) and np.array_equal(k3["surface"], k1["surface"])
    assert (k3["add"][:, 1:] > 0).any()


def test_a_zero_material_gives_zero_irradiance_and_the_same_surface():
    ref = BC.reference("multi_k3")
    zero = BC.run_reference("multi_k3", mats=tuple(np.zeros_like(m) for m in BC.materials("multi_k3")))
    assert (zero["data"][..., :3] == 0).all() and (ref["data"][..., :3] > 0).any()
    assert np.array_equal(zero["data"][..., 3], ref["data"][..., 3]) and (ref["data"][..., 3] > 0).any()


def test_disjoint_sample_ranges_add_up():
    whole = BC.reference("cbox_k3")["data"]
    parts = BC.run_reference("cbox_k3", samples=(0, 2))["data"] + BC.run_reference("cbox_k3", samples=(2, 4))["data"]
    assert np.abs(whole - parts).max() < 1e-12
    assert np.array_equal(whole[..., 3], parts[..., 3])
    tail = BC.reference("cbox_k3_range")["data"] + BC.run_reference("cbox_k3", samples=(0, 1))["data"]
    assert np.abs(whole - tail).max() < 1e-12


def test_the_ceiling_of_the_cornell_box_has_no_direct_light_and_mostly_bounced_light():
    n, dark, lit = BC.ceiling_statement(LC.reference("cbox_16x16")["data"], BC.reference("cbox_k3")["data"], BC.points("cbox_k3"))
    reached = BC.reached("cbox_k3")
    direct0 = reached & (LC.reference("cbox_16x16")["data"][..., :3].sum(-1) == 0)
    print(f"[texel bounce ceiling] ceiling texels {n}, direct irradiance exactly 0 on {dark}, bounced light after three bounces on {lit}; reached {int(reached.sum())}, "
          f"no direct light {int(direct0.sum())}, of those with bounced light: one bounce {int((direct0 & (BC.reference('cbox_k1')['data'][..., :3].sum(-1) > 0)).sum())}, "
          f"three {int((direct0 & (BC.reference('cbox_k3')['data'][..., :3].sum(-1) > 0)).sum())}")
    assert n > 0 and dark == n
    assert lit > n // 2


def test_the_environment_case_accepts_environment_samples_at_its_bounce_vertices():
    share = BC.env_accept_share("env_k2")
    ref = BC.reference("env_k2")
    on_second = ((ref["flags"] & BR.F_ADDED) != 0) & (ref["inst"] == 1)
    print(f"[texel bounce env] {share:.3f} of the bounce vertices accept an environment sample; {int(on_second.sum())} of them on the second material")
    assert share >= 0.05 and on_second.any()


def test_vertices_land_on_a_material_that_is_not_the_baked_one():
    ref = BC.reference("multi_k3")
    on_slab = ((ref["flags"] & BR.F_SHADED) != 0) & (ref["inst"] == 3)
    assert on_slab.sum() > 10
    assert BC.materials("multi_k3")[1].shape[:2] != BC.materials("multi_k3")[0].shape[:2]


# ------------------------------------------------------------------------------- margins
@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_margins_are_the_measurement(name):
    e, same, total = BC.margin(name)
    print(f"[texel bounce margins] {name}: float32 against float64, largest error of an add {e:.3e} over {same} of {total} samples; table {BC.MARGINS[name]:.3e}")
    assert same >= (1 - BC.MAX_SET_ASIDE) * total
    assert e <= BC.MARGINS[name] <= 1.02 * e + 1e-12                  # the constant IS the measurement, rounded up
    line = [l for l in open(os.path.join(ROOT, "profiles", "texel_bounce_margins.txt")) if re.match(r"\s+%s\s+samples" % re.escape(name), l)]
    assert line and f"{e:.3e}" in line[0], (name, line)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_few_walks_change_when_every_barycentric_moves_by_the_ray_tests_error(name):
    for pattern in range(4):
        changed, total = BC.perturbed_signature_changes(name, pattern)
        print(f"[texel bounce fragility] {name}, sign pattern {pattern}: {changed} of {total} samples change signature under +-{BC.BARY_EPS:g}")
        assert changed <= BC.MAX_FRAGILE * total, (name, pattern, changed, total)


def test_the_bindings_exist():
    for sym in ("zdr_texel_bounce_workspace_bytes", "zdr_texel_bounce_lanes_shift", "zdr_scene_texel_bounce", "zdr_texel_bounce_dump"):
        assert sym in _native.EXPORTS and getattr(_native.lib(), sym).argtypes is not None
    import zdr_amd
    assert hasattr(zdr_amd, "TexelBounce")
    for name in ("texel_bounce", "texel_bounce_forward", "texel_bounce_dump"):
        assert hasattr(zdr_amd.Scene, name)
    assert "gradient" in zdr_amd.Scene.texel_bounce.__doc__
    header = open(os.path.join(ROOT, "include", "zdr.h")).read()
    assert "zdr_texel_bounce_params" in header and "#define ZDR_ABI_VERSION 4" in header
    assert os.path.exists(_native.BOUNCE_LIB_PATH)
    L = _native.lib()
    assert L.zdr_texel_bounce_lanes_shift(24, 24, 0, 9) == 3 and L.zdr_texel_bounce_lanes_shift(16, 16, 1, 4) == 1
    assert L.zdr_texel_bounce_lanes_shift(1024, 1024, 0, 16) == 0 and L.zdr_texel_bounce_lanes_shift(16, 16, 2, 2) == -1
    assert L.zdr_texel_bounce_workspace_bytes(16, 16) == 16 + 4 * 256
