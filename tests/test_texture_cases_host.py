"""The cases of tests/texture_cases.py judged without a GPU: the float64 reference against the oracle's read_bsdf / write_bsdf_grad, the
conditions on the inputs, the exactness precondition, the measurement behind K, the storage regimes as DESIGN.md states them, and proof
that the judge bites — six one-line faults in the float32 restatement, every one of them rejected."""
import os

import numpy as np
import pytest

import texture_cases as tc

F64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [("borders", tc.general_case("borders", (s,)), True) for s in [(4, 4), (3, 6), (4, 5), (7, 1), (37, 91)]] + \
        [("borders", tc.general_case("borders", tuple(tc.TABLES["copies"]), env=True), False)]


def exact_cases():
    return [tc.exact_case((s,)) for s in tc.EXACT_SIZES] + [tc.exact_case(((2, 3), s, (1, 1))) for s in tc.EXACT_SIZES[:6]] + \
           [tc.exact_case(tuple(tc.TABLES["lds"])), tc.exact_case(((17, 33), (3, 5)), True)]


# ----------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (5, 5), (9, 1), (17, 33)])
def test_reference_equals_the_oracle_on_the_exact_family(size):
    case = tc.exact_case((size,))
    ref, _ = case.reference(0)
    for variant in ("ieee", "fma"):
        np.testing.assert_array_equal(tc.oracle_scatter(case, 0, variant).astype(F64), ref)
        i = case.of(0)[:3000]
        val, _ = tc.ref_lookup(case.tex(0), case.u[i], case.v[i])
        np.testing.assert_array_equal(tc.oracle_lookup(case.tex(0), case.u[i], case.v[i], variant).astype(F64), val)


@pytest.mark.parametrize("family", tc.UV_FAMILIES)
def test_oracle_is_inside_the_bound_on_a_general_family(family):
    for size in [(4, 5), (37, 91)]:
        case = tc.general_case(family, (size,))
        i = case.of(0)[:3000]
        val, lb = tc.ref_lookup(case.tex(0), case.u[i], case.v[i])
        assert tc.scatter_ratio(case, 0, tc.oracle_scatter(case, 0, "ieee")) <= 1.0
        assert tc.ratio(np.abs(tc.oracle_lookup(case.tex(0), case.u[i], case.v[i], "ieee").astype(F64) - val), lb) <= 1.0


def test_map_reference_is_texel_centred_floor_and_clamp():
    """env_lookup's footprint by hand: u W - 0.5, floor (not trunc: x = -0.25 has base -1), clamp to edge; the adjoint is its transpose."""
    tex = np.arange(2 * 4 * 4, dtype=np.float32).reshape(2, 4, 4)
    u, v = np.array([0.5, 0.0625, 1.0, 0.3125], np.float32), np.array([0.5, 0.25, 2.0, 0.75], np.float32)
    val, _ = tc.ref_lookup(tex, u, v, env=True)
    np.testing.assert_array_equal(val[0], 0.5 * (0.5 * tex[0, 1] + 0.5 * tex[0, 2]) + 0.5 * (0.5 * tex[1, 1] + 0.5 * tex[1, 2]))
    np.testing.assert_array_equal(val[1], tex[0, 0])                          # x = -0.25: both corners clamp to texel 0
    np.testing.assert_array_equal(val[2], tex[1, 3])
    np.testing.assert_array_equal(val[3], 0.25 * tex[1, 0] + 0.75 * tex[1, 1])   # x = 0.75, y = 1: the lower corners carry no weight
    g = np.random.default_rng(0).integers(-8, 9, (4, 4)).astype(np.float32)
    grad, _ = tc.ref_scatter((2, 4), u, v, g, np.zeros((2, 4, 4), np.float32), env=True)
    assert float((grad * tex).sum()) == float((val * g).sum())


# ----------------------------------------------------------------------------- conditions, precondition
def test_input_conditions_hold_for_every_case():
    for c in exact_cases() + [c for _, c, _ in tc.all_general_cases()]:
        assert tc.input_conditions(c) is None, c.name
    # the exact family holds px = -1 and py = -1 themselves, and W - 1, W, 0
    c = tc.exact_case(((5, 5),))
    px, py = tc.footprint(c.u[c.of(0)], c.v[c.of(0)], (5, 5))[:2]
    for x in (-2.0, -1.0, -0.25, 0.0, 4.0, 5.0, 6.0):
        assert (px == x).any() and (py == x).any(), x
    # ... and the condition notices what it is there for
    bad = tc.general_case("uniform", ((5, 5),))
    u = bad.u.copy(); u[bad.of(0)[0]] = np.float32(-0.25)                     # px = -1
    moved = tc.Case("moved", bad.sizes, bad.active, u, bad.v, bad.g, bad.mat, bad.n, 0, False)
    assert "px = -1" in tc.input_conditions(moved)
    u[bad.of(0)[0]] = np.float32(2.0 ** 23)
    assert "2^24" in tc.input_conditions(tc.Case("far", bad.sizes, bad.active, u, bad.v, bad.g, bad.mat, bad.n, 0, False))


def test_exactness_precondition():
    """Largest sum of |term| (pre-fill included) below 2^20, every term a multiple of 2^-4: any float32 order gives the float64 sum."""
    for c in exact_cases():
        worst, dyadic = tc.exact_precondition(c)
        assert dyadic and worst < 2.0 ** 20, (c.name, worst, dyadic)
        r = c.rows()
        assert (r[:, 2:6] == np.rint(r[:, 2:6])).all() and np.abs(r[:, 2:6]).max() <= 8
        one_minus_v = np.float32(1) - c.v
        assert (one_minus_v.astype(F64) == 1.0 - c.v.astype(F64)).all()       # 1 - v is exact


def test_push_patterns_reach_every_branch_of_the_queue():
    a = tc.deal(16, np.random.default_rng(0))
    n = a.sum(2)
    assert (n[0] == 64).all() and (n[1] == 1).all() and (n[2] == [64, 0, 64, 0, 0, 64]).all()
    assert (n[3] == 40).all() and (n[4] == [63, 1, 63, 1, 63, 1]).all() and (n[5] == [64, 0, 0, 0, 0, 3]).all() and n[6].sum() == 0
    assert len({int(np.flatnonzero(a[1, r])[0]) for r in range(tc.ROUNDS)}) == tc.ROUNDS      # the one lane moves
    d = tc.queue_drops(a)
    assert d[3].sum(1).tolist() == [0, 16, 0, 16, 0, 16] and not d[[0, 1, 2, 4, 5, 6]].any()   # 40 + 40: the 65th to 80th entry
    c = tc.exact_case(((5, 5),))
    assert c.n % 64 == 37 and c.active.shape[0] == tc.WAVES                   # a partial last wave


# ----------------------------------------------------------------------------- the regimes, from the design text
def test_expected_regimes():
    def single(s):
        return tc.in_lds([s]), tc.expected_copies_single(s)
    assert tc.cells_of((3, 5)) == 24 and single((3, 5)) == (True, 1024)
    assert tc.cells_of((3, 6)) == 28 and single((3, 6)) == (True, 1024)       # the LDS limit itself
    assert tc.cells_of((4, 5)) == 30 and single((4, 5)) == (False, 1024)
    assert tc.cells_of((5, 5)) == 36 and single((5, 5)) == (False, 1024)
    assert single((17, 33)) == (False, 1024) and single((37, 91)) == (False, 299) and single((129, 129)) == (False, 62)
    assert tc.cells_of((254, 255)) == 65280 and single((254, 255)) == (False, 16)
    assert tc.cells_of((255, 255)) == 1 << 16 and single((255, 255)) == (False, 1)
    assert tc.cells_of((257, 257)) == 66564 and single((257, 257)) == (False, 1)
    assert tc.in_lds(tc.TABLES["lds"]) and tc.expected_copies_table(tc.TABLES["lds"]) == [1024] * 3      # 21 cells, copied as one array
    assert tc.expected_copies_table(tc.TABLES["copies"]) == [99, 1024, 1024]  # (2^20 / 3) / 3,496 cells
    assert tc.expected_copies_table(tc.TABLES["one_copy"]) == [1, 1024, 1024]
    assert tc.expected_copies_table(tc.TABLES["sixteen"])[:2] == [18, 7] and not tc.in_lds(tc.TABLES["sixteen"])
    assert tc.expected_copies_env(tc.ENV_SIZE) == 1024 and not tc.in_lds(tc.TABLES["lds"], env=True)


# ----------------------------------------------------------------------------- K
def test_k_is_the_measured_one():
    k, _, per_family, med = tc.measure_k(SMALL)
    assert k <= tc.K_MEASURED and tc.K == 4 * tc.K_MEASURED
    assert all(r > 0 for r in per_family["borders"].values())
    text = open(os.path.join(ROOT, "profiles", "texture_cases_margins.txt")).read()
    assert "K_MEASURED = %d " % tc.K_MEASURED in text
    medians = {}                                                              # a family whose bound is loose finds nothing
    for fam, case, _ in tc.all_general_cases():
        medians.setdefault(fam, []).append(tc.median_relative_bound(case))
    for fam, m in medians.items():
        assert np.median(m) <= 1e-4, (fam, np.median(m))


# ----------------------------------------------------------------------------- the judge bites
def restated(case, k, single, **kw):
    return tc.restate32(case, k, case.copies(single)[k], lds=tc.in_lds(case.sizes, case.env), **kw)


@pytest.mark.parametrize("fault", tc.FAULTS)
def test_exact_family_rejects_the_fault(fault):
    """(5, 5): copies, no LDS; (129, 129): 62 copies that wrap; (257, 257): one copy — the restatement is bit-equal without the fault
    and differs with it, wherever the fault can act at all (one copy has no stride; LDS has no queue)."""
    acted = 0
    for size in [(3, 5), (5, 5), (129, 129), (257, 257)]:
        case = tc.exact_case((size,))
        ref, _ = case.reference(0)
        assert np.array_equal(restated(case, 0, True).astype(F64), ref), size
        can_act = not (fault == "copy_stride" and case.copies(True)[0] == 1) and not (fault == "queue_drops_65th" and tc.in_lds([size]))
        differs = not np.array_equal(restated(case, 0, True, fault=fault).astype(F64), ref)
        assert differs == can_act, (fault, size)
        acted += differs
    assert acted >= 2


# the families that exercise the faulty line: the corner index acts on every row; the base clamp and floor need px < 0 (floor also a
# fraction: at px = -1e-45 the lookup is continuous and both give the same answer), the fold's last-column term a base cell at ix = W - 1,
# i.e. u >= 1 — `outside` has all of them, `borders` rows at u = 1 and beyond
REJECTS = {"corner_index": ("uniform", "borders", "outside"), "base_clamp_0": ("outside",), "fold_last_column": ("borders", "outside"),
           "floor_for_trunc": ("outside",)}


@pytest.mark.parametrize("fault", tc.FAULTS[:4])
def test_general_families_reject_the_fault_under_the_bound(fault):
    for family in REJECTS[fault]:
        case = tc.general_case(family, ((37, 91),))
        assert tc.scatter_ratio(case, 0, restated(case, 0, True)) <= 1.0
        assert tc.scatter_ratio(case, 0, restated(case, 0, True, fault=fault)) > 1.0, (fault, family)
