"""The NumPy reference of the gather plan (tests/gather_plan_ref.py) against the existing transposes, on the existing cases.  No GPU.

The float32 references of the three scatters (texel_project_ref.gather_adjoint_ref, texel_mip_ref.scatter_mip_ref,
texel_aniso_ref.scatter_aniso_ref with dtype float32) form every addend operation for operation as the kernels do, and so does
``plan_ref``: given the SAME float32 view the addends are the same bits, and the two results differ in the summation alone.  The float64
apply of the plan sums those addends exactly (to 2^-53), the float32 references round each product once and each partial sum once, so
per row  |apply64 - ref32| <= (R + 1) 2^-24 sum |weight d_color|  with R the row's length (the standard bound of recursive summation,
first order).  That bound is what "equal to rounding" means here; it is asserted with a factor 1.01 for the second-order terms."""
import numpy as np
import pytest

import gather_plan_ref as GR
import texel_aniso_cases as AC
import texel_aniso_ref as AR
import texel_mip_ref as MR
import texel_project_cases as PC
import texel_project_ref as PR

F = np.float32
EPS = 2.0 ** -24
PROJECT_CASES = ["cbox_16x16_standard", "cbox_64x64_standard", "cbox_64x64_inside", "cbox_64x64_inside_1x1"]
ANISO_CASES = ["cbox_16x16_standard", "cbox_64x64_inside"]


def view32(name):
    return PC.reference(name)["data"].astype(F)


def cotangent(shape, seed=3):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def summation_bound(plan, g):
    absplan = dict(plan, weight=np.abs(plan["weight"]))
    return 1.01 * (GR.counts(plan) + 1)[:, None] * EPS * GR.apply_ref(absplan, np.abs(g), np.float64)


def packed_rows(d_image, G, res, levels=0):
    """the rows of a plan from the (d_image, [None, G_1 ..]) of the scatter references"""
    rows = [np.asarray(d_image).reshape(-1, 4)]
    if len(G) > 1:
        rows += [g.reshape(-1, 4) for g in G[1:]]
    else:
        rows.append(np.zeros((1, 4), rows[0].dtype))
    return np.concatenate(rows, 0)


@pytest.mark.parametrize("name", PROJECT_CASES)
def test_bilinear_plan_is_the_transpose_reference_and_has_four_entries_per_visible_texel(name):
    view, res = view32(name), PC.CASES[name][2]
    plan = GR.plan_ref(view, None, res, "bilinear")
    on = (view[..., 0] != 0) & ~np.isnan(view[..., 0])
    assert plan["nnz"] == 4 * int(on.sum()) and plan["rows"] == res[0] * res[1] and plan["row_start"][-1] == plan["nnz"]
    assert (np.diff(plan["id_texel"]) >= 0).all() and (np.diff(plan["row"]) >= 0).all()
    g = cotangent(view.shape[:2] + (4,))
    got, want = GR.apply_ref(plan, g, np.float64), PR.gather_adjoint_ref(g, view, res, F).reshape(-1, 4)
    err, bound = np.abs(got - want), summation_bound(plan, g)
    print(f"[gather plan host] {name} bilinear: nnz {plan['nnz']}, longest row {GR.counts(plan).max()}, largest error {err.max():.3e}")
    assert (err <= bound).all() and np.abs(want).max() > 0


@pytest.mark.parametrize("footprint", [1.0, 3.0])
@pytest.mark.parametrize("name", PROJECT_CASES)
def test_mip_plan_is_the_transpose_reference_and_counts_the_upper_taps(name, footprint):
    view, res = view32(name), PC.CASES[name][2]
    plan = GR.plan_ref(view, None, res, "mip", footprint)
    v = view.reshape(-1, 8)
    on = (v[:, 0] != 0) & ~np.isnan(v[:, 0])
    L = len(MR.layout(res)) - 1
    _, fr = MR.level_split(v[:, 6], footprint, L, F)
    upper = int((on & (fr != 0)).sum())
    assert plan["nnz"] == 4 * int(on.sum()) + 4 * upper and 4 * int(on.sum()) <= plan["nnz"] <= 8 * int(on.sum())
    assert plan["rows"] == GR.rows_of(res, "mip")[1]
    g = cotangent(view.shape[:2] + (4,))
    d_image, G = MR.scatter_mip_ref(g, view, res, footprint, 0, F)
    got, want = GR.apply_ref(plan, g, np.float64), packed_rows(d_image, G, res)
    err, bound = np.abs(got - want), summation_bound(plan, g)
    print(f"[gather plan host] {name} mip x{footprint}: nnz {plan['nnz']} ({upper} texels with an upper level), largest error {err.max():.3e}")
    assert got.shape == want.shape and (err <= bound).all() and np.abs(want).max() > 0


@pytest.mark.parametrize("max_aniso", [8, 2])
@pytest.mark.parametrize("name", ANISO_CASES)
def test_aniso_plan_is_the_transpose_reference(name, max_aniso):
    view, fp, res = AC.view_reference(name)["data"].astype(F), AC.footprint_reference(name).astype(F), AC.CASES[name][2]
    plan = GR.plan_ref(view, fp, res, "aniso", 1.0, max_aniso)
    g = cotangent(view.shape[:2] + (4,))
    d_image, G = AR.scatter_aniso_ref(g, view, fp, res, 1.0, max_aniso, 0, F)
    got, want = GR.apply_ref(plan, g, np.float64), packed_rows(d_image, G, res)
    err, bound = np.abs(got - want), summation_bound(plan, g)
    N = AR.probes(fp[view[..., 0] == 1], 1.0, max_aniso, F)[0]
    print(f"[gather plan host] {name} aniso x{max_aniso}: nnz {plan['nnz']}, probes up to {N.max()}, largest error {err.max():.3e}")
    assert 1 < N.max() <= max_aniso and 4 * N.sum() <= plan["nnz"] <= 8 * N.sum()
    assert got.shape == want.shape and (err <= bound).all() and np.abs(want).max() > 0


def test_the_plan_is_the_transpose_of_the_forward_references():
    """<K x, y> = <x, K^T y> in float64.  K is the forward reference in float64 on the float32 view; K^T is the plan, whose weights were
    formed in float32.  Bilinear and mip: the taps sit where the float64 reference's do (X - 0.5 and X 2^-l are exact), and a weight is
    at most eight float32 roundings off (1 - tx, 1 - ty, their product, the level fraction and 1 - f, the share, 1 / N, visible), each
    2^-24 relative: the two sides agree to 8 x 2^-24 = 4.8e-7 of sum |y| K|x|.  Aniso adds the rounding of the probe's position,
    X + (t footprint) major_x, to float32: half an ulp of a position below 128 pixels is 2^-18 = 3.8e-6 pixels in X and in Y, and a
    bilinear weight moves by as much, absolutely — hence 1e-5 there (texels within NEAR of a switch of N or of a clamp are left out
    of y).  The figures printed are far below both: the roundings do not add up in one direction."""
    rng = np.random.default_rng(5)
    name, res = "cbox_16x16_standard", AC.CASES["cbox_16x16_standard"][2]
    view, fp = AC.view_reference(name)["data"].astype(F), AC.footprint_reference(name).astype(F)
    x = rng.random((res[1], res[0], 4))
    y = rng.standard_normal(view.shape[:2] + (4,))
    y[AR.exempt(fp, 1.0, 8)] = 0.0
    for filter, forward in (("bilinear", lambda im: PR.gather_ref(im, view)), ("mip", lambda im: MR.gather_mip_ref(im, view, 3.0)),
                            ("aniso", lambda im: AR.gather_aniso_ref(im, view, fp, 1.0, 8))):
        plan = GR.plan_ref(view, fp, res, filter, 3.0 if filter == "mip" else 1.0, 8)
        rows = GR.apply_ref(plan, y, np.float64)
        d_image = rows[:plan["p0"]].reshape(res[1], res[0], 4)
        if filter != "bilinear":
            d_image = d_image + MR.pyramid_adjoint_ref(rows[plan["p0"]:], res)
        lhs, rhs = float((forward(x) * y).sum()), float((x * d_image).sum())
        scale = float((forward(np.abs(x)) * np.abs(y)).sum())
        print(f"[gather plan host] transpose {filter}: <Kx, y> {lhs:.9e}, <x, K^T y> {rhs:.9e}, relative to sum |y| K|x| {abs(lhs - rhs) / scale:.2e}")
        assert abs(lhs - rhs) <= (1e-5 if filter == "aniso" else 8 * EPS) * scale and scale > 0


@pytest.mark.parametrize("R", [0, 1, 15, 16, 17, 33, 1000])
def test_the_sixteen_way_order_against_a_literal_loop(R):
    p = np.random.default_rng(R).standard_normal((R, 4)).astype(F) * F(1e3)
    want = np.zeros(4, F)
    for c in range(4):
        s = [F(0.0)] * 16
        for j in range(16):
            for k in range(j, R, 16):
                s[j] = F(s[j] + p[k, c])
        for half in (8, 4, 2):
            for j in range(half):
                s[j] = F(s[j] + s[j + half])
        want[c] = F(s[0] + s[1])
    assert GR.sum16(p).view(np.uint32).tolist() == want.view(np.uint32).tolist()
    plan = {"rows": 3, "row": np.full(R, 1), "texel": np.arange(R), "weight": np.ones(R, F), "row_start": np.array([0, 0, R, R])}
    got = GR.apply_ref(plan, p)
    assert got[1].view(np.uint32).tolist() == want.view(np.uint32).tolist() and not got[0].any() and not got[2].any()
    if R > 16:                                                       # the order matters: a plain running sum gives other bits somewhere
        assert any(GR.sum16(np.random.default_rng(s).standard_normal((R, 1)).astype(F))[0] !=
                   np.cumsum(np.random.default_rng(s).standard_normal((R, 1)).astype(F), dtype=F)[-1] for s in range(8))
