"""The NumPy reference of the UV tangents (tests/texel_tangent_ref.py) and its cases (tests/texel_tangent_cases.py) pinned on the host:
the measured constants, the tangents as finite differences of the positions, the area against texel_size^2 and the zero rows, the
orientation, the footprint from tangents tied to the pinned square-patch reference, and the quality table against the supersampled
true patch.  No GPU."""
import numpy as np
import pytest

import texel_aniso_cases as AC
import texel_aniso_ref as AR
import texel_cases as TC
import texel_lighting_cases as LC
import texel_project_ref as PR
import texel_tangent_cases as TT
import texel_tangent_ref as TR

# quality table, float64 reference: (case, image) -> RMSE of bilinear, mip 1, mip 0.5, aniso square, aniso uv (rounded to 4 digits)
QUALITY = {
    ("cbox_16x64", "noise"): (0.1740, 0.0705, 0.0665, 0.0633, 0.0483),
    ("cbox_16x64", "blocks"): (0.1757, 0.0973, 0.0834, 0.0760, 0.0348),
    ("cbox_64x16", "noise"): (0.1823, 0.0777, 0.0833, 0.0670, 0.0491),
    ("cbox_64x16", "blocks"): (0.2097, 0.0955, 0.1114, 0.0845, 0.0301),
}


@pytest.mark.parametrize("name", list(TT.CASES))
def test_the_measured_margins_hold(name):
    e = TT.errors(name, TT.reference(name, "float32")["data"])
    r32 = TT.reference(name, "float32")
    e = e + (TT.area_relative_error(r32["data"], r32["aovs"]["data"]),)
    for x, m in zip(e, TT.MARGINS[name]):
        assert x <= m and (m == 0 or x >= 0.5 * m), (name, e, TT.MARGINS[name])


@pytest.mark.parametrize("name", list(TT.FOOTPRINT_CASES))
def test_the_measured_footprint_margins_hold(name):
    vis = TT.visible(name)
    ref = TT.footprint_reference(name)
    err = TT.footprint_errors(TT.footprint_reference(name, "float32"), ref)[vis].max(0)
    for x, m in zip(err, TT.FOOTPRINT_MARGINS[name]):
        assert x <= m and (m == 0 or x >= 0.5 * m), (name, err, TT.FOOTPRINT_MARGINS[name])
    assert not TT.footprint_failing(name, TT.footprint_reference(name, "float32"), ref).any()


@pytest.mark.parametrize("name", ["cbox_5x7", "panel_3x2", "soup_130", "cbox_16x64", "cbox_64x16", "panel_mirrored"])
def test_a_tangent_is_the_difference_of_two_neighbours_positions(name):
    """float32 positions against float64 tangents, where two neighbours have the same coverage winner"""
    tan = TT.reference(name)["data"]
    a32 = TT.reference(name, "float32")["aovs"]
    pos, g = a32["data"][..., 8:11].astype(np.float64), a32["cov_g"]
    make = TT.CASES[name][0]
    extent = float(np.abs(TC.R.world_triangles(make(), np.float64)[0]).max())
    # the position bar of texel_cases: the case's own where it has one, else by its rule with the largest margin measured there
    pos_bar = TC.bars(name)[0] if name in TC.CASES else max(4.0 * max(m[0] for m in TC.MARGINS.values()), TC.FLOOR_ULPS * TC.EPS32 * extent)
    bar = 2.0 * pos_bar + TT.bars(name)[0]
    keep = TT.compared(name)
    same_x = (g[:, 1:] == g[:, :-1]) & (g[:, 1:] != TC.R.EMPTY) & keep[:, 1:] & keep[:, :-1]
    same_y = (g[1:, :] == g[:-1, :]) & (g[1:, :] != TC.R.EMPTY) & keep[1:, :] & keep[:-1, :]
    assert same_x.sum() > 0 and (same_y.sum() > 0 or name == "cbox_5x7"), name      # (5 rows: no two covered rows of one triangle)
    dx = np.abs((pos[:, 1:] - pos[:, :-1]) - tan[:, :-1, 0:3])[same_x]
    dy = np.abs((pos[1:, :] - pos[:-1, :]) - tan[:-1, :, 4:7])[same_y]
    ex, ey = float(dx.max()), float(dy.max()) if dy.size else 0.0
    print(f"[tangent finite differences] {name}: along x {ex:.3e} ({int(same_x.sum())} pairs), along y {ey:.3e} ({int(same_y.sum())} pairs), bar {bar:.3e}")
    assert ex <= bar and ey <= bar, (name, ex, ey, bar)


@pytest.mark.parametrize("name", list(TT.CASES))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_area_is_texel_size_squared_and_rows_are_zero_where_texel_size_is(name, dtype):
    ref = TT.reference(name, dtype)
    tan, aovs = ref["data"], ref["aovs"]["data"]
    reached = aovs[..., 12] == 1
    assert TT.area_relative_error(tan, aovs) <= TT.area_bar(name), name
    assert np.array_equal(TR.zero_rows(tan)[reached], (aovs[..., 7] == 0)[reached]), name
    assert TR.zero_rows(tan)[~reached].all(), name
    if name in ("cbox_1x1", "cbox_no_instance"):
        assert TR.zero_rows(tan).all(), name


@pytest.mark.parametrize("name", list(TT.ORIENTATION))
def test_the_orientation_is_the_charts(name):
    ref = TT.reference(name)
    reached = ref["aovs"]["data"][..., 12] == 1
    assert reached.any() and (ref["data"][..., 7][reached] == TT.ORIENTATION[name]).all(), name
    assert TT.ORIENTATION["panel_mirrored"] == -TT.ORIENTATION["panel_3x2"]


@pytest.mark.parametrize("name", list(AC.CASES))
def test_the_square_patchs_tangents_give_the_square_patchs_footprint(name):
    """Tx = texel_size t1, Ty = texel_size t2 of make_onb: the pinned reference of zdr_texel_footprint, to 1e-12 relative"""
    pts = AC.points(name)
    H, W = pts.shape[:2]
    t1, t2 = AR.make_onb(pts[..., 4:7].reshape(-1, 3).astype(np.float64), np.float64)
    ts = pts[..., 7].reshape(-1, 1).astype(np.float64)
    tan = np.zeros((H * W, 8))
    tan[:, 0:3], tan[:, 4:7], tan[:, 3], tan[:, 7] = ts * t1, ts * t2, ts[:, 0] ** 2, 1.0
    tan[~np.isfinite(tan).all(-1) | (ts[:, 0] == 0)] = 0
    got = TR.footprint_tangents_ref(pts, tan.reshape(H, W, 8), AC.camera(name), AC.CASES[name][2])
    ref = AC.footprint_reference(name)
    keep = PR.shaded(pts) & (pts[..., 7] != 0)
    assert keep.sum() > 0
    scale = np.abs(ref[keep]).max()
    assert np.abs(got[keep][:, 2:] - ref[keep][:, 2:]).max() <= 1e-12 * scale, name
    round_ = ref[..., 3] < AC.MIN_RATIO * ref[..., 2]               # (the direction of a near-circle selects nothing)
    sel = keep & ~round_
    assert np.abs(np.abs(got[sel][:, 0] * ref[sel][:, 0] + got[sel][:, 1] * ref[sel][:, 1]) - ref[sel][:, 3] ** 2).max() <= 1e-12 * scale ** 2, name


@pytest.mark.parametrize("name", TT.SANITY_CASES)
def test_on_an_isotropic_chart_the_uv_footprint_is_the_square_patchs(name):
    case = AC.CASES[name][0]
    make, slots, hw = LC.CASES[case][:3]
    tan = TR.tangents_ref(make(), slots, 0, hw, np.float64)["data"]
    vis = AC.visible(name)
    sq = AC.footprint_reference(name)[vis]
    uv = TR.footprint_tangents_ref(AC.points(name), tan, AC.camera(name), AC.CASES[name][2])[vis]
    d_major, d_minor = np.abs(uv[:, 3] - sq[:, 3]) / sq[:, 3], np.abs(uv[:, 2] - sq[:, 2]) / sq[:, 3]
    print(f"[uv footprint sanity] {name}: major {d_major.max():.3e}, minor {d_minor.max():.3e}")
    assert d_major.max() <= 1e-2 and d_minor.max() <= 1e-2, (name, d_major.max(), d_minor.max())


@pytest.mark.parametrize("name", TT.QUALITY_CASES)
def test_the_uv_footprint_is_the_best_of_the_five_on_a_non_square_texture(name):
    case, cam, res = TT.FOOTPRINT_CASES[name]
    v64 = TT.view_reference(name)["data"]
    fp_sq = AR.footprint_ref(TT.points(case), cam, res)
    fp_uv = TT.footprint_reference(name, tangents=TT.reference(case)["data"])
    for label, image in AC.images().items():
        row = {k: TT.rmse(name, c, TT.truths(name)[label]) for k, c in TT.quality_row(name, image, v64, fp_sq, fp_uv).items()}
        print(f"[uv quality, float64] {name} {label}: " + "  ".join(f"{k} {v:.4f}" for k, v in row.items()))
        assert all(row["aniso uv"] < v for k, v in row.items() if k != "aniso uv"), (name, label, row)
        assert tuple(round(v, 4) for v in row.values()) == QUALITY[(name, label)], (name, label, row)


@pytest.mark.parametrize("name", list(TT.CASES))
def test_at_most_one_percent_of_a_cases_texels_are_uncertain(name):
    unc = TT.reference(name)["aovs"]["uncertain"]
    assert unc.sum() <= TT.MAX_UNCERTAIN * unc.size, name
    assert int(unc.sum()) == (2 if name == "soup_130" else 0), name


@pytest.mark.parametrize("name,visible", [("cbox_16x64", 458), ("cbox_64x16", 465)])
def test_at_most_one_percent_of_the_visible_texels_are_exempt(name, visible):
    vis = TT.visible(name)
    assert int(vis.sum()) == visible
    ex = AR.exempt(TT.footprint_reference(name), 1.0, 8) & vis
    assert ex.sum() <= TT.MAX_EXEMPT * vis.sum() and int(ex.sum()) == 0, (name, int(ex.sum()))
