"""The NumPy reference of the anisotropic gather (tests/texel_aniso_ref.py) and its cases (tests/texel_aniso_cases.py) pinned on the
host: the measured constants, the ellipse's independence of the tangent basis, the on-axis texel, the properties include/zdr.h states
for the gather in float32 bit for bit, the adjoint as the exact transpose in float64, and the quality condition against the
supersampled patch.  No GPU."""
import numpy as np
import pytest

import texel_aniso_cases as AC
import texel_aniso_ref as AR
import texel_mip_ref as MR
import texel_project_ref as PR
from test_texel_mip_ref_host import bits, synthetic

SIZES = [(96, 64), (33, 17), (7, 5), (1, 1)]           # (width, height)


def synthetic_footprint(rng, n, major=(0.3, 30.0), ratio=(1.0, 20.0)):
    """footprint rows (n, 1, 4): a major axis of log-uniform length in any direction, minor = major / a log-uniform ratio"""
    fp = np.zeros((n, 1, 4), np.float32)
    m = np.exp(rng.uniform(np.log(major[0]), np.log(major[1]), n))
    phi = rng.uniform(0, 2 * np.pi, n)
    fp[:, 0, 0] = m * np.cos(phi); fp[:, 0, 1] = m * np.sin(phi)
    fp[:, 0, 3] = np.sqrt(fp[:, 0, 0].astype(np.float64) ** 2 + fp[:, 0, 1].astype(np.float64) ** 2)
    fp[:, 0, 2] = fp[:, 0, 3] / np.exp(rng.uniform(np.log(ratio[0]), np.log(ratio[1]), n))
    return fp


@pytest.mark.parametrize("name", list(AC.CASES))
def test_the_measured_constants_hold(name):
    assert AC.probe_counts(name) == AC.PROBE_COUNTS[name]
    vis = AC.visible(name)
    err = AC.footprint_errors(name, AC.footprint_reference(name, "float32"))[vis].max(0)
    for e, m in zip(err, AC.MARGINS[name]):
        assert e <= m and (m == 0 or e >= 0.5 * m), (name, err, AC.MARGINS[name])
    assert not AC.footprint_failing(name, AC.footprint_reference(name, "float32")).any()
    ref = AC.footprint_reference(name)
    for footprint in (1.0, 0.5):
        for max_aniso in (8, 2):
            assert int((AR.exempt(ref, footprint, max_aniso) & vis).sum()) <= AC.MAX_EXEMPT_REF * vis.sum()
    shaded = PR.shaded(AC.points(name))
    front = AC.view_reference(name)["front"]
    assert (ref[~shaded] == 0).all() and (ref[shaded & ~front] == 0).all() and (ref[vis][:, 3] >= ref[vis][:, 2]).all() and (ref[vis][:, 2] > 0).all()


def test_the_cases_have_the_classes_the_issue_names():
    assert AC.PROBE_COUNTS["cbox_64x64_standard"] == (1815, [453, 0, 1106, 245, 11, 0, 0, 0])
    assert AC.PROBE_COUNTS["cbox_16x16_standard"][1][7] > 0                       # reaches N = 8
    ref = AC.view_reference("cbox_64x64_inside")
    reached = AC.points("cbox_64x64_inside")[..., 12] == 1
    assert int((reached & ~ref["front"]).sum()) > 100 and int((reached & ref["front"] & ~ref["inside"]).sum()) > 100
    assert all(c > 0 for c in AC.PROBE_COUNTS["cbox_64x64_inside"][1][1:7])       # N from 2 to 7


@pytest.mark.parametrize("name", ["cbox_64x64_standard", "cbox_64x64_inside"])
def test_the_footprint_does_not_depend_on_the_tangent_basis(name):
    ref = AC.footprint_reference(name)
    vis = AC.visible(name)
    for angle in (0.3, 1.0, 2.5):
        rot = AR.footprint_ref(AC.points(name), AC.camera(name), AC.RES, np.float64, rotate=angle)
        assert np.abs(rot[..., 2:] - ref[..., 2:])[vis].max() <= 1e-12 * ref[vis][:, 3].max()
        e = np.abs((rot[..., 0] * ref[..., 0] + rot[..., 1] * ref[..., 1])[vis]) / (ref[vis][:, 3] ** 2)
        keep = ref[vis][:, 3] >= AC.MIN_RATIO * ref[vis][:, 2]
        assert np.abs(1 - e[keep]).max() <= 1e-12


def test_on_the_optical_axis_facing_the_camera_both_axes_are_the_views_scale():
    cam = (0.8, (0.5, 1.0, 2.0), (0.1, 0.4, -3.0), (0.0, 1.0, 0.0))
    res = (96, 64)
    o, fwd, *_ = PR.camera_frame(cam, res)
    pts = np.zeros((1, 3, 16), np.float32)
    for i, depth in enumerate((0.5, 2.0, 7.0)):
        pts[0, i, 8:11] = o + np.float32(depth) * fwd
        pts[0, i, 4:7] = -fwd; pts[0, i, 7] = 0.01 * (i + 1); pts[0, i, 12] = 1
    frame = PR.camera_frame(cam, res)
    z, *_ = PR.project(pts[0, :, 8:11].astype(np.float64), frame, res, np.float64)
    scale = pts[0, :, 7].astype(np.float64) * (0.5 * res[0]) / (float(frame[4]) * z)
    for dtype, tol in ((np.float64, 1e-6), (np.float32, 1e-5)):                   # (the frame itself is float32: fwd is a unit vector to 1e-7)
        fp = AR.footprint_ref(pts, cam, res, dtype)[0].astype(np.float64)
        assert np.abs(fp[:, 3] / scale - 1).max() <= tol and np.abs(fp[:, 2] / scale - 1).max() <= tol, (dtype, fp, scale)


def test_the_probe_rule():
    fp = np.zeros((9, 4), np.float32)
    fp[:, 3] = [0.5, 1.0, 4.0, 4.0, 4.0, 64.0, np.nan, 4.0, 9.0]
    fp[:, 2] = [0.1, 1.0, 4.0, 2.0, 0.1, 1.0, 1.0, np.nan, 8.0]
    N, s = AR.probes(fp, 1.0, 8, np.float32)
    assert N.tolist() == [1, 1, 1, 2, 4, 8, 1, 4, 1]
    assert s.tolist() == [1.0, 1.0, 4.0, 2.0, 1.0, 8.0, 1.0, 1.0, 8.0] and s.dtype == np.float32
    assert AR.probes(fp, 1.0, 1, np.float32)[0].tolist() == [1] * 9
    assert AR.probes(fp[2:5], 1.0, 2)[0].tolist() == [1, 2, 2] and AR.probes(fp[4:5], 1.0, 2)[1].tolist() == [2.0]      # the A / max_aniso clamp
    assert AR.probes(fp[2:3], 0.5, 8)[1].tolist() == [2.0]
    # a ratio of exactly 1 (a plane parallel to the image plane) and one a few ulps above it both give one probe: the offset of 1/8
    fp[:2, 3] = [5.0, np.nextafter(np.float32(5.0), np.float32(6.0))]; fp[:2, 2] = 5.0
    assert AR.probes(fp[:2], 1.0, 8, np.float32)[0].tolist() == [1, 1]
    ex = AR.exempt(np.array([[0, 0, 2.0, 6.25], [0, 0, 1.5, 3.2], [0, 0, 0.2, 1.00001], [0, 0, 1.00001, 3.3], [0, 0, 0.5, 4.00001], [0, 0, 0.3, 0.7]]), 1.0, 8)
    assert ex.tolist() == [True, False, True, True, True, False]


@pytest.mark.parametrize("res", SIZES)
def test_the_exact_families_in_float32_bit_for_bit(res):
    rng = np.random.default_rng(31)
    image = rng.normal(size=(res[1], res[0], 4)).astype(np.float32)
    view = synthetic(rng, 300, res)
    iso = np.zeros((300, 1, 4), np.float32)
    iso[:, 0, 0] = iso[:, 0, 2] = iso[:, 0, 3] = view[:, 0, 6]
    for footprint in (1.0, 3.0, 0.5):                                             # major_axis = (scale, 0), minor = major = scale: the mip gather
        assert np.array_equal(bits(AR.gather_aniso_ref(image, view, iso, footprint, 8, 0, np.float32)), bits(MR.gather_mip_ref(image, view, footprint, 0, np.float32)))
    fp = synthetic_footprint(rng, 300)
    fp[:, 0, 3] = view[:, 0, 6]; fp[:, 0, 2] = view[:, 0, 6] * rng.uniform(0.05, 1.0, 300).astype(np.float32)
    assert np.array_equal(bits(AR.gather_aniso_ref(image, view, fp, 1.0, 1, 0, np.float32)), bits(MR.gather_mip_ref(image, view, 1.0, 0, np.float32)))   # max_aniso = 1
    fp = synthetic_footprint(rng, 300, major=(0.01, 1.0))                         # major footprint <= 1: the bilinear gather
    assert np.array_equal(bits(AR.gather_aniso_ref(image, view, fp, 1.0, 8, 0, np.float32)), bits(PR.gather_ref(image, view, np.float32)))
    fp = synthetic_footprint(rng, 300)
    const = np.full((res[1], res[0], 4), np.float32(0.3), np.float32)
    got = AR.gather_aniso_ref(const, view, fp, 1.0, 8, 0, np.float32)       # visible is 0 or 1 here: visible x the constant within 2 ulps
    ulp = float(np.spacing(np.float32(0.3)))
    assert np.abs(got.astype(np.float64) - view[..., 0:1].astype(np.float64) * np.float64(np.float32(0.3))).max() <= 2 * ulp


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("footprint,max_aniso", [(1.0, 8), (0.5, 8), (1.0, 2), (2.0, 16)])
def test_the_adjoint_is_the_exact_transpose_in_float64(res, footprint, max_aniso):
    rng = np.random.default_rng(32)
    view, fp = synthetic(rng, 300, res), synthetic_footprint(rng, 300)
    view[:, 0, 0] *= rng.uniform(0.2, 1.0, 300).astype(np.float32)
    N, _ = AR.probes(fp, footprint, max_aniso)
    assert N.max() == max_aniso and N.min() == 1
    x, y = rng.normal(size=(res[1], res[0], 4)), rng.normal(size=(300, 1, 4))
    lhs = float((AR.gather_aniso_ref(x, view, fp, footprint, max_aniso) * y).sum())
    rhs = float((x * AR.gather_aniso_adjoint_ref(y, view, fp, res, footprint, max_aniso)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    d_image, G = AR.scatter_aniso_ref(y, view, fp, res, footprint, max_aniso, 2)
    assert len(G) == len(MR.layout(res, 2)) and d_image.shape == (res[1], res[0], 4)


@pytest.mark.parametrize("name", ["cbox_16x16_standard", "cbox_64x64_standard"])
def test_the_quality_condition_on_the_float64_reference(name):
    """against the mean of the image over the texel's own patch the anisotropic gather at the default footprint beats the bilinear
    gather and both footprints of the mip gather, on both images"""
    view, fp = AC.view_reference(name)["data"], AC.footprint_reference(name)
    for label, image in AC.images().items():
        truth = AR.truth_ref(image, AC.points(name), AC.camera(name), AC.RES)
        aniso = AC.rmse(name, AR.gather_aniso_ref(image, view, fp, 1.0, 8), truth)
        others = {"bilinear": AC.rmse(name, PR.gather_ref(image, view), truth), "mip 1": AC.rmse(name, MR.gather_mip_ref(image, view, 1.0), truth),
                  "mip 0.5": AC.rmse(name, MR.gather_mip_ref(image, view, 0.5), truth)}
        print(f"[texel aniso quality, float64 reference] {name} {label}: aniso {aniso:.4f}  " + "  ".join(f"{k} {v:.4f}" for k, v in others.items())
              + f"  (aniso / best other {aniso / min(others.values()):.2f})")
        for k, v in others.items():
            assert aniso < v, (name, label, k, aniso, v)
