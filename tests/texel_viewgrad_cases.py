"""The cases of the camera gradients that are compared with the float64 references (tests/texel_viewgrad_ref.py), shared by the host
test (tests/test_texel_viewgrad_ref_host.py) and the GPU tests (tests/test_gpu_texel_viewgrad.py), and their bars.

A case is a case of tests/texel_project_cases.py — sample points, a camera (standard, inside), an image size (24 x 16, 1 x 1) — with
three images of that size (smooth, noise, ramp), a random colour cotangent and, for the camera sums, a random view cotangent.  Filters:
bilinear, mip with footprint 1 and mip with footprint 4.

Bars, by the convention of tests/texel_project_cases.py (``linear_bar``: the rule applied to the very inputs the kernel is given).
d_view: per channel (d_X, d_Y, d_scale) 4 x the float32 reference's largest error against the float64 one over the certain texels,
floor FLOOR_ULPS float32 ulps of the channel's largest value.  The 10 camera sums cancel, so their floor is FLOOR_ULPS ulps of the sum
over the texels of |the texel's term| instead.  A texel is UNCERTAIN where the float64 fx or fy of a sampled level lies within
``PR.JIGGLE`` of an integer, where s lies within 1e-4 relative of a power of two, or where ``visible`` is uncertain in ``PC.reference``;
uncertain plus failing texels may be MAX_UNCERTAIN of the reached ones, and the float32 reference alone stays below MAX_UNCERTAIN_REF.

``python tests/texel_viewgrad_cases.py`` prints profiles/texel_viewgrad_margins.txt (no GPU involved) on the float32 reference's view
buffers, and the MARGINS table below, which the host test holds the references to."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import texel_project_cases as PC                                 # noqa: E402
import texel_project_ref as PR                                   # noqa: E402
import texel_viewgrad_ref as VR                                  # noqa: E402

MAX_UNCERTAIN = PC.MAX_UNCERTAIN
MAX_UNCERTAIN_REF = PC.MAX_UNCERTAIN_REF
FLOOR_ULPS = PC.FLOOR_ULPS
EPS32 = PC.EPS32
CASES = tuple(PC.CASES)
IMAGES = ("smooth", "noise", "ramp")
FILTERS = (("bilinear", 1.0), ("mip", 1.0), ("mip", 4.0))          # (filter, footprint)
DVIEW_CHANNELS = (2, 3, 6)                                         # d_X, d_Y, d_scale
# image sizes that differ from the case's own in tests/texel_project_cases.py: at 24 x 16 the 16 x 16 texture has a texel on a tap
# boundary (1 of 208 reached texels uncertain, above MAX_UNCERTAIN_REF); one column fewer and it has none
RES = {"cbox_16x16_standard": (23, 16)}
RAMP = (0.25, -0.125, 0.5)                                        # alpha x + beta y + gamma, channel c scaled by c + 1

# largest |float32 reference - float64 reference| of (d_X, d_Y, d_scale) over the certain texels and all images, per filter, on the
# float32 reference's view buffer; then of the 10 camera sums relative to their floor's sum of |terms|
# (python tests/texel_viewgrad_cases.py; profiles/texel_viewgrad_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_16x16_standard/bilinear/1": (5.08e-07, 1.45e-06, 0.00e+00),
    "cbox_16x16_standard/mip/1": (2.31e-07, 6.68e-07, 8.80e-07),
    "cbox_16x16_standard/mip/4": (2.56e-07, 2.07e-07, 1.96e-06),
    "cbox_64x64_standard/bilinear/1": (1.10e-06, 1.02e-06, 0.00e+00),
    "cbox_64x64_standard/mip/1": (1.10e-06, 1.02e-06, 2.44e-06),
    "cbox_64x64_standard/mip/4": (3.28e-07, 5.07e-07, 3.92e-06),
    "multi_24_standard/bilinear/1": (9.33e-07, 1.81e-06, 0.00e+00),
    "multi_24_standard/mip/1": (3.01e-07, 1.09e-06, 1.50e-06),
    "multi_24_standard/mip/4": (2.69e-07, 3.73e-07, 2.40e-06),
    "cbox_16x16_inside/bilinear/1": (3.30e-07, 5.93e-07, 0.00e+00),
    "cbox_16x16_inside/mip/1": (5.97e-08, 4.41e-08, 4.25e-08),
    "cbox_16x16_inside/mip/4": (2.14e-08, 0.00e+00, 9.48e-08),
    "cbox_64x64_inside/bilinear/1": (9.67e-07, 8.11e-07, 0.00e+00),
    "cbox_64x64_inside/mip/1": (5.17e-07, 2.52e-07, 1.07e-06),
    "cbox_64x64_inside/mip/4": (2.44e-07, 1.05e-07, 1.12e-06),
    "cbox_64x64_inside_1x1/bilinear/1": (0.00e+00, 0.00e+00, 0.00e+00),
    "cbox_64x64_inside_1x1/mip/1": (0.00e+00, 0.00e+00, 0.00e+00),
    "cbox_64x64_inside_1x1/mip/4": (0.00e+00, 0.00e+00, 0.00e+00),
}
# A record, not a bar (the float32 autograd's order of addition is the host library's): in float32 ulps of the sum of |terms|.  The
# inside camera stands in the box: texels close to its plane z = 0 have X, Y and scale ~ 1 / z with z itself a cancelled float32 sum,
# so there float32 alone costs hundreds of ulps, and up.y — whose terms cancel to nothing — thousands
CAMERA_MARGINS = {
    "cbox_16x16_standard": (2.89e-02, 8.55e-01, 1.30e+00, 1.90e-01, 1.19e-01, 4.42e-02, 0.00e+00, 3.05e-01, 0.00e+00, 0.00e+00),
    "cbox_64x64_standard": (3.32e-02, 2.31e-01, 3.19e-01, 1.10e-02, 3.90e-02, 4.40e-02, 0.00e+00, 2.51e-02, 0.00e+00, 0.00e+00),
    "multi_24_standard": (3.12e-01, 3.23e-01, 7.74e-01, 2.19e-01, 1.25e-01, 3.06e-01, 0.00e+00, 9.66e-02, 0.00e+00, 0.00e+00),
    "cbox_16x16_inside": (7.94e+00, 2.70e+01, 3.54e+01, 3.13e+01, 3.43e+01, 8.11e+00, 3.00e+01, 4.24e+00, 8.15e+03, 3.75e+00),
    "cbox_64x64_inside": (2.25e+01, 3.16e+02, 3.24e+02, 3.09e+02, 3.20e+02, 3.10e+02, 3.06e+02, 6.99e+00, 6.08e+03, 7.00e+00),
    "cbox_64x64_inside_1x1": (2.28e+01, 3.15e+02, 3.21e+02, 3.08e+02, 3.20e+02, 3.05e+02, 3.05e+02, 6.88e+00, 3.89e+02, 6.80e+00),
}


def image(kind, res, seed=0):
    """(height, width, 4) float32"""
    w, h = res
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "ramp":
        a, b, c = RAMP
        base = a * (x + 0.5) + b * (y + 0.5) + c
        return np.stack([base * (k + 1) for k in range(4)], -1).astype(np.float32)
    if kind == "smooth":
        return np.stack([np.sin(0.31 * x + 0.2 * k) * np.cos(0.23 * y - 0.1 * k) + 0.1 * k for k in range(4)], -1).astype(np.float32)
    return np.random.default_rng(100 + seed).standard_normal((h, w, 4)).astype(np.float32)


def d_color(name, seed=0):
    H, W = PC.points(name).shape[:2]
    return np.random.default_rng(200 + seed).standard_normal((H, W, 4)).astype(np.float32)


def d_view(shape, seed=0):
    return np.random.default_rng(300 + seed).standard_normal(tuple(shape[:2]) + (8,)).astype(np.float32)


def res_of(name):
    return RES.get(name, PC.CASES[name][2])


def camera_of(name):
    return PC.CAMERAS[PC.CASES[name][1]]


@functools.lru_cache(None)
def reference(name, dtype="float64"):
    """``PC.reference`` at this file's image size"""
    if res_of(name) == PC.CASES[name][2]:
        return PC.reference(name, dtype)
    return PR.view_ref(PC.points(name), camera_of(name), res_of(name), PC.oracle_scene(name), np.dtype(dtype).type)


def view32(name):
    """the float32 reference's view buffer of a case: what the host test and the margins are computed on"""
    return reference(name, "float32")["data"]


def uncertain(name, view, filter, footprint):
    """(H, W) bool over the texels of a case for a given view buffer"""
    return VR.dview_uncertain(view, res_of(name), filter, footprint) | reference(name)["uncertain"]


def dview_bars(r32, r64, certain):
    """per channel of DVIEW_CHANNELS: (bar, largest float32 error, largest value)"""
    out = []
    for c in DVIEW_CHANNELS:
        with np.errstate(invalid="ignore"):
            err = float(np.max(np.abs(r32[..., c].astype(np.float64) - r64[..., c])[certain], initial=0.0))
            top = float(np.max(np.abs(r64[..., c])[certain], initial=0.0))
        out.append((max(4.0 * err, FLOOR_ULPS * EPS32 * top), err, top))
    return out


def dview_check(name, kind, filter, footprint, view, got):
    """-> (bad (H, W) bool over certain texels, uncertain (H, W), bars) for a kernel result ``got`` on the view buffer ``view``"""
    img, g = image(kind, res_of(name)), d_color(name)
    r64 = VR.dview_ref(img, view, g, filter, footprint, 0, np.float64)
    r32 = VR.dview_ref(img, view, g, filter, footprint, 0, np.float32)
    unc = uncertain(name, view, filter, footprint)
    bars = dview_bars(r32, r64, ~unc)
    got = np.asarray(got, np.float64)
    bad = np.zeros(unc.shape, bool)
    for c, (bar, _, _) in zip(DVIEW_CHANNELS, bars):
        bad |= ~(np.abs(got[..., c] - r64[..., c]) <= bar)
    for c in (0, 1, 4, 5, 7):
        bad |= got[..., c] != 0
    return bad & ~unc, unc, bars


def camera_bars(points, camera, res, d_view_):
    """-> (float64 gradient (10,), bars (10,), float32 reference's error (10,), sum of |terms| (10,))"""
    import torch
    g64, terms = VR.camera_grad_ref(points, camera, res, d_view_, torch.float64, terms=True)
    g32 = VR.camera_grad_ref(points, camera, res, d_view_, torch.float32)
    err = np.abs(g32 - g64)
    return g64, np.maximum(4.0 * err, FLOOR_ULPS * EPS32 * terms), err, terms


def planar_points(H, W, seed=0):
    """a synthetic (H, W, 16) texel buffer: a tilted plane in front of the standard camera, every texel shaded but a sprinkle of
    unshaded ones (reach 0) and NaN positions — shapes that cross the loop boundaries of the reduction need no scene"""
    rng = np.random.default_rng(400 + seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    pts = np.zeros((H, W, 16), np.float32)
    pts[..., 8] = -2.5 + 5.0 * (u + 0.5) / W
    pts[..., 9] = 0.5 + 4.0 * (v + 0.5) / H
    pts[..., 10] = -1.0 + 0.6 * (u + 0.5) / W - 0.3 * (v + 0.5) / H
    n = np.asarray([-0.6, 0.3, 1.0]) / np.linalg.norm([-0.6, 0.3, 1.0])
    pts[..., 4:7] = n
    pts[..., 7] = 5.0 / W
    pts[..., 12] = 1.0
    holes = rng.random((H, W)) < 0.02
    pts[holes, 12] = 0.0
    nans = rng.random((H, W)) < 0.01
    pts[nans, 8] = np.nan
    return pts


def _round_up(x):
    return 0.0 if x == 0 else float(np.ceil(x / 10.0 ** (np.floor(np.log10(x)) - 2)) * 10.0 ** (np.floor(np.log10(x)) - 2))


if __name__ == "__main__":      # the tables of profiles/texel_viewgrad_margins.txt
    print("float32 references against the float64 ones (tests/texel_viewgrad_ref.py; no GPU involved), on the float32 reference's view "
          "buffer of each case.\nd_view: reached and visible texels, uncertain ones, and per channel the largest absolute error over the "
          "certain texels and the three images (largest value, floor)")
    margins, cam_margins = {}, {}
    for name in CASES:
        view, reached = view32(name), PC.reached(name)
        vis = int((reached & (view[..., 0] != 0)).sum())
        for filter, footprint in FILTERS:
            unc = uncertain(name, view, filter, footprint) & reached
            worst = [(0.0, 0.0)] * 3
            for kind in IMAGES:
                img, g = image(kind, res_of(name)), d_color(name)
                r64 = VR.dview_ref(img, view, g, filter, footprint, 0, np.float64)
                r32 = VR.dview_ref(img, view, g, filter, footprint, 0, np.float32)
                worst = [(max(w[0], b[1]), max(w[1], b[2])) for w, b in zip(worst, dview_bars(r32, r64, ~unc))]
            key = f"{name}/{filter}/{footprint:g}"
            margins[key] = tuple(_round_up(w[0]) for w in worst)
            share = unc.sum() / max(int(reached.sum()), 1)
            print(f"  {key:36s} reached {int(reached.sum()):5d}  visible {vis:5d}  uncertain {int(unc.sum()):3d} ({100 * share:.3f} %"
                  f"{'' if share < MAX_UNCERTAIN_REF else '  ABOVE MAX_UNCERTAIN_REF'})")
            print("    " + "  ".join(f"{ch} {w[0]:.3e} (largest {w[1]:.3e}, floor {FLOOR_ULPS * EPS32 * w[1]:.3e})" for ch, w in zip(("d_X", "d_Y", "d_scale"), worst)))
    print("camera sums: per parameter (fov, origin, target, up) the float32 reference's error / the sum of |terms|, in float32 ulps (2^-24)")
    for name in CASES:
        pts = PC.points(name)
        g64, bars, err, terms = camera_bars(pts, camera_of(name), res_of(name), d_view(pts.shape))
        rel = err / np.where(terms > 0, terms, 1.0) / EPS32
        cam_margins[name] = tuple(_round_up(float(x)) for x in rel)
        print(f"  {name:24s} " + " ".join(f"{x:.3f}" for x in rel))
    print("MARGINS = {")
    for k, v in margins.items():
        print(f'    "{k}": (' + ", ".join(f"{x:.2e}" for x in v) + "),")
    print("}\nCAMERA_MARGINS = {      # in float32 ulps of the sum of |terms|")
    for k, v in cam_margins.items():
        print(f'    "{k}": (' + ", ".join(f"{x:.2e}" for x in v) + "),")
    print("}")
