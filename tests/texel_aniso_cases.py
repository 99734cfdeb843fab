"""The cases of the anisotropic gather that are compared with the float64 reference (tests/texel_aniso_ref.py), shared by the host test
(tests/test_texel_aniso_ref_host.py) and the GPU tests (tests/test_gpu_texel_aniso.py), and their bars.

A case is the sample points of a case of tests/texel_lighting_cases.py, a camera of tests/texel_project_cases.py and an image of
96 x 64: at that size a texel of the Cornell box's walls covers several pixels and the probe counts reach ``max_aniso``.  The STANDARD
camera looks into the box from outside; the INSIDE one stands in the box, so that texels lie behind it and outside its image.

Bars, by the project's rule.  The footprint buffer is compared as ``major``, ``minor`` and the direction up to sign (1 - |e . e_ref|,
only where major / minor >= 1.125: below that the direction selects nothing), over the VISIBLE texels of the float64 view reference —
the texels a gather reads a footprint for; next to the camera plane (the inside camera's invisible texels) the axes grow without bound
and an absolute bar says nothing.  Each bar is 4 x the largest error of the float32 reference against the float64 one (MARGINS,
measured by ``python tests/texel_aniso_cases.py``, which prints profiles/texel_aniso_margins.txt; no GPU involved), floor FLOOR_ULPS
float32 ulps of the largest value.  The gather and its adjoint: the same rule on the kernel's own view and footprint buffers
(``gather_bar``), the exempt texels of ``texel_aniso_ref.exempt`` left out.  At most 1 % of a case's visible texels may be exempt or
failing; the reference alone stays below 0.1 %."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import texel_aniso_ref as AR                                     # noqa: E402
import texel_lighting_cases as LC                                # noqa: E402
import texel_mip_ref as MR                                       # noqa: E402
import texel_project_cases as PC                                 # noqa: E402
import texel_project_ref as PR                                   # noqa: E402

MAX_EXEMPT = 0.01
MAX_EXEMPT_REF = 0.001               # what the reference alone stays below
FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
MIN_RATIO = 1.125                    # the direction is compared from this major / minor on
RES = (96, 64)
QUANTITIES = ("major", "minor", "direction")

# name: (points of texel_lighting_cases, camera of texel_project_cases, (width, height))
CASES = {
    "cbox_16x16_standard": ("cbox_16x16", "standard", RES),
    "cbox_64x64_standard": ("cbox_64x64", "standard", RES),
    "multi_24_standard": ("multi_24_spp4", "standard", RES),
    "cbox_64x64_inside": ("cbox_64x64", "inside", RES),
}

# visible texels, and how many of them take N = 1 .. 8 probes at footprint 1, max_aniso 8 (float64 reference)
PROBE_COUNTS = {
    "cbox_16x16_standard": (117, [36, 0, 16, 35, 16, 0, 3, 11]),
    "cbox_64x64_standard": (1815, [453, 0, 1106, 245, 11, 0, 0, 0]),
    "multi_24_standard": (252, [65, 0, 38, 86, 29, 0, 5, 29]),
    "cbox_64x64_inside": (128, [6, 88, 9, 11, 6, 4, 4, 0]),
}

# largest |float32 reference - float64 reference| of major, minor and 1 - |e . e_ref| over the visible texels
# (python tests/texel_aniso_cases.py; profiles/texel_aniso_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_16x16_standard": (3.99e-06, 2.21e-06, 1.23e-07),
    "cbox_64x64_standard": (1.08e-06, 8.32e-07, 1.34e-07),
    "multi_24_standard": (2.01e-06, 2.40e-06, 1.14e-07),
    "cbox_64x64_inside": (3.08e-06, 3.33e-06, 1.25e-07),
}


def points(name):
    return LC.points(CASES[name][0])


def camera(name):
    return PC.CAMERAS[CASES[name][1]]


@functools.lru_cache(None)
def view_reference(name, dtype="float64"):
    pts, cam, res = CASES[name]
    return PR.view_ref(points(name), PC.CAMERAS[cam], res, LC.oracle_scene(LC.CASES[pts][0]), np.dtype(dtype).type)


@functools.lru_cache(None)
def footprint_reference(name, dtype="float64"):
    return AR.footprint_ref(points(name), camera(name), CASES[name][2], np.dtype(dtype).type)


def visible(name):
    """(H, W) bool: the texels the float64 view reference sees, the uncertain ones left out"""
    ref = view_reference(name)
    return (ref["data"][..., 0] == 1) & ~ref["uncertain"]


def probe_counts(name, footprint=1.0, max_aniso=8):
    """(visible, [how many of them take N = 1 .. max_aniso probes]) of the float64 reference"""
    vis = visible(name)
    N, _ = AR.probes(footprint_reference(name)[vis], footprint, max_aniso)
    return int(vis.sum()), [int((N == k).sum()) for k in range(1, max_aniso + 1)]


def footprint_errors(name, fp):
    """per texel (H, W, 3): |major - ref|, |minor - ref|, 1 - |e . e_ref| (0 where major / minor < MIN_RATIO in the reference)"""
    ref, fp = footprint_reference(name), np.asarray(fp, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(fp[..., 0] * ref[..., 0] + fp[..., 1] * ref[..., 1]) / (fp[..., 3] * ref[..., 3])
        direction = np.where(ref[..., 3] >= MIN_RATIO * ref[..., 2], np.abs(1.0 - e), 0.0)
    return np.stack([np.abs(fp[..., 3] - ref[..., 3]), np.abs(fp[..., 2] - ref[..., 2]), direction], -1)


def footprint_scales(name):
    ref = footprint_reference(name)[visible(name)]
    return float(ref[:, 3].max()), float(ref[:, 2].max()), 1.0


def footprint_bars(name):
    return tuple(max(4.0 * m, FLOOR_ULPS * EPS32 * s) for m, s in zip(MARGINS[name], footprint_scales(name)))


def footprint_failing(name, fp):
    """(H, W) bool: the visible texels where the buffer is off the float64 reference by more than a bar (a NaN fails)"""
    err = footprint_errors(name, fp)
    bad = np.zeros(err.shape[:2], bool)
    for c, b in enumerate(footprint_bars(name)):
        bad |= ~(err[..., c] <= b)
    return bad & visible(name)


def gather_bar(r32, r64, keep=None):
    """the rule of ``texel_mip_ref.linear_bar`` over the texels (or pixels) ``keep``"""
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64)
    if keep is not None:
        r32, r64 = r32[keep], r64[keep]
    return max(4.0 * float(np.abs(r32 - r64).max()), FLOOR_ULPS * EPS32 * float(np.abs(r64).max()))


def images(res=RES):
    """the two images of the quality condition: noise, and noise in 2 x 2 blocks"""
    w, h = res
    noise = np.random.default_rng(0).random((h, w, 4))
    return {"noise": noise, "blocks": np.repeat(np.repeat(noise[::2, ::2], 2, 0), 2, 1)[:h, :w]}


def rmse(name, color, truth):
    vis = visible(name)
    return float(np.sqrt(np.mean((np.asarray(color, np.float64)[vis] - truth[vis]) ** 2)))


if __name__ == "__main__":      # the table of profiles/texel_aniso_margins.txt
    print("float32 reference against the float64 reference (tests/texel_aniso_ref.py; no GPU involved): per case the visible texels, how "
          "many of them take N = 1 .. 8 probes (footprint 1, max_aniso 8), the ratio major / minor, the exempt texels, and the largest "
          "absolute error of major, minor and the direction (1 - |e . e_ref|, where major / minor >= 1.125) over the visible texels")
    for name in CASES:
        vis = visible(name)
        nvis, counts = probe_counts(name)
        ref = footprint_reference(name)
        ratio = ref[vis][:, 3] / ref[vis][:, 2]
        err = footprint_errors(name, footprint_reference(name, "float32"))[vis].max(0)
        ex = AR.exempt(ref, 1.0, 8) & vis
        ex10 = [int((AR.exempt(ref, fpr, m) & vis).sum()) for fpr in (1.0, 0.5) for m in (8, 2)]
        print(f"  {name:22s} visible {nvis:5d}  N = 1 .. 8: {counts}  mean N {sum((k + 1) * c for k, c in enumerate(counts)) / max(nvis, 1):.2f}  "
              f"ratio median {np.median(ratio):.2f} largest {ratio.max():.2f}  exempt {int(ex.sum())} (footprint 1 / 0.5 x max_aniso 8 / 2: {ex10})")
        s = footprint_scales(name)
        print("    " + "  ".join(f"{q} {x:.3e} (largest {y:.3e}, floor {FLOOR_ULPS * EPS32 * y:.3e})" for q, x, y in zip(QUANTITIES, err, s)))
        up = [0.0 if x == 0 else np.ceil(x / 10.0 ** (np.floor(np.log10(x)) - 2)) * 10.0 ** (np.floor(np.log10(x)) - 2) for x in err]
        print(f'    "{name}": (' + ", ".join(f"{x:.2e}" for x in up) + "),")
        print(f'    "{name}": ({nvis}, {counts}),')
    print("quality, float64 reference: RMSE over the visible texels against the mean of the image over the texel's own patch (8 x 8 points)")
    for name in ("cbox_16x16_standard", "cbox_64x64_standard"):
        v64, fp = view_reference(name)["data"], footprint_reference(name)
        for label, image in images().items():
            truth = AR.truth_ref(image, points(name), camera(name), RES)
            row = {"bilinear": PR.gather_ref(image, v64), "mip 1": MR.gather_mip_ref(image, v64, 1.0), "mip 0.5": MR.gather_mip_ref(image, v64, 0.5),
                   "aniso": AR.gather_aniso_ref(image, v64, fp, 1.0, 8)}
            print(f"  {name:22s} {label:7s} " + "  ".join(f"{k} {rmse(name, c, truth):.4f}" for k, c in row.items()))
