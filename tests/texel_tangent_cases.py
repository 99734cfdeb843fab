"""The cases of the UV tangents that are compared with the float64 reference (tests/texel_tangent_ref.py), shared by the host test
(tests/test_texel_tangent_ref_host.py) and the GPU tests (tests/test_gpu_texel_tangents.py), and their bars.

A tangent case is (SceneArrays, slot table, material, (H, W)), as in tests/texel_cases.py: three of its cases, the Cornell box on two
NON-SQUARE textures (16 x 64 and 64 x 16: every texel is a 4 : 1 rectangle on the surface), the stretched panel mirrored in u (the
orientation of the other sign), a 1 x 1 texture (every triangle degenerate: all zeros) and a material that no instance has.  A footprint
case adds a camera and the 96 x 64 image of tests/texel_aniso_cases.py.

Bars, by the project's rule: 4 x the largest error of the float32 reference against the float64 one over the compared texels (MARGINS
and FOOTPRINT_MARGINS, measured by ``python tests/texel_tangent_cases.py``, which prints profiles/texel_tangent_margins.txt; no GPU
involved), floor FLOOR_ULPS float32 ulps of the channel's scale: the largest |component| of a tangent, the largest area.  ``orientation``
and the zero rows are compared exactly.  The footprint is compared as tests/texel_aniso_cases.py compares it, over the visible texels of
the float64 view reference.  At most 1 % of a case's texels may be uncertain, at most 1 % of the visible ones exempt from the gather
comparison."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import texel_aniso_cases as AC                                   # noqa: E402
import texel_aniso_ref as AR                                     # noqa: E402
import texel_cases as TC                                         # noqa: E402
import texel_lighting_cases as LC                                # noqa: E402
import texel_mip_ref as MR                                       # noqa: E402
import texel_project_cases as PC                                 # noqa: E402
import texel_project_ref as PR                                   # noqa: E402
import texel_ref as R                                            # noqa: E402
import texel_tangent_ref as TR                                   # noqa: E402
from zdr_amd import geometry                                     # noqa: E402
from zdr_amd.scenes import CBOX_CAMERA, panel_mesh               # noqa: E402

MAX_UNCERTAIN = TC.MAX_UNCERTAIN
MAX_EXEMPT = AC.MAX_EXEMPT
FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
RES = AC.RES
UNUSED_MATERIAL = 3


@functools.lru_cache(None)
def panel_mirrored_arrays():
    """texel_cases.panel_arrays with u -> 1 - u: the same surface under a mirrored chart"""
    v, t = panel_mesh(3, 2)
    v = v.copy()
    v[:, 3:5] = np.float32(0.0712) + np.float32(0.8371) * v[:, 3:5]
    v[:, 3] = np.float32(1.0) - v[:, 3]
    v[:, 5:8] = np.array([0.28, 0.96, 0.0], np.float32)
    return geometry.from_arrays(v, t, inst_xform=TC.PANEL_XFORM.reshape(1, 16))


CASES = {
    "cbox_5x7": TC.CASES["cbox_5x7"],
    "panel_3x2": TC.CASES["panel_3x2"],
    "soup_130": TC.CASES["soup_130"],
    "cbox_16x64": (TC.cbox_arrays, (0, None), 0, (16, 64)),
    "cbox_64x16": (TC.cbox_arrays, (0, None), 0, (64, 16)),
    "panel_mirrored": (panel_mirrored_arrays, (0,), 0, (10, 11)),
    "cbox_1x1": (TC.cbox_arrays, (0, None), 0, (1, 1)),
    "cbox_no_instance": (TC.cbox_arrays, (0, None), UNUSED_MATERIAL, (5, 7)),
}
ORIENTATION = {"cbox_5x7": -1, "cbox_16x64": -1, "cbox_64x16": -1, "panel_3x2": 1, "soup_130": 1, "panel_mirrored": -1}

# The panel lies tilted in space (texel_cases.PANEL_XFORM); this camera stands off its upper side and sees all of it.
PANEL_CAMERA = (CBOX_CAMERA[0], (0.9, 0.6, 5.6), (1.62, -0.55, 2.5), (0.0, 1.0, 0.0))
# name: (tangent case, camera, (width, height))
FOOTPRINT_CASES = {
    "cbox_16x64": ("cbox_16x64", PC.CAMERAS["standard"], RES),
    "cbox_64x16": ("cbox_64x16", PC.CAMERAS["standard"], RES),
    "panel_3x2": ("panel_3x2", PANEL_CAMERA, RES),
}
QUALITY_CASES = ("cbox_16x64", "cbox_64x16")
SANITY_CASES = ("cbox_16x16_standard", "cbox_64x64_standard", "multi_24_standard")        # of texel_aniso_cases

# largest |float32 reference - float64 reference| of (a tangent component, area) over the compared texels, and the largest relative
# |area - texel_size^2| of the float32 reference (python tests/texel_tangent_cases.py; profiles/texel_tangent_margins.txt), rounded up
MARGINS = {
    "cbox_5x7": (6.13e-07, 3.73e-06, 2.22e-07),
    "panel_3x2": (5.68e-08, 2.56e-08, 3.18e-07),
    "soup_130": (7.50e-08, 5.09e-09, 2.71e-07),
    "cbox_16x64": (2.74e-07, 1.48e-07, 2.41e-07),
    "cbox_64x16": (5.47e-07, 2.38e-07, 2.85e-07),
    "panel_mirrored": (7.21e-08, 2.56e-08, 3.18e-07),
    "cbox_1x1": (0.0, 0.0, 0.0),
    "cbox_no_instance": (0.0, 0.0, 0.0),
}
# largest |float32 reference - float64 reference| of major, minor and 1 - |e . e_ref| over the visible texels, both on the float32
# reference's buffers
FOOTPRINT_MARGINS = {
    "cbox_16x64": (2.59e-06, 7.95e-07, 1.23e-07),
    "cbox_64x16": (3.73e-06, 5.74e-07, 1.17e-07),
    "panel_3x2": (1.29e-06, 1.61e-06, 9.35e-08),
}


@functools.lru_cache(None)
def reference(name, dtype="float64"):
    """the dict of texel_tangent_ref.tangents_ref: ``data`` (H, W, 8) and ``aovs``, the dict of texel_ref.texel_aovs_ref"""
    make, slots, material, hw = CASES[name]
    return TR.tangents_ref(make(), slots, material, hw, np.dtype(dtype).type)


def compared(name):
    """(H, W) bool: the texels of a case on which anything is compared with the float64 reference"""
    return ~reference(name)["aovs"]["uncertain"]


def reached(name):
    return reference(name)["aovs"]["data"][..., 12] == 1


def scales(name):
    """(largest |tangent component|, largest area): what a float32 ulp is measured against"""
    d = np.abs(reference(name)["data"])
    return float(max(d[..., 0:3].max(), d[..., 4:7].max())), float(d[..., 3].max())


def errors(name, data):
    """largest |data - float64 reference| of (a tangent component, area) over the compared texels that the reference reaches"""
    keep = compared(name) & reached(name)
    if not keep.any():
        return 0.0, 0.0
    d = np.abs(np.asarray(data, np.float64) - reference(name)["data"])[keep]
    return float(max(d[:, 0:3].max(), d[:, 4:7].max())), float(d[:, 3].max())


def bars(name):
    return tuple(max(4.0 * m, FLOOR_ULPS * EPS32 * s) for m, s in zip(MARGINS[name][:2], scales(name)))


def area_relative_error(tangents, aovs):
    """largest |area - texel_size^2| / texel_size^2 over the texels with texel_size > 0"""
    ts = np.asarray(aovs, np.float64)[..., 7]
    keep = ts > 0
    if not keep.any():
        return 0.0
    return float(np.max(np.abs(np.asarray(tangents, np.float64)[..., 3][keep] - ts[keep] ** 2) / ts[keep] ** 2))


def area_bar(name):
    """the relative bar of area against texel_size^2: two roundings of a float32 product apart at the least"""
    return max(4.0 * MARGINS[name][2], FLOOR_ULPS * EPS32)


# ------------------------------------------------------------------------------------------------------------------ footprint cases
@functools.lru_cache(None)
def points(name):
    """(H, W, 16) float32: the sample points of a tangent case — the float32 buffer of tests/texel_ref.py, as texel_lighting_cases.points"""
    return np.ascontiguousarray(reference(name, "float32")["aovs"]["data"], np.float32)


def oracle_scene(name):
    return LC.oracle_scene(CASES[FOOTPRINT_CASES[name][0]][0])


@functools.lru_cache(None)
def view_reference(name, dtype="float64"):
    case, cam, res = FOOTPRINT_CASES[name]
    return PR.view_ref(points(case), cam, res, oracle_scene(name), np.dtype(dtype).type)


def visible(name):
    """(H, W) bool: the texels the float64 view reference sees, the uncertain ones left out"""
    ref = view_reference(name)
    return (ref["data"][..., 0] == 1) & ~ref["uncertain"]


def footprint_reference(name, dtype="float64", pts=None, tangents=None):
    """texel_tangent_ref.footprint_tangents_ref of a footprint case, on ``pts`` and ``tangents`` (default: the float32 reference's)"""
    case, cam, res = FOOTPRINT_CASES[name]
    pts = points(case) if pts is None else pts
    tangents = reference(case, "float32")["data"] if tangents is None else tangents
    return TR.footprint_tangents_ref(pts, tangents, cam, res, np.dtype(dtype).type)


def footprint_errors(fp, ref):
    """per texel (H, W, 3): |major - ref|, |minor - ref|, 1 - |e . e_ref| (0 where major / minor < MIN_RATIO in the reference)"""
    ref, fp = np.asarray(ref, np.float64), np.asarray(fp, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(fp[..., 0] * ref[..., 0] + fp[..., 1] * ref[..., 1]) / (fp[..., 3] * ref[..., 3])
        direction = np.where(ref[..., 3] >= AC.MIN_RATIO * ref[..., 2], np.abs(1.0 - e), 0.0)
    return np.stack([np.abs(fp[..., 3] - ref[..., 3]), np.abs(fp[..., 2] - ref[..., 2]), direction], -1)


def footprint_bars(name, ref):
    r = np.asarray(ref)[visible(name)]
    s = (float(r[:, 3].max()), float(r[:, 2].max()), 1.0)
    return tuple(max(4.0 * m, FLOOR_ULPS * EPS32 * x) for m, x in zip(FOOTPRINT_MARGINS[name], s))


def footprint_failing(name, fp, ref):
    """(H, W) bool: the visible texels where ``fp`` is off the float64 reference ``ref`` by more than a bar (a NaN fails)"""
    err = footprint_errors(fp, ref)
    bad = np.zeros(err.shape[:2], bool)
    for c, b in enumerate(footprint_bars(name, ref)):
        bad |= ~(err[..., c] <= b)
    return bad & visible(name)


def rmse(name, color, truth):
    vis = visible(name)
    return float(np.sqrt(np.mean((np.asarray(color, np.float64)[vis] - truth[vis]) ** 2)))


@functools.lru_cache(None)
def truths(name):
    """{image label: truth_uv_ref} of a quality case, on the float64 tangents: computed once, shared by the host and the GPU test"""
    case, cam, res = FOOTPRINT_CASES[name]
    return {label: TR.truth_uv_ref(image, points(case), reference(case)["data"], cam, res) for label, image in AC.images().items()}


def quality_row(name, image, view, fp_square, fp_uv):
    """the five gathers of the quality table in float64 on one view buffer: {label: (H, W, 4)}"""
    return {"bilinear": PR.gather_ref(image, view), "mip 1": MR.gather_mip_ref(image, view, 1.0), "mip 0.5": MR.gather_mip_ref(image, view, 0.5),
            "aniso square": AR.gather_aniso_ref(image, view, fp_square, 1.0, 8), "aniso uv": AR.gather_aniso_ref(image, view, fp_uv, 1.0, 8)}


def _up(x):
    return 0.0 if x == 0 else float(np.ceil(x / 10.0 ** (np.floor(np.log10(x)) - 2)) * 10.0 ** (np.floor(np.log10(x)) - 2))


if __name__ == "__main__":      # the table of profiles/texel_tangent_margins.txt
    print("float32 reference against the float64 reference (tests/texel_tangent_ref.py; no GPU involved): largest absolute error of a tangent "
          "component and of the area over the compared texels, and the largest relative |area - texel_size^2| of the float32 reference")
    for name in CASES:
        ref, r32 = reference(name), reference(name, "float32")
        unc = ref["aovs"]["uncertain"]
        e, s = errors(name, r32["data"]), scales(name)
        rel = area_relative_error(r32["data"], r32["aovs"]["data"])
        zero = int((TR.zero_rows(ref["data"]) & reached(name)).sum())
        ori = sorted(set(ref["data"][..., 7][reached(name) & ~TR.zero_rows(ref["data"])].tolist()))
        print(f"  {name:17s} texels {unc.size:5d}  reached {int(reached(name).sum()):5d}  uncertain {int(unc.sum()):3d}  zero rows among the reached {zero:4d}  "
              f"orientation {ori}  tangent {e[0]:.3e} (largest {s[0]:.3e}, floor {FLOOR_ULPS * EPS32 * s[0]:.3e})  area {e[1]:.3e} "
              f"(largest {s[1]:.3e}, floor {FLOOR_ULPS * EPS32 * s[1]:.3e})  area against texel_size^2 {rel:.3e}")
        print(f'    "{name}": ({_up(e[0]):.2e}, {_up(e[1]):.2e}, {_up(rel):.2e}),')
    print("footprint from tangents: per case the visible texels, the ratio major / minor, the exempt texels, and the largest absolute error of "
          "major, minor and the direction (1 - |e . e_ref|, where major / minor >= 1.125) over the visible texels")
    for name in FOOTPRINT_CASES:
        vis = visible(name)
        ref, r32 = footprint_reference(name), footprint_reference(name, "float32")
        ratio = ref[vis][:, 3] / ref[vis][:, 2]
        err = footprint_errors(r32, ref)[vis].max(0)
        ex = AR.exempt(ref, 1.0, 8) & vis
        print(f"  {name:12s} visible {int(vis.sum()):5d}  ratio median {np.median(ratio):.2f} largest {ratio.max():.2f}  exempt {int(ex.sum())}  "
              + "  ".join(f"{q} {x:.3e}" for q, x in zip(AC.QUANTITIES, err)))
        print(f'    "{name}": (' + ", ".join(f"{_up(x):.2e}" for x in err) + "),")
    print("sanity: on the isotropic charts of texel_aniso_cases the UV footprint's major and minor against the square patch's major, largest relative difference")
    for name in SANITY_CASES:
        case = AC.CASES[name][0]
        make, slots, hw = LC.CASES[case][:3]
        tan = TR.tangents_ref(make(), slots, 0, hw, np.float64)["data"]
        vis = AC.visible(name)
        sq = AC.footprint_reference(name)
        uv = TR.footprint_tangents_ref(AC.points(name), tan, AC.camera(name), AC.CASES[name][2])
        print(f"  {name:22s} |major - major| / major {np.max(np.abs(uv[vis][:, 3] - sq[vis][:, 3]) / sq[vis][:, 3]):.3e}  "
              f"|minor - minor| / major {np.max(np.abs(uv[vis][:, 2] - sq[vis][:, 2]) / sq[vis][:, 3]):.3e}")
    print("quality, float64 reference: RMSE over the visible texels against the mean of the image over the texel's TRUE patch (8 x 8 points)")
    for name in QUALITY_CASES:
        case, cam, res = FOOTPRINT_CASES[name]
        v64 = view_reference(name)["data"]
        fp_sq, fp_uv = AR.footprint_ref(points(case), cam, res), footprint_reference(name, tangents=reference(case)["data"])
        for label, image in AC.images().items():
            row = quality_row(name, image, v64, fp_sq, fp_uv)
            print(f"  {name:12s} {label:7s} " + "  ".join(f"{k} {rmse(name, c, truths(name)[label]):.4f}" for k, c in row.items()))
