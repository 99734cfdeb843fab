"""The cases of the texture-space views that are compared with the float64 reference (tests/texel_project_ref.py), shared by the host
test (tests/test_texel_project_ref_host.py) and the GPU tests (tests/test_gpu_texel_project.py), and their bars.

A case is the sample points of a case of tests/texel_lighting_cases.py (the float32 buffer of tests/texel_ref.py for material 0 — the
same floats go to both references and to the kernels), a camera and an image size.  Two cameras: the STANDARD one looks into the box
from outside, the INSIDE one stands in the box and looks at a corner, so that texels lie behind it and outside its image.  Image sizes:
24 x 16 (not square: a wrong aspect shows) and 1 x 1.

Bars, by the convention of tests/texel_cases.py.  ``visible`` must be equal outside the uncertain texels.  Every continuous channel —
cosine, pixel x, pixel y, depth, distance, scale — has a bar of 4 x the largest error of the float32 reference against the float64 one
over the compared texels (MARGINS below, measured by ``python tests/texel_project_cases.py``, which prints
profiles/texel_project_margins.txt; no GPU involved), with a floor of FLOOR_ULPS float32 ulps of the channel's largest value.  The
gather and its adjoint: the same rule on the kernel's own view buffer (``linear_bar``).  A case may have at most 1 %
of its reached texels uncertain or failing."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import texel_deep_cases as DC                                    # noqa: E402
import texel_lighting_cases as LC                                # noqa: E402
import texel_project_ref as PR                                   # noqa: E402
from zdr_amd.scenes import CBOX_CAMERA                           # noqa: E402

MAX_UNCERTAIN = 0.01
MAX_UNCERTAIN_REF = 0.001            # what the reference alone stays below
FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
CHANNELS = ("cosine", "pixel_x", "pixel_y", "depth", "distance", "scale")      # floats 1 .. 6 of the view buffer

CAMERAS = {
    "standard": (CBOX_CAMERA[0], (-0.2, 2.6, 6.0), (-0.2, 2.6, -2.5), (0.0, 1.0, 0.0)),
    "inside": (CBOX_CAMERA[0], (0.3, 2.0, 0.5), (2.5, 1.0, -1.5), (0.0, 1.0, 0.0)),
    **DC.cameras(),
}

# name: (points of texel_lighting_cases, camera, (width, height))
CASES = {
    "cbox_16x16_standard": ("cbox_16x16", "standard", (24, 16)),
    "cbox_64x64_standard": ("cbox_64x64", "standard", (24, 16)),
    "multi_24_standard": ("multi_24_spp4", "standard", (24, 16)),
    "cbox_16x16_inside": ("cbox_16x16", "inside", (24, 16)),
    "cbox_64x64_inside": ("cbox_64x64", "inside", (24, 16)),
    "cbox_64x64_inside_1x1": ("cbox_64x64", "inside", (1, 1)),
}

# reached, behind, outside, visible, occluded, seen from behind, uncertain: measured with the oracle's any-hit query
CLASSES = {
    "cbox_16x16_standard": (208, 0, 48, 117, 43, 6, 0),
    "cbox_64x64_standard": (3052, 0, 572, 1815, 665, 44, 0),
    "multi_24_standard": (445, 0, 90, 252, 103, 8, 0),
    "cbox_16x16_inside": (208, 33, 161, 5, 9, 0, 0),
    "cbox_64x64_inside": (3052, 466, 2356, 128, 102, 7, 1),
    "cbox_64x64_inside_1x1": (3052, 466, 2290, 175, 121, 8, 3),
}

# largest |float32 reference - float64 reference| per channel of CHANNELS over the compared texels
# (python tests/texel_project_cases.py; profiles/texel_project_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_16x16_standard": (8.78e-08, 2.08e-06, 1.72e-06, 4.77e-07, 1.26e-06, 5.67e-07),
    "cbox_64x64_standard": (1.44e-07, 2.54e-06, 2.15e-06, 4.77e-07, 1.37e-06, 1.68e-07),
    "multi_24_standard": (1.02e-07, 2.35e-06, 1.58e-06, 4.77e-07, 1.31e-06, 4.47e-07),
    "cbox_16x16_inside": (1.25e-07, 4.06e-03, 9.70e-04, 5.14e-07, 4.82e-07, 1.03e-03),
    "cbox_64x64_inside": (1.51e-07, 5.09e-01, 2.18e-01, 5.81e-07, 5.35e-07, 3.24e-02),
    "cbox_64x64_inside_1x1": (1.51e-07, 2.12e-02, 9.06e-03, 5.81e-07, 5.35e-07, 1.35e-03),
    **DC.VIEW_MARGINS,                                                # DEEP_CASES
}

# the view down a shaft whose BVH is deeper than the LDS part of the traversal stack (tests/texel_deep_cases.py): the same tuples,
# looked up by ``case(name)``, in a table of their own so that the parametrised tests over CASES keep their size
DEEP_CASES = DC.VIEW


def case(name):
    return CASES[name] if name in CASES else DEEP_CASES[name]


def points(name):
    return LC.points(case(name)[0])


def oracle_scene(name):
    return LC.oracle_scene(LC.case(case(name)[0])[0])


@functools.lru_cache(None)
def reference(name, dtype="float64"):
    _, cam, res = case(name)
    return PR.view_ref(points(name), CAMERAS[cam], res, oracle_scene(name), np.dtype(dtype).type)


def reached(name):
    return points(name)[..., 12] == 1


def compared(name):
    """(H, W) bool: the reached texels of a case that are not uncertain"""
    return reached(name) & ~reference(name)["uncertain"]


def classes(name):
    """(reached, behind, outside, visible, occluded, seen from behind, uncertain) of the float64 reference"""
    ref, r = reference(name), reached(name)
    d = ref["data"]
    vis = r & (d[..., 0] == 1)
    return (int(r.sum()), int((r & ~ref["front"]).sum()), int((r & ref["front"] & ~ref["inside"]).sum()), int(vis.sum()),
            int((r & ref["inside"] & ~vis).sum()), int((vis & (d[..., 1] < 0)).sum()), int((r & ref["uncertain"]).sum()))


def scales(name):
    """the largest |value| of each channel over the reached texels: what a float32 ulp is measured against"""
    d = np.abs(reference(name)["data"][reached(name)])
    return tuple(float(d[:, c].max()) for c in range(1, 7))


def errors(name, data):
    """largest |data - float64 reference| per channel over the compared texels"""
    d = np.abs(np.asarray(data, np.float64) - reference(name)["data"])[compared(name)]
    return tuple(float(d[:, c].max()) for c in range(1, 7))


def bars(name):
    return tuple(max(4.0 * m, FLOOR_ULPS * EPS32 * s) for m, s in zip(MARGINS[name], scales(name)))


def failing(name, data):
    """(H, W) bool: the texels where the buffer is off the float64 reference — visible at all, a continuous channel by more than its bar"""
    ref = reference(name)["data"]
    data = np.asarray(data, np.float64)
    bad = data[..., 0] != ref[..., 0]
    for c, b in zip(range(1, 7), bars(name)):
        bad |= ~(np.abs(data[..., c] - ref[..., c]) <= b)
    return bad


def linear_bar(view, src, res, adjoint):
    """The bar of the gather (or, with ``adjoint``, of its transpose) on one view buffer and one input: 4 x the float32 reference's own
    error against the float64 one, floor FLOOR_ULPS float32 ulps of the float64 result's largest value.  For the adjoint the float32
    reference adds in texel order; the kernel's atomics add in another, which the factor 4 is for.  -> (bar, float64 result)"""
    fn = (lambda d: PR.gather_adjoint_ref(src, view, res, d)) if adjoint else (lambda d: PR.gather_ref(src, view, d))
    r64, r32 = fn(np.float64), fn(np.float32)
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(r32.astype(np.float64) - r64)))
    return max(4.0 * err, FLOOR_ULPS * EPS32 * float(np.nanmax(np.abs(r64)))), r64


def cbox_first_hits(res=(24, 16), seed=0):
    """The oracle's first hits of the Cornell box through the standard camera at ``res``, spp 1, tent filter off — the camera ray of
    pixel_ray from the sampler's own draw, the closest hit and the surface point there (zdro_surface_interact) — as an (h, w, 16) buffer
    in the layout of the texel buffers: normal, position and reach = the pixel's ray hit something.  -> (points, hit mask)"""
    import oracle
    import texel_cases as TC
    w, h = res
    osc = LC.oracle_scene(TC.cbox_arrays)
    o, fwd, right, upp, tan, aspect = PR.camera_frame(CAMERAS["standard"], res)
    F = np.float32
    rays = np.zeros((h * w, 8), np.float32)
    for y in range(h):
        for x in range(w):
            u = oracle.sampler_dump(oracle.SAMPLER_CMJ, x, y, seed, 1, 0, 1, 2)[:2]
            px = (F(2.0) / F(w) * (F(x) + u[0]) - F(1.0)) * tan
            py = (F(2.0) / F(h) * (F(y) + u[1]) - F(1.0)) * aspect * tan
            d = (right * px - upp * py + fwd).astype(F)
            d = (d * (F(1.0) / np.sqrt(PR._dot(d, d)))).astype(F)
            rays[y * w + x] = (*o, 0.0, *d, 1e30)
    ip, bt = osc.trace_closest(rays)
    hit = ip[:, 0] >= 0
    rows = np.zeros((h * w, 16), np.float32)
    rows[:, 0:2] = ip.view(np.float32); rows[:, 2:4] = bt[:, 0:2]
    surf = osc.light_rows("interact", rows[hit])
    pts = np.zeros((h * w, 16), np.float32)
    k = np.nonzero(hit)[0]
    pts[k, 8:11] = surf[:, 0:3]; pts[k, 4:7] = surf[:, 5:8]; pts[k, 12] = 1.0
    return pts.reshape(h, w, 16), hit.reshape(h, w)


def round_trip_exempt(view64, res):
    """(h, w) bool: hit pixels whose own projection lies within 1e-3 pixel of a pixel's border, or that the reference calls uncertain"""
    X, Y = view64["data"][..., 2], view64["data"][..., 3]
    near = (np.abs(X - np.rint(X)) < PR.BORDER_TOL) | (np.abs(Y - np.rint(Y)) < PR.BORDER_TOL)
    return near | view64["uncertain"]


if __name__ == "__main__":      # the table of profiles/texel_project_margins.txt
    print("float32 reference against the float64 reference (tests/texel_project_ref.py; no GPU involved): the classes of each case and the "
          "largest absolute error per channel over the compared texels")
    for name in CASES:
        c = classes(name)
        e, s = errors(name, reference(name, "float32")["data"]), scales(name)
        v32 = reference(name, "float32")["data"][..., 0][compared(name)] != reference(name)["data"][..., 0][compared(name)]
        print(f"  {name:22s} reached {c[0]:5d}  behind {c[1]:4d}  outside {c[2]:5d}  visible {c[3]:5d}  occluded {c[4]:4d}  seen from behind {c[5]:3d}  "
              f"uncertain {c[6]:2d}  visible differs {int(v32.sum())}")
        print("    " + "  ".join(f"{ch} {x:.3e} (largest {y:.3e}, floor {FLOOR_ULPS * EPS32 * y:.3e})" for ch, x, y in zip(CHANNELS, e, s)))
        up = [0.0 if x == 0 else np.ceil(x / 10.0 ** (np.floor(np.log10(x)) - 2)) * 10.0 ** (np.floor(np.log10(x)) - 2) for x in e]
        print(f'    "{name}": (' + ", ".join(f"{x:.2e}" for x in up) + "),")
