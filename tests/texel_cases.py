"""The cases of the texture-space feature buffers that are compared with the float64 reference (tests/texel_ref.py), shared by the host
test (tests/test_texel_ref_host.py) and the GPU test (tests/test_gpu_texel_aovs.py), and their bars.

A case is (SceneArrays, slot table, material, (H, W)).  The discrete channels (coverage, reach, instance, slot, and the winners) are
compared exactly outside the case's UNCERTAIN texels — those where, in float64, some candidate triangle's deciding quantity lies within
1e-4 pixels of zero (texel_ref.texel_aovs_ref) — and a case may have at most 1 % of them.  The continuous channels are compared on the
same texels with the bar of ``bars``: 4 x the error of the float32 reference against the float64 one (MARGINS below, measured by
``python tests/texel_cases.py``, which prints profiles/texel_aovs_margins.txt; no GPU involved), because the kernels and the float32
reference may order their operations differently, with a floor of FLOOR_ULPS float32 ulps of the channel's scale: the scene's extent for
position, 1 for the normal, the largest texel size for texel_size."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script)
    sys.path.insert(0, ROOT)

import texel_ref as R                                            # noqa: E402
from zdr_amd import geometry                                     # noqa: E402
from zdr_amd.scenes import cbox_models, panel_mesh               # noqa: E402

MAX_UNCERTAIN = 0.01
FLOOR_ULPS = 4
EPS32 = 2.0 ** -24

PANEL_XFORM = np.array([[0.8, -0.36, 0.48, 1.5], [0.6, 0.48, -0.64, -0.7], [0.0, 0.8, 0.6, 2.25], [0, 0, 0, 1]], np.float32) @ np.diag([1.5, 1.0, 0.75, 1.0]).astype(np.float32)
SOUP_XFORM = np.array([[0.6, 0.0, 0.8, -1.0], [0.0, 1.25, 0.0, 0.5], [-0.8, 0.0, 0.6, 3.0], [0, 0, 0, 1]], np.float32)
SOUP_HW = (40, 48)


@functools.lru_cache(None)
def cbox_arrays():
    return geometry.assemble(cbox_models())


@functools.lru_cache(None)
def panel_arrays():
    """panel_mesh(3, 2) with its atlas shrunk into the texture's interior (the unit square puts a lattice point on every border edge),
    under a rotation, a non-uniform scale and a translation: world space is not object space."""
    v, t = panel_mesh(3, 2)
    v = v.copy()
    v[:, 3:5] = np.float32(0.0712) + np.float32(0.8371) * v[:, 3:5]
    v[:, 5:8] = np.array([0.28, 0.96, 0.0], np.float32)           # a tilted normal: the inverse transpose is not the matrix itself
    return geometry.from_arrays(v, t, inst_xform=PANEL_XFORM.reshape(1, 16))


@functools.lru_cache(None)
def soup_arrays():
    """A seeded triangle soup of 130 triangles (two waves of shade slots, the second partial) for a 48 x 40 texture.  g = 0, 1: two large
    triangles, nearly half of the texture each, with a band of about three texels between them (the wave-cooperative route).  g = 2 .. 101:
    sub-texel slivers, 0.7 texels long and 0.05 wide, most without a lattice point.  g = 102 .. 129: triangles of 4 to 14 texels, of both
    windings, overlapping each other and the large ones.  Where the large ones lie they win every texel (the lowest g); in the band and on
    the rim the others decide it among themselves.  World positions are a smooth function of uv, so a sliver is small in the world too;
    normals are seeded, within 25 degrees of +y."""
    rng = np.random.default_rng(20241)
    H, W = SOUP_HW
    uv = [[(0.02, 0.02), (0.98, 0.02), (0.02, 0.98)], [(0.98, 0.10), (0.98, 0.98), (0.10, 0.98)]]
    for _ in range(100):
        c = rng.uniform(0.05, 0.95, 2)
        a = rng.uniform(0, np.pi)
        d, n = np.array([np.cos(a), np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
        px = [-0.35 * d, 0.35 * d, 0.05 * n + rng.uniform(-0.3, 0.3) * d]
        uv.append([tuple(c + p / np.array([W - 1, H - 1])) for p in px])
    for k in range(28):
        c = rng.uniform(0.1, 0.9, 2)
        r = rng.uniform(4, 14) / np.array([W - 1, H - 1])
        a = np.sort(rng.uniform(0, 2 * np.pi, 3))
        a = a + np.array([0.0, 0.4, 0.8]) * (a[1] - a[0] < 0.4)     # (keep it from collapsing)
        tri = [tuple(c + 0.5 * r * np.array([np.cos(t), np.sin(t)])) for t in a]
        uv.append(tri[::-1] if k % 2 else tri)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    verts = np.zeros((uv.shape[0], 8), np.float32)
    u, v = uv[:, 0], uv[:, 1]
    verts[:, 0] = 4 * u - 2; verts[:, 1] = 0.5 * np.sin(3 * u) * np.cos(2 * v); verts[:, 2] = 3 * v - 1
    verts[:, 3:5] = uv
    n = np.stack([0.4 * rng.uniform(-1, 1, uv.shape[0]), np.ones(uv.shape[0]), 0.4 * rng.uniform(-1, 1, uv.shape[0])], 1)
    verts[:, 5:8] = n / np.linalg.norm(n, axis=1, keepdims=True)
    tris = np.arange(uv.shape[0], dtype=np.int32).reshape(-1, 3)
    assert tris.shape[0] == 130
    return geometry.from_arrays(verts, tris, inst_xform=SOUP_XFORM.reshape(1, 16))


CASES = {
    "cbox_8x8": (cbox_arrays, (0, None), 0, (8, 8)),
    "cbox_16x16": (cbox_arrays, (0, None), 0, (16, 16)),
    "cbox_5x7": (cbox_arrays, (0, None), 0, (5, 7)),
    "cbox_64x64": (cbox_arrays, (0, None), 0, (64, 64)),
    "panel_3x2": (panel_arrays, (0,), 0, (10, 11)),
    "soup_130": (soup_arrays, (0,), 0, SOUP_HW),
}

# largest |float32 reference - float64 reference| of (position, normal, texel_size) over the texels that are compared
# (python tests/texel_cases.py; profiles/texel_aovs_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_8x8": (9.93e-07, 9.20e-08, 6.24e-07),
    "cbox_16x16": (8.01e-07, 9.19e-08, 3.41e-07),
    "cbox_5x7": (6.97e-07, 9.08e-08, 3.19e-07),
    "cbox_64x64": (1.43e-06, 1.18e-07, 7.55e-08),
    "panel_3x2": (3.60e-07, 9.15e-08, 5.06e-08),
    "soup_130": (7.83e-07, 1.48e-07, 2.98e-08),
}


@functools.lru_cache(None)
def reference(name, dtype="float64"):
    make, slots, material, hw = CASES[name]
    return R.texel_aovs_ref(make(), slots, material, hw, np.dtype(dtype).type)


def compared(name):
    """(H, W) bool: the texels of a case on which anything is compared with the float64 reference"""
    return ~reference(name)["uncertain"]


def scales(name):
    """(extent, 1, largest texel size): what a float32 ulp is measured against, per continuous channel"""
    make = CASES[name][0]
    P = R.world_triangles(make(), np.float64)[0]
    return float(np.abs(P).max()), 1.0, float(reference(name)["data"][..., 7].max())


def errors(name, data):
    """largest |data - float64 reference| of (position, normal, texel_size) over the compared texels that the reference reaches"""
    ref = reference(name)["data"]
    keep = compared(name) & (ref[..., 12] == 1)
    d = np.abs(np.asarray(data, np.float64) - ref)[keep]
    return float(d[:, 8:11].max()), float(d[:, 4:7].max()), float(d[:, 7].max())


def bars(name):
    return tuple(max(4.0 * m, FLOOR_ULPS * EPS32 * s) for m, s in zip(MARGINS[name], scales(name)))


if __name__ == "__main__":      # the table of profiles/texel_aovs_margins.txt
    print("float32 reference against the float64 reference (tests/texel_ref.py; no GPU involved): largest absolute error over the compared texels")
    for name in CASES:
        ref = reference(name)
        unc = ref["uncertain"]
        e = errors(name, reference(name, "float32")["data"])
        s = scales(name)
        print(f"  {name:11s} texels {unc.size:5d}  covered {int(ref['data'][..., 11].sum()):5d}  reached {int(ref['data'][..., 12].sum()):5d}  uncertain {int(unc.sum()):3d}"
              f"  position {e[0]:.3e}  normal {e[1]:.3e}  texel_size {e[2]:.3e}   floors ({FLOOR_ULPS} ulps) {FLOOR_ULPS * EPS32 * s[0]:.3e} {FLOOR_ULPS * EPS32 * s[1]:.3e} {FLOOR_ULPS * EPS32 * s[2]:.3e}")
