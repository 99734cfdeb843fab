"""The cases of the texture-space lighting that are compared with the float64 reference (tests/texel_lighting_ref.py), shared by the host
test (tests/test_texel_lighting_ref_host.py) and the GPU tests (tests/test_gpu_texel_lighting.py), and their bars.

A case is a scene (SceneArrays, slot table, optionally an environment map), a texture size, spp and max_distance.  Its SAMPLE POINTS are
the float32 buffer of tests/texel_ref.py for material 0 — the same floats go to the float64 reference, to the float32 reference and to
the kernels (any buffer with the normal, position and reach channels is a valid input), so the comparison is of the estimator alone.

Bars, by the convention of tests/texel_cases.py.  Irradiance: 4 x the largest error of the float32 reference against the float64 one over
the texels that are not uncertain (MARGINS below, measured by ``python tests/texel_lighting_cases.py``, which prints
profiles/texel_lighting_margins.txt; no GPU involved), because the kernels and the float32 reference may order and round their
operations differently, with a floor of FLOOR_ULPS float32 ulps of the case's largest irradiance.  Openness: exact equality (with the
float64 value rounded to float32) — it is a count over spp.  A case may have at most 1 % of its reached texels uncertain."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import envmap_tables as ET                                       # noqa: E402
import texel_cases as TC                                         # noqa: E402
import texel_deep_cases as DC                                    # noqa: E402
import texel_lighting_ref as LR                                  # noqa: E402
import texel_ref as R                                            # noqa: E402
from oracle import OracleScene                                   # noqa: E402
from zdr_amd import envmap as E                                  # noqa: E402
from zdr_amd import geometry, scenes                             # noqa: E402

MAX_UNCERTAIN = 0.01
FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
SEED = 7

MULTI_SLOTS = (0, None, None, None, None)


@functools.lru_cache(None)
def multi_arrays():
    return scenes.multi_light_arrays()


@functools.lru_cache(None)
def env_panel_arrays():
    """A panel of 3 x 2 cells facing up (atlas shrunk into the texture's interior, as texel_cases.panel_arrays) and, 0.6 above it, a
    blocker of a quarter of its size over one corner: part of the panel sees the whole sky, part of it sees the blocker.  Both are tilted
    by 17 degrees about z (a normal of exactly +y sits on make_onb's branch, which the reference calls uncertain).  Nothing emits: every
    light sample goes to the environment map."""
    v, t = scenes.panel_mesh(3, 2)
    v = v.copy()
    v[:, 3:5] = np.float32(0.0712) + np.float32(0.8371) * v[:, 3:5]
    bv, bt = scenes.panel_mesh(1, 1)
    flip = np.array([[0.5, 0, 0, 0.45], [0, -1, 0, 0.6], [0, 0, -0.5, 0.4], [0, 0, 0, 1]], np.float32)      # faces down, like the blocker of multi_light_arrays
    c, s = np.cos(np.radians(17.0)), np.sin(np.radians(17.0))
    tilt = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    return geometry.from_arrays(np.concatenate([v, bv]), np.concatenate([t, bt + v.shape[0]]), [0, t.shape[0], t.shape[0] + bt.shape[0]],
                                np.stack([tilt.reshape(16), (tilt @ flip).reshape(16)]))


@functools.lru_cache(None)
def sun_env():
    """(tex, alias_prob, alias_idx, pdf, map_w, map_h): a 16 x 32 sky with a sun of a few texels about 35 degrees from the zenith, and
    the tables zdr_amd/envmap.py builds for it (MIS compensation on: almost every sample goes to the sun)"""
    img = ET.make_map("sun_sky", (16, 32))
    prob, alias, pdf = ET.host_tables(img, True)
    return E.prepare_image(img), prob, alias, pdf, E.SAMPLE_MAP_W, E.SAMPLE_MAP_H


# name: (arrays, slot table, (H, W), spp, max_distance, environment)
CASES = {
    "cbox_16x16": (TC.cbox_arrays, (0, None), (16, 16), 4, None, None),
    "cbox_64x64": (TC.cbox_arrays, (0, None), (64, 64), 4, None, None),
    "multi_24_spp4": (multi_arrays, MULTI_SLOTS, (24, 24), 4, None, None),
    "multi_24_spp9": (multi_arrays, MULTI_SLOTS, (24, 24), 9, None, None),
    "env_panel_8x8": (env_panel_arrays, (0, None), (8, 8), 4, None, sun_env),
    "cbox_16x16_ao": (TC.cbox_arrays, (0, None), (16, 16), 4, 1.0, None),
    "cbox_16x16_pmj02bn": (TC.cbox_arrays, (0, None), (16, 16), 4, None, None),
    "cbox_16x16_pmj_tail": (TC.cbox_arrays, (0, None), (16, 16), 16, None, None),
}
# Every other case draws with CMJ; these with pmj02bn, from seeded tables of (sets, samples per set).  The tail case: one set of exactly
# spp samples, 8 lanes per texel and the 15 samples [1, 16) — in the second trip the last lane of a texel has no sample left, and a
# sample index past the range's end would be an index past the table's end.
SAMPLERS = {"cbox_16x16_pmj02bn": (5, 256), "cbox_16x16_pmj_tail": (1, 16)}
RANGES = {"cbox_16x16_pmj_tail": (1, 16)}           # the sample range of a case that does not take all of [0, spp)

# largest |float32 reference - float64 reference| of the irradiance over the texels that are compared
# (python tests/texel_lighting_cases.py; profiles/texel_lighting_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_16x16": 4.14e-07,
    "cbox_64x64": 1.44e-06,
    "multi_24_spp4": 1.67e-06,
    "multi_24_spp9": 9.23e-07,
    "env_panel_8x8": 2.68e-04,
    "cbox_16x16_ao": 4.14e-07,
    "cbox_16x16_pmj02bn": 2.36e-07,
    "cbox_16x16_pmj_tail": 1.76e-07,
    **DC.LIGHTING_MARGINS,                                            # DEEP_CASES
}

# The cases on a BVH deeper than the LDS part of the traversal stack (tests/texel_deep_cases.py), and the sample points of its view
# case: the same tuples, looked up by ``case(name)``, in a table of their own so that the parametrised tests over CASES keep their size.
DEEP_CASES = {**DC.LIGHTING, **DC.LIGHTING_POINTS}


def case(name):
    """the tuple of a case of CASES or of DEEP_CASES"""
    return CASES[name] if name in CASES else DEEP_CASES[name]


@functools.lru_cache(None)
def points(name):
    """(H, W, 16) float32: the sample points of a case"""
    make, slots, hw = case(name)[:3]
    return np.ascontiguousarray(R.texel_aovs_ref(make(), slots, 0, hw, np.float32)["data"], np.float32)


@functools.lru_cache(None)
def oracle_scene(make):
    return OracleScene.from_arrays(make())


@functools.lru_cache(None)
def pmj_tables(name):
    """(pmj, bn): the seeded pmj02bn tables of a case, for the reference's sampler dump and for the scene alike"""
    from zdr_amd import pmj02bn_tables as T
    n_sets, n_samples = SAMPLERS[name]
    return T.pmj02_sets(n_sets=n_sets, n_samples=n_samples, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2)


@functools.lru_cache(None)
def reference(name, dtype="float64", samples=None):
    make, slots, hw, spp, max_distance, env = case(name)
    pmj = name in SAMPLERS
    return LR.texel_lighting_ref(make(), oracle_scene(make), points(name), spp=spp, seed=SEED, samples=RANGES.get(name) if samples is None else samples,
                                 max_distance=max_distance, sampler="pmj02bn" if pmj else "cmj", env=env() if env else None,
                                 dtype=np.dtype(dtype).type, tables=pmj_tables(name) if pmj else None)


def reached(name):
    return points(name)[..., 12] == 1


def compared(name):
    """(H, W) bool: the reached texels of a case that are not uncertain"""
    return reached(name) & ~reference(name)["uncertain"]


def scale(name):
    """the case's largest irradiance: what a float32 ulp is measured against"""
    return float(reference(name)["data"][..., :3].max())


def error(name, data):
    """largest |data - float64 reference| of the irradiance over the compared texels"""
    d = np.abs(np.asarray(data, np.float64)[..., :3] - reference(name)["data"][..., :3])
    return float(d[compared(name)].max())


def bar(name):
    return max(4.0 * MARGINS[name], FLOOR_ULPS * EPS32 * scale(name))


def failing(name, data, ref=None):
    """(H, W) bool: the texels where either output is off the float64 reference — irradiance by more than the bar, openness at all"""
    ref = reference(name) if ref is None else ref
    data = np.asarray(data)
    irr = np.abs(data[..., :3].astype(np.float64) - ref["data"][..., :3]).max(-1) > bar(name)
    opn = data[..., 3].astype(np.float32) != ref["data"][..., 3].astype(np.float32)
    return irr | opn


if __name__ == "__main__":      # the table of profiles/texel_lighting_margins.txt
    print(f"float32 reference against the float64 reference (tests/texel_lighting_ref.py; no GPU involved), seed {SEED}: largest absolute error of the "
          "irradiance over the compared texels")
    for name in CASES:
        ref, r32 = reference(name), reference(name, "float32")
        keep = compared(name)
        e, s = error(name, r32["data"]), scale(name)
        opn = int((r32["data"][..., 3][keep].astype(np.float32) != ref["data"][..., 3][keep].astype(np.float32)).sum())
        lit0 = int((reached(name) & (ref["lit"] == 0)).sum())
        print(f"  {name:19s} texels {keep.size:5d}  reached {int(reached(name).sum()):5d}  uncertain {int((reached(name) & ref['uncertain']).sum()):3d}  unlit {lit0:5d}"
              f"  largest irradiance {s:.4e}  error {e:.3e} ({e / s:.2e} of it)  openness differs {opn}   floor ({FLOOR_ULPS} ulps) {FLOOR_ULPS * EPS32 * s:.3e}")
