"""The cases of the adjoint of the bounced light in the environment map (include/zdr.h, zdr_scene_texel_bounce_backward_env), shared by
the host test (tests/test_texel_bounce_envgrad_host.py), the GPU tests (tests/test_gpu_texel_bounce_envgrad.py) and the margins tool
(tools/texel_bounce_envgrad_margins.py).  A table of its own, by the convention of tests/texel_bounce_cases.py: the parametrised tests over
that module's tables keep their size.

A case is a scene (SceneArrays, slot table, an environment map with its sampling tables), the materials, a texture size, spp, the number
of bounces K, the sampler and a sample range.  All on the geometry of ``texel_bounce_cases.env_bounce_arrays`` — a panel that faces up and
a reflector that sees the panel and the sun, both with a material — or, for env_lit_k2, the panel under an emitting blocker.

  env_k2, env_lit_k2   the cases of tests/texel_bounce_cases.py, as they are (their points, materials and references are shared);
  env_k2_pmj02bn       env_k2 drawn with pmj02bn from seeded tables;
  env_k2_range         env_k2 with the sample subrange [1, 4);
  env_k3               three bounces on the same geometry;
  env_wave             5 x 5 texels and spp 64: a whole wave per texel, and most of its lanes fall into the sun's few cells;
  env_wave_ragged      the same with the 37 samples [3, 40): 32 lanes per texel in two trips, the second one ragged, two texels per wave
                       and an odd number of shaded texels, so that half of the last wave has no texel;
  env_sky              5 x 5 texels and spp 64 under a near-uniform sky with a bright zenith row: the samples of a wave spread over more
                       distinct cells than the merge has rounds, and some fall into the map's top row or its last column, where the
                       footprint is clamped.
The three cases of 25 texels have a list of shaded texels in row-major order (one wave compacts them), so the waves of the shading
kernel are known and the header's count of groups can be predicted exactly.
tests/test_texel_bounce_envgrad_host.py asserts on the float64 reference that the cases are what this list says."""
import functools

import numpy as np

import envmap_tables as ET
import texel_bounce_cases as BC
import texel_bounce_ref as BR
import texel_deep_cases as DC
import texel_lighting_cases as LC
import texel_ref as R
from zdr_amd import envmap as E

SEED = BC.SEED
MERGE_ROUNDS = 4              # ZDR_LGRAD_MERGE_ROUNDS (csrc/bakegrad.h)
WAVE = 64


@functools.lru_cache(None)
def sky_env():
    """(tex, alias_prob, alias_idx, pdf, map_w, map_h): a 16 x 32 sky within 5 % of uniform — the near-uniform sky of
    tools/texel_lighting_grad_cost.py at this size — whose top row is 40 times as bright (per solid angle; the row is small), with the
    tables zdr_amd/envmap.py builds for it without MIS compensation: the samples spread over the whole map, and the up-facing panel
    sends some into the upper half of the top row, where the footprint's base row is -1"""
    img = (1.0 + 0.05 * np.random.default_rng(0).uniform(-1.0, 1.0, (16, 32, 3))).astype(np.float32)
    img[0] *= np.float32(40.0)
    prob, alias, pdf = ET.host_tables(img, False)
    return E.prepare_image(img), prob, alias, pdf, E.SAMPLE_MAP_W, E.SAMPLE_MAP_H


def _case(make, slots, hw, second, spp, K, env, sampler=None, samples=None, shared=None):
    return {"make": make, "slots": slots, "hw": hw, "second": second, "spp": spp, "K": K, "env": env, "sampler": sampler, "samples": samples,
            "shared": shared}


_ENV_K2 = BC.case("env_k2")
_ENV_LIT = BC.case("env_lit_k2")
CASES = {
    "env_k2": _case(*_ENV_K2[:7], shared="env_k2"),
    "env_lit_k2": _case(*_ENV_LIT[:7], shared="env_lit_k2"),
    "env_k2_pmj02bn": _case(*_ENV_K2[:7], sampler=(5, 256)),
    "env_k2_range": _case(*_ENV_K2[:7], samples=(1, 4)),
    "env_k3": _case(*_ENV_K2[:5], 3, _ENV_K2[6]),
    "env_wave": _case(BC.env_bounce_arrays, BC.ENV_SLOTS, (5, 5), (3, 4), 64, 2, LC.sun_env),
    "env_wave_ragged": _case(BC.env_bounce_arrays, BC.ENV_SLOTS, (5, 5), (3, 4), 64, 2, LC.sun_env, samples=(3, 40)),
    "env_sky": _case(BC.env_bounce_arrays, BC.ENV_SLOTS, (5, 5), (3, 4), 64, 2, sky_env),
}
# the cases on a BVH deeper than the LDS part of the traversal stack (tests/texel_deep_cases.py): those of BC.DEEP_CASES that have a map,
# shared with tests/texel_bounce_cases.py as env_k2 is, in a table of their own so that the parametrised tests over CASES keep their size
DEEP_CASES = {n: _case(*BC.case(n)[:7], shared=n) for n in DC.BOUNCE_ENV}
VERTEX_OF_CONDITION_1 = {"env_lit_k2": 1}      # the vertex index (0-based) that must accept 8 environment samples; every other case: 0


def case(name):
    return CASES[name] if name in CASES else DEEP_CASES[name]


@functools.lru_cache(None)
def points(name):
    """(H, W, 16) float32: the sample points of a case, the float32 buffer of tests/texel_ref.py for material 0"""
    c = case(name)
    if c["shared"]:
        return BC.points(c["shared"])
    return np.ascontiguousarray(R.texel_aovs_ref(c["make"](), c["slots"], 0, c["hw"], np.float32)["data"], np.float32)


@functools.lru_cache(None)
def materials(name):
    """the case's materials, float32 (h, w, 4), seeded as tests/texel_bounce_cases.py seeds them"""
    c = case(name)
    if c["shared"]:
        return BC.materials(c["shared"])
    rng = np.random.default_rng(11)
    sizes = [c["hw"]] + ([c["second"]] if c["second"] else [])
    return tuple(np.ascontiguousarray(np.concatenate([rng.uniform(0.2, 0.9, (h, w, 3)), rng.uniform(0.1, 0.9, (h, w, 1))], -1), np.float32) for h, w in sizes)


@functools.lru_cache(None)
def pmj_tables(name):
    from zdr_amd import pmj02bn_tables as T
    n_sets, n_samples = case(name)["sampler"]
    return T.pmj02_sets(n_sets=n_sets, n_samples=n_samples, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2)


def sampler(name):
    return "pmj02bn" if case(name)["sampler"] else "cmj"


def tables(name):
    return pmj_tables(name) if case(name)["sampler"] else None


def sample_range(name):
    c = case(name)
    return c["samples"] if c["samples"] else (0, c["spp"])


def env(name):
    return case(name)["env"]()


def reached(name):
    return points(name)[..., 12] == 1


def run_reference(name, dtype="float64", hits=None, env_tuple=None):
    c = case(name)
    return BR.texel_bounce_ref(c["make"](), LC.oracle_scene(c["make"]), points(name), materials(name), c["slots"], spp=c["spp"], bounces=c["K"], seed=SEED,
                               samples=c["samples"], sampler=sampler(name), env=env(name) if env_tuple is None else env_tuple,
                               dtype=np.dtype(dtype).type, tables=tables(name), hits=hits)


@functools.lru_cache(None)
def reference(name):
    """the free-running float64 reference of the forward: the walks and the bake; shared, read-only"""
    c = case(name)
    if c["shared"]:
        return BC.reference(c["shared"])
    return run_reference(name)


def lanes_shift(name):
    """zdr_bounce_lanes_shift (csrc/bounce.h) for the case's texture and range"""
    h, w = case(name)["hw"]
    b, e = sample_range(name)
    want, cap = (262144 + h * w - 1) // (h * w), min(e - b, WAVE)
    shift = 0
    while (2 << shift) <= cap and (1 << shift) < want:
        shift += 1
    return shift
