"""The cases of the bounced light that are compared with the float64 reference (tests/texel_bounce_ref.py), shared by the host test
(tests/test_texel_bounce_ref_host.py) and the GPU tests (tests/test_gpu_texel_bounce.py), and their bars.

A case is a scene (SceneArrays, slot table, optionally an environment map), the materials, a texture size, spp, the number of bounces K,
the sampler and a sample range.  The SAMPLE POINTS are those of tests/texel_lighting_cases.py where the scene is one of its scenes — the
float32 buffer of tests/texel_ref.py for material 0 — and the seed is its seed, 7.  The smallest shapes that still cross every branch:
the Cornell box at 16 x 16 with one and with three bounces; the light stage at 24 x 24 and spp 9, where 8 lanes per texel run two trips
and the last lane runs short in the second, with a second material of ANOTHER size on the down-facing slab, so that vertices land on a
material that is not the baked one; a panel under an environment map with a tilted reflector above it that carries a material too;
pmj02bn from seeded tables; a sample subrange.

Bars.  MARGINS[case] is the largest |float32 reference - float64 reference| of a vertex's ``add`` over the samples whose flags and
triangles agree (``python tests/texel_bounce_cases.py`` prints the host part of profiles/texel_bounce_margins.txt; no GPU involved).  The kernels' beta
and add must lie within max(4 x MARGINS, 4 float32 ulps of the case's largest add) of the float64 reference run on the kernels' own hits."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import texel_bounce_ref as BR                                    # noqa: E402
import texel_cases as TC                                         # noqa: E402
import texel_deep_cases as DC                                    # noqa: E402
import texel_lighting_cases as LC                                # noqa: E402
import texel_ref as R                                            # noqa: E402
from zdr_amd import geometry, scenes                             # noqa: E402

SEED = LC.SEED
FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
MAX_SET_ASIDE = 0.01          # samples whose flags differ from the reference's on the same hits
MIN_WALK_AGREEMENT = 0.99     # samples whose free-running walk agrees in nvert and triangles
MAX_FRAGILE = 0.0025          # samples whose signature changes under a +-4.8e-6 perturbation of the barycentrics
BARY_EPS = 4.8e-6             # the largest float32-against-float64 barycentric error of profiles/ray_cases_margins.txt

MULTI_SLOTS = (0, None, None, 1, None)
ENV_SLOTS = (0, 1)


@functools.lru_cache(None)
def env_bounce_arrays():
    """env_panel_arrays of tests/texel_lighting_cases.py with the blocker turned into a reflector: the same panel of 3 x 2 cells facing up,
    tilted by 17 degrees about z, and on the side of it that lies away from the sun of ``sun_env`` a reflector: a slab that stands almost
    upright, its front turned towards the sun's azimuth and 15 degrees down — it sees the panel AND the sun, so that light samples at
    vertices on either model are accepted.  Nothing emits: every light sample goes to the environment map."""
    v, t = scenes.panel_mesh(3, 2)
    v = v.copy()
    v[:, 3:5] = np.float32(0.0712) + np.float32(0.8371) * v[:, 3:5]
    bv, bt = scenes.panel_mesh(1, 1)
    az = np.array([0.773, 0.0, -0.634])                           # the sun's azimuth (the sun itself: about (0.33, 0.90, -0.27))
    d = np.radians(15.0)
    nrm = np.cos(d) * az + np.array([0.0, -np.sin(d), 0.0])       # the front's normal: the slab's local +y
    tan = np.array([0.634, 0.0, 0.773])                           # local x: horizontal, along the slab
    up = np.cross(tan, nrm)                                       # local z (x cross y)
    centre = -0.6 * az + np.array([0.0, 0.95, 0.0])
    flip = np.eye(4, dtype=np.float32)
    flip[:3, 0], flip[:3, 1], flip[:3, 2], flip[:3, 3] = 1.0 * tan, nrm, 0.8 * up, centre
    c, s = np.cos(np.radians(17.0)), np.sin(np.radians(17.0))
    tilt = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    return geometry.from_arrays(np.concatenate([v, bv]), np.concatenate([t, bt + v.shape[0]]), [0, t.shape[0], t.shape[0] + bt.shape[0]],
                                np.stack([tilt.reshape(16), (tilt @ flip).reshape(16)]))


# name: (arrays, slot table, (H, W), second material's size or None, spp, K, environment, points of this texel_lighting case or None)
CASES = {
    "cbox_k1": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 1, None, "cbox_16x16"),
    "cbox_k3": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 3, None, "cbox_16x16"),
    "multi_k3": (LC.multi_arrays, MULTI_SLOTS, (24, 24), (5, 7), 9, 3, None, "multi_24_spp9"),
    "env_k2": (env_bounce_arrays, ENV_SLOTS, (12, 12), (3, 4), 4, 2, LC.sun_env, None),
    "cbox_pmj02bn_k2": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 2, None, "cbox_16x16"),
    "cbox_k3_range": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 3, None, "cbox_16x16"),
}


@functools.lru_cache(None)
def hall_arrays():
    import many_lights as ML
    return ML.hall_arrays()


def _lit_panel_arrays():
    import texel_lighting_grad_cases as GC
    return GC.env_panel_lit_arrays()


HALL_SLOTS = (0,) + (None,) * 43

# The cases at the edges of the launch shapes (tests/test_gpu_texel_bake_edges.py, tests/test_texel_bake_edges_host.py): the same
# tuples, looked up by ``case(name)`` like the others, but in a table of their own so that the parametrised tests over CASES keep their
# size.  hall: 43 lights, past the 32 the adjoint sums on chip.  cbox_k8: the documented maximum of bounces, with CMJ and with pmj02bn.
# cbox_wave*: 64 texels, so a whole wave per texel at spp 64, one lane for a single sample, 32 lanes in two trips (the second ragged) for
# the 37 samples [3, 40).  cbox_wide: more live workgroups than the emission accumulator has rows and than its 64 x 64 material has
# copies of its cells.  tiny_*: material tables of 4, 28, 30 and 12 + 6 staging cells (MATERIAL_SIZES) around ZDR_LDS_CELLS = 28.
# cbox_k3_nan: NaNs in two sample points (NAN_POINTS).  env_lit_k2: an environment map and a mesh light in one light list.
EDGE_CASES = {
    "hall_k2": (hall_arrays, HALL_SLOTS, (16, 16), None, 4, 2, None, None),
    "cbox_k8": (TC.cbox_arrays, (0, None), (8, 8), None, 4, 8, None, None),
    "cbox_k8_pmj02bn": (TC.cbox_arrays, (0, None), (8, 8), None, 4, 8, None, None),
    "cbox_wave": (TC.cbox_arrays, (0, None), (8, 8), None, 64, 2, None, None),
    "cbox_wave_one": (TC.cbox_arrays, (0, None), (8, 8), None, 64, 2, None, None),
    "cbox_wave_ragged": (TC.cbox_arrays, (0, None), (8, 8), None, 64, 2, None, None),
    "cbox_wide": (TC.cbox_arrays, (0, None), (40, 40), None, 16, 2, None, None),
    "tiny_1x1": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 3, None, "cbox_16x16"),
    "tiny_3x6": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 3, None, "cbox_16x16"),
    "tiny_4x5": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 3, None, "cbox_16x16"),
    "tiny_multi": (LC.multi_arrays, MULTI_SLOTS, (16, 16), None, 9, 3, None, None),
    "cbox_k3_nan": (TC.cbox_arrays, (0, None), (16, 16), None, 4, 3, None, "cbox_16x16"),
    "env_lit_k2": (_lit_panel_arrays, ENV_SLOTS, (16, 16), (3, 4), 4, 2, LC.sun_env, None),
}
MATERIAL_SIZES = {"cbox_wide": ((64, 64),), "tiny_1x1": ((1, 1),), "tiny_3x6": ((3, 6),), "tiny_4x5": ((4, 5),), "tiny_multi": ((2, 3), (1, 2))}   # materials that are not sized by the sample points
# (row-major index of a reached texel's rank, float of its row): a NaN in a position and, 100 reached texels on, one in a normal
NAN_POINTS = {"cbox_k3_nan": ((20, 9), (120, 5))}

# The cases on a BVH deeper than the LDS part of the traversal stack (tests/texel_deep_cases.py; tests/test_gpu_texel_deep_stack.py,
# tests/test_texel_deep_stack_host.py): the same tuples, in a table of their own like EDGE_CASES.
DEEP_CASES = DC.BOUNCE

SAMPLERS = {"cbox_pmj02bn_k2": (5, 256), "cbox_k8_pmj02bn": (5, 256), **DC.BOUNCE_SAMPLERS}   # pmj02bn from seeded tables of (sets, samples per set); every other case draws with CMJ
RANGES = {"cbox_k3_range": (1, 4), "cbox_wave_one": (0, 1), "cbox_wave_ragged": (3, 40)}   # the sample range of a case that does not take all of [0, spp)

# largest |float32 reference - float64 reference| of a vertex's add over the samples whose signatures agree
# (python tests/texel_bounce_cases.py; profiles/texel_bounce_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_k1": 1.71e-06,
    "cbox_k3": 4.67e-06,
    "multi_k3": 4.54e-05,
    "env_k2": 5.19e-05,
    "cbox_pmj02bn_k2": 2.86e-06,
    "cbox_k3_range": 4.67e-06,
    # EDGE_CASES
    "hall_k2": 3.80e-05,
    "cbox_k8": 9.20e-07,
    "cbox_k8_pmj02bn": 8.99e-07,
    "cbox_wave": 2.32e-05,
    "cbox_wave_one": 1.45e-06,
    "cbox_wave_ragged": 2.53e-06,
    "cbox_wide": 7.00e-05,
    "tiny_1x1": 3.35e-06,
    "tiny_3x6": 3.80e-06,
    "tiny_4x5": 2.40e-06,
    "tiny_multi": 3.84e-05,
    "cbox_k3_nan": 4.67e-06,
    "env_lit_k2": 2.30e-05,
    **DC.BOUNCE_MARGINS,                                              # DEEP_CASES
}


def case(name):
    """the tuple of a case of CASES, of EDGE_CASES or of DEEP_CASES"""
    return CASES[name] if name in CASES else EDGE_CASES[name] if name in EDGE_CASES else DEEP_CASES[name]


def bounces(name):
    return case(name)[5]


def nan_texels(name):
    """[(y, x, float), ...]: the floats of the case's sample points that hold a NaN (NAN_POINTS), as texels of the buffer"""
    make, slots, hw = case(name)[:3]
    clean = LC.points(case(name)[7])
    ys, xs = np.nonzero(clean[..., 12] == 1)
    return [(int(ys[rank]), int(xs[rank]), f) for rank, f in NAN_POINTS.get(name, ())]


@functools.lru_cache(None)
def points(name):
    """(H, W, 16) float32: the sample points of a case"""
    make, slots, hw = case(name)[:3]
    if name in NAN_POINTS:
        pts = LC.points(case(name)[7]).copy()
        for y, x, f in nan_texels(name):
            pts[y, x, f] = np.nan
        return pts
    if case(name)[7] is not None:
        return LC.points(case(name)[7])
    return np.ascontiguousarray(R.texel_aovs_ref(make(), slots, 0, hw, np.float32)["data"], np.float32)


def material_sizes(name):
    if name in MATERIAL_SIZES:
        return list(MATERIAL_SIZES[name])
    return [case(name)[2]] + ([case(name)[3]] if case(name)[3] else [])


@functools.lru_cache(None)
def materials(name):
    """the case's materials, float32 (h, w, 4): a seeded random albedo in [0.2, 0.9] and a roughness the walk ignores"""
    rng = np.random.default_rng(11)
    sizes = material_sizes(name)
    return tuple(np.ascontiguousarray(np.concatenate([rng.uniform(0.2, 0.9, (h, w, 3)), rng.uniform(0.1, 0.9, (h, w, 1))], -1), np.float32) for h, w in sizes)


@functools.lru_cache(None)
def pmj_tables(name):
    from zdr_amd import pmj02bn_tables as T
    n_sets, n_samples = SAMPLERS[name]
    return T.pmj02_sets(n_sets=n_sets, n_samples=n_samples, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2)


def run_reference(name, dtype="float64", samples=None, mats=None, K=None, hits=None, oscene=None, spp=None, seed=SEED):
    make, slots, hw, _, case_spp, case_K, env, _ = case(name)
    pmj = name in SAMPLERS
    return BR.texel_bounce_ref(make(), LC.oracle_scene(make) if oscene is None else oscene, points(name), materials(name) if mats is None else mats, slots,
                               spp=case_spp if spp is None else spp, bounces=case_K if K is None else K, seed=seed,
                               samples=RANGES.get(name) if samples is None else samples, sampler="pmj02bn" if pmj else "cmj",
                               env=env() if env else None, dtype=np.dtype(dtype).type, tables=pmj_tables(name) if pmj else None, hits=hits)


@functools.lru_cache(None)
def reference(name, dtype="float64"):
    """the case's reference, computed once and shared: treat it as read-only"""
    return run_reference(name, dtype)


def reached(name):
    return points(name)[..., 12] == 1


def scale(name):
    """the case's largest add: what a float32 ulp is measured against"""
    return float(reference(name)["add"].max())


def margin(name):
    """(largest |float32 - float64| of a vertex's add over the samples whose signatures agree, how many samples agree, how many there are)"""
    a, b = reference(name), reference(name, "float32")
    same = BR.signature_equal(a, b)
    return float(np.abs(a["add"][same] - b["add"][same].astype(np.float64)).max()), int(same.sum()), int(same.size)


def bar(name):
    return max(4.0 * MARGINS[name], FLOOR_ULPS * EPS32 * scale(name))


def env_accept_share(name):
    """the share of the case's bounce vertices whose accepted light sample came from the environment map (a case without mesh lights)"""
    ref = reference(name)
    have = np.arange(bounces(name))[None, :] < ref["nvert"][:, None]
    return float(((ref["flags"] & BR.F_ADDED) != 0)[have].mean()) if have.any() else 0.0


def ceiling_statement(direct, bounced, points):
    """(ceiling texels, those with direct irradiance exactly 0, those with bounced light) of lighting buffers over the sample points ``points``"""
    ceiling = (points[..., 12] == 1) & (points[..., 5] < -0.99)
    return int(ceiling.sum()), int((ceiling & (direct[..., :3].sum(-1) == 0)).sum()), int((ceiling & (bounced[..., :3].sum(-1) > 0)).sum())


def perturbed_signature_changes(name, pattern):
    """How many samples change signature — triangle per vertex and flags — when the barycentrics of every hit of the float64 reference
    are moved by +-BARY_EPS with the seeded sign pattern ``pattern``: the reference shades the moved hits (``hits=``), and from the
    first vertex whose flags differ the free-running walk would have gone elsewhere."""
    ref = reference(name)
    rng = np.random.default_rng(100 + pattern)
    sign = rng.choice(np.array([-1.0, 1.0]), size=ref["uv"].shape)
    hits = {"nvert": ref["nvert"], "inst": ref["inst"], "prim": ref["prim"], "uv": (ref["uv"] + BARY_EPS * sign).astype(np.float32)}
    moved = run_reference(name, hits=hits)
    return int((~BR.signature_equal(ref, moved)).sum()), int(ref["nvert"].size)


def table_lines(names=None):
    """the host part of profiles/texel_bounce_margins.txt (tools/texel_bounce_margins.py adds the kernels' walks on a GPU) for the cases
    ``names`` (None: CASES)"""
    names = list(CASES) if names is None else list(names)
    lines = [f"float32 reference against the float64 reference (tests/texel_bounce_ref.py; no GPU involved), seed {SEED}: largest absolute error of a "
             "vertex's add over the samples whose signatures (nvert, triangle and flags per vertex) agree"]
    for name in names:
        ref = reference(name)
        e, same, total = margin(name)
        s = scale(name)
        near = int(ref["near"][:, -1].sum())
        lines.append(f"  {name:16s} samples {total:5d}  signatures agree {same:5d}  near {near:4d}  vertices {int(ref['nvert'].sum()):6d}  accepted {int(((ref['flags'] & BR.F_ADDED) != 0).sum()):6d}"
                     f"  largest add {s:.4e}  error {e:.3e} ({e / s:.2e} of it)  floor ({FLOOR_ULPS} ulps) {FLOOR_ULPS * EPS32 * s:.3e}"
                     f"  mean bounced irradiance {float(ref['data'][..., :3][reached(name)].mean()):.4f}")
    if "env_k2" in names:
        lines.append(f"share of the bounce vertices of env_k2 that accept an environment sample: {env_accept_share('env_k2'):.3f}")
    for name in names:
        changes = [perturbed_signature_changes(name, k)[0] for k in range(4)]
        lines.append(f"  {name:16s} samples that change signature under +-{BARY_EPS:g} on every barycentric, four sign patterns: {changes} of {reference(name)['nvert'].size}")
    return lines


if __name__ == "__main__":      # the host part of profiles/texel_bounce_margins.txt
    print("\n".join(table_lines()))
