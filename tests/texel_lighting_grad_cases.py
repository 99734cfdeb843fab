"""The cases of the adjoint of the texture-space lighting that are compared with the float64 reference (tests/texel_lighting_grad_ref.py),
shared by the host test (tests/test_texel_lighting_grad_ref_host.py) and the GPU tests (tests/test_gpu_texel_lighting_grad.py,
tests/test_zz_gpu_graph_texel_lighting_grad.py), and their bars — by the convention of tests/texel_lighting_cases.py.

A case is a scene (SceneArrays, slot table, optionally an environment map), a texture size, spp, optionally a pmj02bn table and a sample
range.  Its SAMPLE POINTS are the float32 buffer of tests/texel_ref.py for material 0; its COTANGENT is a seeded normal per float, set to 0
on the texels the float64 reference calls uncertain (a discrete decision of one of their samples could flip under float32 rounding, and
a flipped sample moves a whole term): the same floats go to both references and to the kernels.

Bar per gradient entry (a float of d_emission or of d_env): max(4 x margin, 16 x 2^-24 x sum |terms of that entry|).  The margin is the
float32 reference's largest error against the float64 one over the entries of that target (MARGINS below, measured by
``python tests/texel_lighting_grad_cases.py``, which prints profiles/texel_lighting_grad_margins.txt; no GPU involved): the kernels and
the float32 reference may order and round their operations differently.  The second term bounds what any order of summation can cost
(float atomics arrive in any order); it is still a thousand times below the loss of one sample among some hundreds.  A case may have at
most 1 % of its reached texels uncertain."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import many_lights as ML                                         # noqa: E402
import texel_cases as TC                                         # noqa: E402
import texel_deep_cases as DC                                    # noqa: E402
import texel_lighting_cases as LC                                # noqa: E402
import texel_lighting_grad_ref as GR                             # noqa: E402
import texel_lighting_ref as LR                                  # noqa: E402
import texel_ref as R                                            # noqa: E402
from zdr_amd import geometry                                     # noqa: E402

MAX_UNCERTAIN = 0.01
EPS32 = 2.0 ** -24
ORDER_ULPS = 16
SEED = 7
COTANGENT_SEED = 23


@functools.lru_cache(None)
def chandelier_arrays():
    return ML.chandelier_arrays()


@functools.lru_cache(None)
def hall_arrays():
    return ML.hall_arrays()


@functools.lru_cache(None)
def env_panel_lit_arrays():
    """the panel and blocker of texel_lighting_cases.env_panel_arrays, the blocker (it faces the panel) emitting (4, 2, 1)"""
    a = LC.env_panel_arrays()
    return geometry.from_arrays(a.verts, a.tris, a.inst_tri_begin, a.inst_xform, np.array([[0, 0, 0], [4, 2, 1]], np.float32))


# name: (arrays, slot table, (H, W), spp, environment)
CASES = {
    "cbox_16x16": (TC.cbox_arrays, (0, None), (16, 16), 4, None),
    "cbox_16x16_spp1": (TC.cbox_arrays, (0, None), (16, 16), 1, None),
    "multi_24_spp9": (LC.multi_arrays, LC.MULTI_SLOTS, (24, 24), 9, None),
    "chandelier_24": (chandelier_arrays, (0,) + (None,) * 16, (24, 24), 4, None),
    "env_panel_8x8": (LC.env_panel_arrays, (0, None), (8, 8), 4, LC.sun_env),
    "env_panel_lit_16": (env_panel_lit_arrays, (0, None), (16, 16), 4, LC.sun_env),
    "cbox_16x16_pmj_tail": (TC.cbox_arrays, (0, None), (16, 16), 16, None),
}
SAMPLERS = {"cbox_16x16_pmj_tail": (1, 16)}         # pmj02bn from seeded tables of (sets, samples per set); every other case draws with CMJ
RANGES = {"cbox_16x16_pmj_tail": (1, 16)}           # the sample range of a case that does not take all of [0, spp)

# The cases at the edges of the launch shapes (tests/test_gpu_texel_bake_edges.py, tests/test_texel_bake_edges_host.py), looked up by
# ``case(name)`` like the others, in a table of their own so that the parametrised tests over CASES keep their size.  hall_16: 43 lights,
# past the 32 k_lgrad_shade sums on chip.  cbox_wide_40: more live workgroups than the emission accumulator has rows.
EDGE_CASES = {
    "hall_16": (hall_arrays, (0,) + (None,) * 43, (16, 16), 4, None),
    "cbox_wide_40": (TC.cbox_arrays, (0, None), (40, 40), 16, None),
}


# the cases on a BVH deeper than the LDS part of the traversal stack (tests/texel_deep_cases.py), by the same convention
DEEP_CASES = DC.LIGHTING_GRAD


def case(name):
    """the tuple of a case of CASES, of EDGE_CASES or of DEEP_CASES"""
    return CASES[name] if name in CASES else EDGE_CASES[name] if name in EDGE_CASES else DEEP_CASES[name]


# largest |float32 reference - float64 reference| over the entries of each target
# (python tests/texel_lighting_grad_cases.py; profiles/texel_lighting_grad_margins.txt), rounded up in the third digit
MARGINS = {
    "cbox_16x16": {"emission": 1.39e-07},
    "cbox_16x16_spp1": {"emission": 2.32e-07},
    "multi_24_spp9": {"emission": 5.14e-07},
    "chandelier_24": {"emission": 1.45e-07},
    "env_panel_8x8": {"env": 8.76e-07},
    "env_panel_lit_16": {"emission": 6.17e-06, "env": 1.25e-06},
    "cbox_16x16_pmj_tail": {"emission": 5.05e-07},
    # EDGE_CASES
    "hall_16": {"emission": 2.00e-07},
    "cbox_wide_40": {"emission": 7.09e-07},
    **DC.LIGHTING_GRAD_MARGINS,                                       # DEEP_CASES
}


@functools.lru_cache(None)
def points(name):
    """(H, W, 16) float32: the sample points of a case"""
    make, slots, hw = case(name)[:3]
    return np.ascontiguousarray(R.texel_aovs_ref(make(), slots, 0, hw, np.float32)["data"], np.float32)


def reached(name):
    return points(name)[..., 12] == 1


@functools.lru_cache(None)
def pmj_tables(name):
    from zdr_amd import pmj02bn_tables as T
    n_sets, n_samples = SAMPLERS[name]
    return T.pmj02_sets(n_sets=n_sets, n_samples=n_samples, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2)


def _common(name, samples):
    make, _, _, spp, env = case(name)
    pmj = name in SAMPLERS
    return dict(spp=spp, seed=SEED, samples=RANGES.get(name) if samples is None else samples, sampler="pmj02bn" if pmj else "cmj",
                tables=pmj_tables(name) if pmj else None), make, env


@functools.lru_cache(None)
def raw_cotangent(name):
    """(H, W, 4) float32 seeded normals, before the uncertain texels are cleared"""
    h, w = case(name)[2]
    return np.random.default_rng(COTANGENT_SEED).standard_normal((h, w, 4)).astype(np.float32)


@functools.lru_cache(None)
def uncertain(name):
    """(H, W) bool: the uncertain texels of the whole sample range (they do not depend on the cotangent)"""
    kw, make, env = _common(name, None)
    return GR.texel_lighting_grad_ref(make(), LC.oracle_scene(make), points(name), raw_cotangent(name), env=env() if env else None, **kw)["uncertain"]


@functools.lru_cache(None)
def cotangent(name):
    """(H, W, 4) float32: seeded normals, 0 on the uncertain texels"""
    g = raw_cotangent(name).copy()
    g[uncertain(name)] = 0
    return g


@functools.lru_cache(None)
def reference(name, dtype="float64", samples=None):
    kw, make, env = _common(name, samples)
    return GR.texel_lighting_grad_ref(make(), LC.oracle_scene(make), points(name), cotangent(name), env=env() if env else None,
                                      dtype=np.dtype(dtype).type, **kw)


def forward(name, emissions=None, env_tex=None):
    """the float64 forward reference of a case, (H, W, 3); ``emissions`` (ninst, 3) with the case's light list; ``env_tex``: another
    (float64) map under the case's tables"""
    kw, make, env = _common(name, None)
    e = env() if env else None
    if e is not None and env_tex is not None:
        e = (env_tex,) + tuple(e[1:])
    if emissions is not None:                                   # the light list stays the case's: light_table takes the rows that are positive
        assert [i for i in range(make().ninst) if (np.asarray(emissions)[i] > 0).any()] == lights(name)
    return LR.texel_lighting_ref(make(), LC.oracle_scene(make), points(name), env=e, emissions=emissions, dtype=np.float64, **kw)["data"][..., :3]


def lights(name):
    """the instances that emit"""
    return GR.light_instances(case(name)[0]())


def targets(name):
    return (("emission",) if lights(name) else ()) + (("env",) if case(name)[4] else ())


def entries(ref, target):
    """(gradient, sum |terms|) of a target, the alpha channel of the map dropped"""
    if target == "emission":
        return ref["d_emission"], ref["abs_emission"]
    return ref["d_env"][..., :3], ref["abs_env"][..., :3]


def error(name, target, got, ref=None):
    """largest |got - float64 reference| over the entries of a target; ``got`` has the target's shape"""
    ref = reference(name) if ref is None else ref
    want, _ = entries(ref, target)
    got = np.asarray(got, np.float64)
    return float(np.abs((got if target == "emission" else got[..., :3]) - want).max())


def bar(name, target, ref=None):
    """the bar of every entry of a target, in its shape"""
    ref = reference(name) if ref is None else ref
    return np.maximum(4.0 * MARGINS[name][target], ORDER_ULPS * EPS32 * entries(ref, target)[1])


def failing(name, target, got, ref=None):
    ref = reference(name) if ref is None else ref
    want, _ = entries(ref, target)
    got = np.asarray(got, np.float64)
    return np.abs((got if target == "emission" else got[..., :3]) - want) > bar(name, target, ref)


def table_lines(names=None):
    """the table of profiles/texel_lighting_grad_margins.txt for the cases ``names`` (None: CASES)"""
    lines = [f"float32 reference against the float64 reference (tests/texel_lighting_grad_ref.py; no GPU involved), seed {SEED}, cotangent seed "
             f"{COTANGENT_SEED}: largest absolute error over the entries of each target"]
    for name in (CASES if names is None else names):
        ref, r32 = reference(name), reference(name, "float32")
        rch = reached(name)
        line = f"  {name:19s} reached {int(rch.sum()):4d}  uncertain {int((rch & ref['uncertain']).sum()):3d}  lights {len(lights(name)):2d}"
        for target in ("emission", "env"):
            if target not in targets(name):
                continue
            want, a = entries(ref, target)
            e = error(name, target, entries(r32, target)[0])
            line += (f"  | {target}: largest |entry| {np.abs(want).max():.4e}  largest sum|terms| {a.max():.4e}  error {e:.3e}"
                     f"  order term at most {ORDER_ULPS * EPS32 * a.max():.3e}")
        if "emission" in targets(name):
            n = ref["n_emission"][lights(name)]
            line += f"  | terms per light {int(n.min())} .. {int(n.max())}"
        if "env" in targets(name):
            line += f"  | texels lit by the map {int((ref['lit_env'] > 0).sum())}, by a mesh light {int((ref['lit_mesh'] > 0).sum())}, map texels with a term {int((ref['n_env'] > 0).sum())}"
        lines.append(line)
    return lines


def kernel_lines(names):
    """from a GPU: the kernels' own distance to their bars (the figures tests/test_gpu_texel_lighting_grad.py prints)"""
    import test_gpu_texel_lighting_grad as T
    lines = ["the kernels against the float64 reference, on an MI355X: largest error per target and its largest share of an entry's bar"]
    for name in names:
        for accel in ("brute", "bvh"):
            got = T.run_case(name, accel, targets(name))
            for target, g in got.items():
                want, _ = entries(reference(name), target)
                err = np.abs((g if target == "emission" else g[..., :3]).astype(np.float64) - want)
                lines.append(f"  [texel lighting grad] {name} {accel} {target}: largest error {err.max():.3e}, {(err / np.maximum(bar(name, target), 1e-300)).max():.3f} of its bar")
    return lines


if __name__ == "__main__":      # the table of profiles/texel_lighting_grad_margins.txt; --edges: of EDGE_CASES; --deep: of DEEP_CASES; --gpu: the kernels' lines for them
    names = list(EDGE_CASES) if "--edges" in sys.argv else list(DEEP_CASES) if "--deep" in sys.argv else None
    print("\n".join(kernel_lines(names or list(CASES)) if "--gpu" in sys.argv else table_lines(names)))
