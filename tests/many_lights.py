"""Scenes with more lights than the emission-gradient kernels' on-chip table holds (ZDR_EMIT_LDS_LIGHTS = 10, zdr_kernels.hip), and the
oracle-side measurement both the host preconditions (test_many_lights_host.py) and the GPU tests (test_gpu_many_lights.py) rest on;
and the hall, with more lights than the table of the texture-space adjoints holds (32; test_gpu_texel_bake_edges.py).
Importable without a GPU; built from the repository's own assets and zdr_amd.scenes."""
from math import acos, cos, pi, sin

import numpy as np

from zdr_amd import Camera, float3, float4x4, geometry
from zdr_amd.scenes import ASSETS, cbox_models, panel_mesh

LDS_LIGHTS = 10                                                  # ZDR_EMIT_LDS_LIGHTS: a light with list index >= 10 takes emit_add's fallback

# the render both test files use for the oracle's forward: the backward is called with seed OSEED - 1
OW, OSPP, OSEED = 48, 16, 6


# ------------------------------------------------------------------------------------------------------------ chandelier
PANELS = 14
PANEL_XZ = [(x, z) for z in (-4.6, -3.0, -1.4, 0.2) for x in (-2.0, -0.8, 0.4, 1.6)][:PANELS]   # z-major
BLOCKER_BEFORE_PANEL = 5
BLOCKER_XFORM = [[0.6, 0, 0, -0.2], [0, -1, 0, 4.2], [0, 0, -0.6, -3.0], [0, 0, 0, 1]]           # the slab of multi_light_arrays


def panel_emissions(seed=7):
    return np.random.default_rng(seed).uniform(5.0, 40.0, (PANELS, 3)).astype(np.float32)


def chandelier_arrays(base=None):
    """The Cornell box (instance 0 cboxuv.obj, instance 1 the ceiling light, emission 20) with 14 small panels of different
    triangle counts facing down at y = 4.9, each with its own rgb, and a non-emitting blocker slab before panel 5: 17 instances,
    116 triangles, 15 lights with list indices 0 ... 14; from the blocker on the list index is no longer instance - 1.
    `base`: other arrays that end with the ceiling light (the split mesh of test_gpu_materials.py) to hang the panels under."""
    base = geometry.assemble(cbox_models()) if base is None else base
    V = [base.verts]; T = [base.tris]; begin = list(base.inst_tri_begin); X = list(base.inst_xform); E = list(base.inst_emission)
    def add(verts, tris, xform, emission):
        nv = sum(v.shape[0] for v in V)
        V.append(verts); T.append(tris + nv); begin.append(begin[-1] + tris.shape[0])
        X.append(np.asarray(xform, np.float32).reshape(16)); E.append(np.asarray(emission, np.float32))
    for i, ((x, z), e) in enumerate(zip(PANEL_XZ, panel_emissions())):
        if i == BLOCKER_BEFORE_PANEL:
            add(*panel_mesh(1, 1), BLOCKER_XFORM, (0, 0, 0))
        add(*panel_mesh(1 + i % 3, 1 + i % 2), [[0.2, 0, 0, x], [0, -1, 0, 4.9], [0, 0, -0.2, z], [0, 0, 0, 1]], e)
    return geometry.from_arrays(np.concatenate(V), np.concatenate(T), begin, np.stack(X), np.stack(E))


HALL_X, HALL_Z = np.linspace(-2.2, 1.8, 6), np.linspace(-4.8, 0.4, 7)
HALL_PANELS = HALL_X.size * HALL_Z.size
TEXEL_LDS_LIGHTS = 32                                            # ZDR_BGRAD_LDS_LIGHTS = ZDR_LGRAD_LDS_LIGHTS: the texture-space adjoints' table


def hall_arrays():
    """The Cornell box with a 6 x 7 grid of small panels of different triangle counts facing down at y = 4.9 (z-major), each with its
    own rgb: 44 instances, 43 lights with list indices 0 ... 42 (list index = instance - 1) — more than the 32 the adjoints of the
    texture-space bakes sum on chip (zdr_bouncegrad.hip, zdr_bakegrad.hip)."""
    base = geometry.assemble(cbox_models())
    V = [base.verts]; T = [base.tris]; begin = list(base.inst_tri_begin); X = list(base.inst_xform); E = list(base.inst_emission)
    em = np.random.default_rng(7).uniform(5.0, 40.0, (HALL_PANELS, 3)).astype(np.float32)
    for n, (z, x) in enumerate((z, x) for z in HALL_Z for x in HALL_X):
        verts, tris = panel_mesh(1 + n % 3, 1 + n % 2)
        nv = sum(v.shape[0] for v in V)
        V.append(verts); T.append(tris + nv); begin.append(begin[-1] + tris.shape[0])
        X.append(np.array([[0.15, 0, 0, x], [0, -1, 0, 4.9], [0, 0, -0.15, z], [0, 0, 0, 1]], np.float32).reshape(16)); E.append(em[n])
    return geometry.from_arrays(np.concatenate(V), np.concatenate(T), begin, np.stack(X), np.stack(E))


def panel_instance(i, first=2):
    """The instance of panel i (`first`: the instance of panel 0, one past the ceiling light)."""
    return first + i + (1 if i >= BLOCKER_BEFORE_PANEL else 0)


# ----------------------------------------------------------------------------------------------------------- light stage
def rotate_mat(theta, phi, offset):                              # test_lightstage.py:24-45, verbatim in structure
    pitch = np.array([[cos(theta), -sin(theta), 0, 0], [sin(theta), cos(theta), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    yaw = np.array([[cos(phi), 0, -sin(phi), 0], [0, 1, 0, 0], [sin(phi), 0, cos(phi), 0], [0, 0, 0, 1]])
    translate = np.array([[1, 0, 0, offset[0]], [0, 1, 0, offset[1]], [0, 0, 1, offset[2]], [0, 0, 0, 1]])
    m = yaw @ pitch @ translate
    return float4x4(*m.transpose().flatten())


NLIGHT = 30
CAMERA = Camera(fov=50 / 180 * 3.1415926, origin=float3(0, 0.5, 2), target=float3(0, 0, 0), up=float3(0.0, 1.0, 0.0))   # sphere_camera1


def stage_light(i, emission):
    return (f"{ASSETS}/quad.obj", rotate_mat(acos((i + 0.5) / NLIGHT * 2 - 1), pi * 2 * 0.618 * (i + 1), (0, 0, 0)), emission)


def stage30_models(seed=11):
    """The reference light stage at its real size: sphere.obj and all NLIGHT = 30 quads, a distinct rgb from U(20, 80) each."""
    e = np.random.default_rng(seed).uniform(20.0, 80.0, (NLIGHT, 3))
    return [(f"{ASSETS}/sphere.obj", rotate_mat(0, -0.4, (0, 0, 0)), None)] + [stage_light(i, tuple(float(c) for c in e[i])) for i in range(NLIGHT)]


def stage30_arrays():
    return geometry.assemble(stage30_models())


def stage_material():
    from zdr_amd.scenes import fd_material_np
    mat = fd_material_np(64, 3); mat[..., 3] = 0.6 + 0.4 * mat[..., 3]      # roughness 0.72 - 0.96, as test_gpu_lightstage.py
    return mat


# ------------------------------------------------------------------------------------------------- the oracle, by light
def light_rows(e):
    return [k for k in range(e.shape[0]) if (e[k] > 0).any()]


def cotangent_planes(g):
    """g as three cotangents that each read one channel: a channel of the image reads only the same channel of an emission, so
    <plane c, I(row k doubled) - I> is the term of component (k, c)."""
    planes = np.zeros((3,) + g.shape, np.float64)
    for c in range(3):
        planes[c, ..., c] = g[..., c]
    return planes


def oracle_terms(S, p, mat, e0, g, rows=None, factor=2.0):
    """(terms, base): terms[k, c] = <g_c, I(e0 with row k times `factor`) - I(e0)> in float64 from the oracle's forward as it stands,
    for the rows in `rows` (default: every light); every render is checked for dropped samples and the clamp.  Leaves S at e0."""
    e0 = np.ascontiguousarray(e0, np.float32)
    planes = cotangent_planes(g)
    S.set_emissions(e0)
    base, cnt = S.render_forward(p, mat, counters=True)
    assert cnt["nan_samples"] == 0 and float(base[..., :3].max()) < 1e4, (cnt, float(base.max()))
    terms = np.zeros((e0.shape[0], 3), np.float64)
    for k in (light_rows(e0) if rows is None else rows):
        e = e0.copy(); e[k] *= np.float32(factor)
        S.set_emissions(e)
        img, cnt = S.render_forward(p, mat, counters=True)
        assert cnt["nan_samples"] == 0 and float(img[..., :3].max()) < 1e4, (k, cnt, float(img.max()))
        d = img.astype(np.float64) - base.astype(np.float64)
        terms[k] = [(planes[c] * d).sum() for c in range(3)]
    S.set_emissions(e0)
    return terms, base


def shares(terms):
    """Each row's part of sum |term|."""
    a = np.abs(terms).sum(axis=1)
    return a / a.sum()
