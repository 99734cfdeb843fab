"""The "shaft": a scene whose BVH needs more traversal-stack entries than the kernels keep in LDS (ZDR_BVH_LDS_STACK = 12, csrc/scene.h),
and the cases of the six texture-space kernel families on it.  Shared by the host test (tests/test_texel_deep_stack_host.py), the GPU test
(tests/test_gpu_texel_deep_stack.py) and the ``--deep`` switch of the margins tools.

Every other scene these families are tested on has a few dozen triangles: the builder reports 8 stack entries and no ray keeps more than
a handful pending, so neither the one-entry-at-a-time push of BvhAccel::consume (csrc/accel.h) nor its patched pop, nor a launch with
lds_stack = 12 and entries in scratch behind it, is ever run by them.

The scene, in its own frame (y up; all of it is then tilted by TILT_DEG about z, because a normal of exactly +-y sits on make_onb's
branch, which the references call uncertain):
  instance 0, the FLOOR    a panel of 3 x 2 cells over the unit square of the xz plane at y = 0, facing up; it is baked (material slot 0),
                           its atlas shrunk into the texture's interior as tests/texel_lighting_cases.py does;
  instance 1, the TOWER    TOWER right triangles (0, y, 0), (1, y, 0), (0, y, 1) at y = GAP + SPACING i, wound to face down, with a
                           material of ANOTHER size (slot 1): a walk that leaves the floor under the tower lands on its lowest triangle
                           and comes back to the floor.  The tower covers the half x + z < 1 of the square; the other half is the open
                           shaft, whose rays pass along all the boxes of the tower;
  instance 2, the CAP      a 1 x 1 panel RISE above the tower's top, facing down, emitting: shadow segments run the shaft's length.
The variant for the environment-map cases has no cap (``shaft_open_arrays``) or one that emits beside the map (``shaft_arrays``, the same
scene): the map is EC.sky_env, whose bright zenith row sends the map samples up the shaft.

The cases sit in tables of their own, reached through the ``case()`` accessors of tests/texel_bounce_cases.py, texel_lighting_cases.py,
texel_lighting_grad_cases.py, texel_bounce_env_cases.py and texel_project_cases.py: the parametrised tests over those modules' CASES keep
their size.  This module imports none of them at import time (they import it)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):       # (run as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

from zdr_amd import geometry, scenes                             # noqa: E402

LDS_STACK = 12                # ZDR_BVH_LDS_STACK (csrc/scene.h)
TOWER = 512                   # triangles; below that the pending sets stay within LDS_STACK
SPACING = 0.001               # a squat tower: with 0.01 the lobe segments keep at most 10 entries pending
GAP = 0.05                    # from the floor to the lowest triangle; with 0.2 only 15 % of the lobe segments exceed LDS_STACK
RISE = 0.5                    # from the highest triangle to the cap
TILT_DEG = 7.0
CAP_EMISSION = (6.0, 5.0, 4.0)

SHAFT_SLOTS = (0, 1, None)
OPEN_SLOTS = (0, 1)


def tilt():
    c, s = np.cos(np.radians(TILT_DEG)), np.sin(np.radians(TILT_DEG))
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)


def _shaft(cap):
    fv, ft = scenes.panel_mesh(3, 2)
    fv = fv.copy()
    fv[:, 3:5] = np.float32(0.0712) + np.float32(0.8371) * fv[:, 3:5]
    place = np.array([[0.5, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, 0.5, 0.5], [0, 0, 0, 1]], np.float32)      # the 2 x 2 panel onto the unit square
    y = (GAP + SPACING * np.arange(TOWER)).astype(np.float32)
    tv = np.zeros((3 * TOWER, 8), np.float32)
    tv[1::3, 0] = 1.0; tv[2::3, 2] = 1.0
    tv[:, 1] = np.repeat(y, 3)
    tv[:, 3] = np.float32(0.05) + np.float32(0.9) * tv[:, 0]; tv[:, 4] = np.float32(0.05) + np.float32(0.9) * tv[:, 2]
    tv[:, 6] = -1.0                                                   # cross(p1 - p0, p2 - p0) = (0, -1, 0): the underside is the front
    tt = np.arange(3 * TOWER, dtype=np.int32).reshape(TOWER, 3)
    verts, tris, begin = [fv, tv], [ft, tt + fv.shape[0]], [0, ft.shape[0], ft.shape[0] + TOWER]
    T = tilt()
    xf, em = [T @ place, T], [(0, 0, 0), (0, 0, 0)]
    if cap:
        cv, ct = scenes.panel_mesh(1, 1)
        top = float(y[-1]) + RISE
        flip = np.array([[0.5, 0, 0, 0.5], [0, -1, 0, top], [0, 0, -0.5, 0.5], [0, 0, 0, 1]], np.float32)  # faces down
        verts.append(cv); tris.append(ct + fv.shape[0] + tv.shape[0]); begin.append(begin[-1] + ct.shape[0])
        xf.append(T @ flip); em.append(CAP_EMISSION)
    return geometry.from_arrays(np.concatenate(verts), np.concatenate(tris), begin, np.stack([m.reshape(16) for m in xf]), np.array(em, np.float32))


@functools.lru_cache(None)
def shaft_arrays():
    """floor, tower and the emitting cap: 12 + 512 + 2 triangles"""
    return _shaft(True)


@functools.lru_cache(None)
def shaft_open_arrays():
    """floor and tower under the open sky: nothing emits"""
    return _shaft(False)


def sky_env():
    """EC.sky_env: near-uniform with a bright zenith row, tables without MIS compensation"""
    import texel_bounce_env_cases as EC
    return EC.sky_env()


# ---------------------------------------------------------------------------------------------------------------- the tables
# tests/texel_bounce_cases.py: (arrays, slot table, (H, W), second material's size, spp, K, environment, None)
BOUNCE = {
    "shaft_k3": (shaft_arrays, SHAFT_SLOTS, (12, 12), (5, 7), 8, 3, None, None),
    "shaft_pmj02bn_k3": (shaft_arrays, SHAFT_SLOTS, (12, 12), (5, 7), 8, 3, None, None),
    "shaft_k8": (shaft_arrays, SHAFT_SLOTS, (12, 12), (5, 7), 8, 8, None, None),          # the largest record block behind a 12-entry stack
    "shaft_env_k3": (shaft_open_arrays, OPEN_SLOTS, (12, 12), (5, 7), 8, 3, sky_env, None),
    "shaft_env_lit_k3": (shaft_arrays, SHAFT_SLOTS, (12, 12), (5, 7), 8, 3, sky_env, None),  # the map beside a mesh light
}
BOUNCE_SAMPLERS = {"shaft_pmj02bn_k3": (5, 256)}
# tests/texel_bounce_env_cases.py: the cases of BOUNCE that have a map, shared with it as env_k2 is
BOUNCE_ENV = ("shaft_env_k3", "shaft_env_lit_k3")
# tests/texel_lighting_cases.py: (arrays, slot table, (H, W), spp, max_distance, environment); max_distance longer than the shaft
LIGHTING = {
    "shaft_16_ao": (shaft_arrays, SHAFT_SLOTS, (16, 16), 4, 2.0, None),
}
# tests/texel_lighting_grad_cases.py: (arrays, slot table, (H, W), spp, environment)
LIGHTING_GRAD = {
    "shaft_16": (shaft_arrays, SHAFT_SLOTS, (16, 16), 4, None),
    "shaft_env_lit_16": (shaft_arrays, SHAFT_SLOTS, (16, 16), 4, sky_env),
}
# tests/texel_project_cases.py: (points of a case of LIGHTING_POINTS, camera, (width, height)); the camera stands above the open shaft
# and looks down it, so the visibility segments of the texels that are not under the tower run the shaft's length
LIGHTING_POINTS = {
    "shaft_open_16": (shaft_open_arrays, OPEN_SLOTS, (16, 16), 4, None, None),
}
VIEW = {
    "shaft_open_16_above": ("shaft_open_16", "above_shaft", (64, 64)),
}


def _world(p):
    return tuple(float(x) for x in (tilt() @ np.array([*p, 1.0], np.float32))[:3])


def cameras():
    """name: (fov in radians, origin, target, up), in the tilted frame of the scene: the floor fills most of the image"""
    up = tuple(float(x) for x in (tilt() @ np.array([0.0, 0.0, 1.0, 0.0], np.float32))[:3])
    return {"above_shaft": (float(np.radians(40.0)), _world((0.62, 2.2, 0.62)), _world((0.55, 0.0, 0.55)), up)}


# ---------------------------------------------------------------------------------------------------------------- the margins
# float32 reference against float64 reference, never a GPU result; measured by the --deep switch of tools/texel_bounce_margins.py,
# tools/texel_bounce_grad_margins.py and tools/texel_bounce_envgrad_margins.py, by ``python tests/texel_lighting_grad_cases.py --deep`` and by
# ``python tests/texel_deep_cases.py`` (lighting and view), rounded up in the third digit; profiles/texel_deep_stack.txt;
# tests/test_texel_deep_stack_host.py pins them to the measurement
BOUNCE_MARGINS = {
    "shaft_k3": 1.33e-06,
    "shaft_pmj02bn_k3": 1.24e-06,
    "shaft_k8": 1.33e-06,
    "shaft_env_k3": 7.70e-06,
    "shaft_env_lit_k3": 7.20e-06,
}
BOUNCE_GRAD_MARGINS = {
    "shaft_k3": (2.21e-07, 3.46e-08),
    "shaft_pmj02bn_k3": (2.33e-07, 2.28e-08),
    "shaft_k8": (2.48e-07, 4.81e-08),
    "shaft_env_k3": (1.06e-06, 0.0),
    "shaft_env_lit_k3": (1.07e-06, 5.21e-08),
}
BOUNCE_ENVGRAD_MARGINS = {
    "shaft_env_k3": 5.86e-07,
    "shaft_env_lit_k3": 8.76e-07,
}
LIGHTING_MARGINS = {
    "shaft_16_ao": 1.25e-06,
}
LIGHTING_GRAD_MARGINS = {
    "shaft_16": {"emission": 2.59e-06},
    "shaft_env_lit_16": {"emission": 3.02e-06, "env": 7.09e-06},
}
VIEW_MARGINS = {
    "shaft_open_16_above": (1.26e-07, 4.86e-06, 6.34e-06, 3.16e-07, 2.51e-07, 5.29e-07),
}


# ------------------------------------------------------------------------------------------- the references' own segments, walked
class SegmentRecorder:
    """stands in for the OracleScene a reference traces with: hands every query on and keeps its rays, in the order of the calls"""
    def __init__(self, oscene):
        self.oscene, self.calls = oscene, []

    def trace_closest(self, rays):
        self.calls.append((False, np.array(rays, np.float32)))
        return self.oscene.trace_closest(rays)

    def trace_any(self, rays):
        self.calls.append((True, np.array(rays, np.float32)))
        return self.oscene.trace_any(rays)

    def __getattr__(self, name):
        return getattr(self.oscene, name)


@functools.lru_cache(None)
def host_bvh(make):
    """(nodes, plane records, stack entries) of the host builder for a scene: what the kernels walk and what they allocate"""
    import test_bvh_emulation as EM
    from zdr_amd import _native
    nodes, _, isect = EM.build(make(), _native.ACCEL_BVH)
    return nodes, isect, int(EM.STACK)


def pending(make, any_hit, rays):
    """the largest pending set of every ray of positive length (n, 8 {o, tmin, d, tmax}) in the walk's mirror
    (tests/test_bvh_emulation.py, traverse) over the host builder's records"""
    import test_bvh_emulation as EM
    nodes, isect, entries = host_bvh(make)
    EM.STACK = entries                                                # (the mirror asserts its pushes against the tree it walks)
    return np.array([EM.traverse(nodes, isect, r[0:3], r[4:7], np.float32(r[3]), np.float32(r[7]), any_hit)[3] for r in rays if r[7] > r[3]], np.int64)


@functools.lru_cache(None)
def bounce_segments(name):
    """{"lobe": [per vertex index k: pending sets of the closest-hit segments that END in vertex k], "shadow": [per k: those of the
    shadow segments that LEAVE vertex k]} of the float64 reference of a case of BOUNCE, run again with a recorder"""
    import texel_bounce_cases as BC
    import texel_lighting_cases as LC
    make, K = BC.case(name)[0], BC.bounces(name)
    rec = SegmentRecorder(LC.oracle_scene(make))
    BC.run_reference(name, oscene=rec)
    out = {"lobe": [], "shadow": [np.zeros(0, np.int64) for _ in range(K)]}
    for any_hit, rays in rec.calls:
        if any_hit:
            out["shadow"][len(out["lobe"]) - 1] = pending(make, True, rays)
        else:
            out["lobe"].append(pending(make, False, rays))
    assert len(out["lobe"]) == K
    return out


@functools.lru_cache(None)
def lighting_segments(name):
    """{"lobe": the openness segments, "shadow": the light samples' segments} of the float64 reference of a case of LIGHTING"""
    import texel_lighting_cases as LC
    import texel_lighting_ref as LR
    make, _, _, spp, max_distance, env = LC.case(name)
    rec = SegmentRecorder(LC.oracle_scene(make))
    LR.texel_lighting_ref(make(), rec, LC.points(name), spp=spp, seed=LC.SEED, max_distance=max_distance, env=env() if env else None)
    (a0, openness), (a1, shadow) = rec.calls
    assert a0 and a1
    return {"lobe": pending(make, True, openness), "shadow": pending(make, True, shadow)}


@functools.lru_cache(None)
def lighting_grad_segments(name):
    """{"shadow": the light samples' segments} of the float64 reference of a case of LIGHTING_GRAD"""
    import texel_lighting_cases as LC
    import texel_lighting_grad_cases as GC
    import texel_lighting_grad_ref as LG
    make, _, _, spp, env = GC.case(name)
    rec = SegmentRecorder(LC.oracle_scene(make))
    LG.texel_lighting_grad_ref(make(), rec, GC.points(name), GC.cotangent(name), env=env() if env else None, spp=spp, seed=GC.SEED)
    assert len(rec.calls) == 1 and rec.calls[0][0]
    return {"shadow": pending(make, True, rec.calls[0][1])}


@functools.lru_cache(None)
def view_segments(name):
    """{"shadow": the visibility segments from the texels to the camera} of the float64 reference of a case of VIEW"""
    import texel_lighting_cases as LC
    import texel_project_cases as PC
    import texel_project_ref as PR
    pts, cam, res = PC.case(name)
    make = LC.case(pts)[0]
    rec = SegmentRecorder(LC.oracle_scene(make))
    PR.view_ref(PC.points(name), PC.CAMERAS[cam], res, rec, np.float64)
    assert rec.calls and rec.calls[0][0]
    return {"shadow": pending(make, True, rec.calls[0][1])}       # (the later calls test the same segments for uncertainty)


def share(p):
    """(segments that keep more than LDS_STACK entries pending, segments, the largest pending set)"""
    return int((p > LDS_STACK).sum()), int(p.size), int(p.max()) if p.size else 0


def _fmt(label, p):
    n, of, top = share(p)
    return f"{label} {n} of {of} ({n / max(of, 1):.2f}) exceed {LDS_STACK}, largest {top}"


def share_lines():
    """the measured shares of profiles/texel_deep_stack.txt: no GPU involved"""
    lines = ["host builder (zdr_debug_build_accel) and the walk's mirror (tests/test_bvh_emulation.py) on the float64 references' own segments: "
             f"segments whose pending set exceeds the {LDS_STACK} entries the kernels keep in LDS"]
    for make in (shaft_arrays, shaft_open_arrays):
        nodes, isect, entries = host_bvh(make)
        lines.append(f"  {make.__name__}: {isect.shape[0]} triangles, {nodes.shape[0]} nodes, stack entries {entries}")
    for name in BOUNCE:
        s = bounce_segments(name)
        lines.append(f"  {name:20s} " + _fmt("closest-hit segments of vertex 0:", s["lobe"][0]) + "; "
                     + _fmt("of later vertices:", np.concatenate(s["lobe"][1:])) + "; " + _fmt("shadow segments from vertices k >= 1:", np.concatenate(s["shadow"][1:]))
                     + "; " + _fmt("from vertex 0:", s["shadow"][0]))
    for name in LIGHTING:
        s = lighting_segments(name)
        lines.append(f"  {name:20s} " + _fmt("openness segments:", s["lobe"]) + "; " + _fmt("shadow segments:", s["shadow"]))
    for name in LIGHTING_GRAD:
        lines.append(f"  {name:20s} " + _fmt("shadow segments:", lighting_grad_segments(name)["shadow"]))
    for name in VIEW:
        lines.append(f"  {name:20s} " + _fmt("visibility segments:", view_segments(name)["shadow"]))
    return lines


def margin_lines():
    """the float32 references of the lighting and view cases against float64 (the bounce families and the lighting adjoint: the --deep
    switch of their tools)"""
    import texel_lighting_cases as LC
    import texel_project_cases as PC
    lines = ["", "float32 reference against the float64 reference (no GPU involved): texel_lighting, largest absolute error of the irradiance over the compared texels"]
    for name in LIGHTING:
        ref, r32 = LC.reference(name), LC.reference(name, "float32")
        keep = LC.compared(name)
        e = float(np.abs(r32["data"][..., :3].astype(np.float64) - ref["data"][..., :3])[keep].max())
        opn = int((r32["data"][..., 3][keep].astype(np.float32) != ref["data"][..., 3][keep].astype(np.float32)).sum())
        lines.append(f"  {name:20s} reached {int(LC.reached(name).sum())}  uncertain {int((LC.reached(name) & ref['uncertain']).sum())}  lit {int((ref['lit'] > 0).sum())}  "
                     f"largest irradiance {float(ref['data'][..., :3].max()):.4e}  error {e:.3e}  openness differs {opn}")
    lines += ["", "texel_view: the classes of the case and the largest absolute error per channel over the compared texels"]
    for name in VIEW:
        c = PC.classes(name)
        ref, r32 = PC.reference(name), PC.reference(name, "float32")
        d = np.abs(r32["data"].astype(np.float64) - ref["data"])[PC.compared(name)]
        e = tuple(float(d[:, ch].max()) for ch in range(1, 7))
        lines.append(f"  {name:20s} reached {c[0]}  behind {c[1]}  outside {c[2]}  visible {c[3]}  occluded {c[4]}  seen from behind {c[5]}  uncertain {c[6]}")
        lines.append("    " + "  ".join(f"{ch} {x:.3e}" for ch, x in zip(PC.CHANNELS, e)))
    return lines


if __name__ == "__main__":      # the host part of profiles/texel_deep_stack.txt that no margins tool writes
    import texel_deep_cases as DC   # (the module the case modules share, not this script's copy of it)
    print("\n".join(DC.share_lines() + DC.margin_lines()))
