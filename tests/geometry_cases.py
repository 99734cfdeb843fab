"""Geometry like a mesh a user might bring, for the ray queries: away from the origin, of mixed scale, degenerate, transformed — judged pair
by pair with the per-pair bounds of tests/ray_cases.py (Case(per_pair=True): see its module docstring for the bounds and their operation
counts).  tests/test_geometry_cases_host.py runs the float32 mirrors on them, tests/test_gpu_geometry_cases.py the kernels.

Every case is small (at most 802 triangles — the 20 x 20 grid —, 2,000 rays), has a last instance that emits (a scene can be made of it), and
gets the same rays: 1,500 AIMED at points inside non-degenerate triangles (all three barycentrics >= 0.1, |n.d| >= 0.3 against the aimed
triangle) from origins 1e-3 ... 1 scene diagonals away (log-uniform; a tenth of them end at twice the distance, a tenth at half of it),
and 500 RANDOM ones from the scene's box grown by half a diagonal, which mostly miss.  No ray is dropped: whatever the reference cannot
decide stays in as an open ray, and the host test asserts that two thirds of every case's rays are decided by the reference alone.

  cbox+1000     the Cornell box translated by (1000, 1000, 1000) in float32                      brute, bvh
  cbox+4096x    ... by (4096, 0, 0)                                                              brute, bvh
  cbox*1e4      ... scaled by 1e4                                                                brute, bvh
  soup          400 triangles, sizes log-uniform in 1e-3 ... 3, centres in [-3, 3]^3            bvh
  soup+300      the same, translated by (300, 300, 300)                                          bvh
  soup60        the first 60 of them                                                             brute
  ground        two triangles of a 2e4-wide plane y = 0 under 300 triangles of size 0.01 ... 0.3 within 5 units of the origin    bvh
  needles       300 triangles of aspect 4000:1 ... 8000:1                                        bvh
  duplicates    100 triangles, each four times                                                   bvh
  concentric    200 triangles of sizes 0.05 ... 3 whose boxes share one centre (the builder's centroid: every SAH bin but one is empty)   bvh
  flat          a 20 x 20 grid exactly in y = 0 (800 triangles; its light is two more in the same plane)    bvh
  degenerate    140 soup triangles, 30 point triangles (three equal corners) and 30 collinear ones whose third corner is the
                float32-representable midpoint of the other two: the area is exactly zero, N = 0, and no answer may name them       bvh
  transformed   the Cornell box through an instance transform with a rotation, a non-uniform scale and a mirror (det < 0); the
                reference works on the world corners M v                                         brute, bvh
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script: python tests/geometry_cases.py prints profiles/geometry_cases_margins.txt)
    sys.path.insert(0, ROOT)

import ray_cases as rc
from zdr_amd import geometry
from zdr_amd.scenes import cbox_models

CASES = ("cbox+1000", "cbox+4096x", "cbox*1e4", "soup", "soup+300", "soup60", "ground", "needles", "duplicates", "concentric", "flat",
         "degenerate", "transformed")
BOTH = ("cbox+1000", "cbox+4096x", "cbox*1e4", "transformed")
N_AIMED, N_RANDOM = 1500, 500
CAP = 2.0 / 3.0                # share of a case's rays the reference must decide by itself


# ------------------------------------------------------------------------------------------------ scenes
def arrays_of(tris, nlight):
    """(T, 3, 3) corners -> SceneArrays of two instances: the last nlight triangles emit"""
    tris = np.asarray(tris, np.float32)
    T = tris.shape[0]
    v = np.zeros((3 * T, 8), np.float32)
    v[:, 0:3] = tris.reshape(-1, 3); v[:, 6] = 1.0
    return geometry.from_arrays(v, np.arange(3 * T, dtype=np.int32).reshape(T, 3), [0, T - nlight, T], None, [[0, 0, 0], [10, 10, 10]])


def moved_cbox(scale=1.0, shift=(0.0, 0.0, 0.0)):
    A = geometry.assemble(cbox_models())
    A.verts[:, 0:3] = (A.verts[:, 0:3].astype(np.float64) * scale + np.asarray(shift, np.float64)).astype(np.float32)
    return A


def rotation(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def transformed_cbox():
    A = geometry.assemble(cbox_models())
    M = np.eye(4)
    M[:3, :3] = rotation((1, 2, 3), 0.7) @ np.diag([-1.3, 0.7, 1.1])         # det < 0: the instance is mirrored
    M[:3, 3] = (2.0, -1.0, 3.0)
    A.inst_xform[:] = M.astype(np.float32).reshape(16)
    return A


def shaped(rng, centre, size):
    """a triangle of two edges of length size and 0.5 ... 1 size, 40 ... 140 degrees apart, in a random plane"""
    e1 = rc.unit(rng.standard_normal(3))
    f = rc.unit(np.cross(e1, rng.standard_normal(3)))
    phi = rng.uniform(np.radians(40), np.radians(140))
    e2 = rng.uniform(0.5, 1.0) * (np.cos(phi) * e1 + np.sin(phi) * f)
    p0 = centre - size * (e1 + e2) / 3
    return np.stack([p0, p0 + size * e1, p0 + size * e2])


def soup_tris(n, seed, lo_size, hi_size, half=3.0):
    rng = np.random.default_rng(seed)
    return np.stack([shaped(rng, rng.uniform(-half, half, 3), np.exp(rng.uniform(np.log(lo_size), np.log(hi_size)))) for _ in range(n)])


def ground_tris():
    W = 1.0e4
    plane = np.array([[[-W, 0, -W], [W, 0, W], [W, 0, -W]], [[-W, 0, -W], [-W, 0, W], [W, 0, W]]])
    small = soup_tris(300, 31, 0.01, 0.3, half=5.0)
    small[:, :, 1] = np.abs(small[:, :, 1]) + 0.4                            # above the plane
    return np.concatenate([plane, small])


def needle_tris():
    rng = np.random.default_rng(32)
    out = []
    for _ in range(300):
        c, e = rng.uniform(-3, 3, 3), rc.unit(rng.standard_normal(3))
        f = rc.unit(np.cross(e, rng.standard_normal(3)))
        L = rng.uniform(1.0, 3.0); w = L / rng.uniform(4000.0, 8000.0)
        out.append(np.stack([c - 0.5 * L * e, c + 0.5 * L * e, c + w * f]))
    return np.stack(out)


def concentric_tris():
    rng = np.random.default_rng(33)
    out = []
    for _ in range(200):
        t = shaped(rng, np.zeros(3), np.exp(rng.uniform(np.log(0.05), np.log(3.0)))).astype(np.float32).astype(np.float64)
        out.append(t - 0.5 * (t.min(0) + t.max(0)))                          # the centre of its box to the origin (up to the rounding to float32)
    return np.stack(out)


def flat_tris():
    g = np.linspace(-3.0, 3.0, 21)
    out = []
    for i in range(20):
        for j in range(20):
            a, b, c, d = (g[i], 0, g[j]), (g[i + 1], 0, g[j]), (g[i + 1], 0, g[j + 1]), (g[i], 0, g[j + 1])
            out += [[a, c, b], [a, d, c]]
    out += [[(4, 0, 4), (5, 0, 5), (5, 0, 4)], [(4, 0, 4), (4, 0, 5), (5, 0, 5)]]    # the light, in the same plane
    return np.array(out, np.float64)


def degenerate_tris():
    """30 points, 30 collinear triangles, 140 soup triangles (the last four emit).  Collinear: corners a, b = a + 2 h, a + h with a and h float32
    numbers of few mantissa bits, so that all three are float32 numbers and the midpoint is exact — cross(e1, e2) = 0 in any arithmetic."""
    rng = np.random.default_rng(34)
    soup = soup_tris(140, 35, 1e-3, 3.0)
    q = lambda x, step: np.round(np.asarray(x) / step) * step               # multiples of a power of two: a few mantissa bits
    pts = [np.tile(q(rng.uniform(-3, 3, 3), 2.0 ** -10).astype(np.float32), (3, 1)) for _ in range(30)]
    col = []
    for _ in range(30):
        a, h = q(rng.uniform(-3, 3, 3), 2.0 ** -8), q(rng.uniform(-1, 1, 3), 2.0 ** -8)
        col.append(np.stack([a, a + 2 * h, a + h]))
    tris = np.concatenate([np.stack(pts).astype(np.float64), np.stack(col), soup])
    t32 = tris.astype(np.float32)
    assert (t32[:60].astype(np.float64) == tris[:60]).all()
    n = np.cross(t32[:60, 1] - t32[:60, 0], t32[:60, 2] - t32[:60, 0])       # in float32, as in any other arithmetic
    assert (n == 0).all()
    return tris


@functools.lru_cache(None)
def case(name):
    accels = ("brute", "bvh") if name in BOTH else ("brute",) if name == "soup60" else ("bvh",)
    if name == "cbox+1000": A = moved_cbox(shift=(1000, 1000, 1000))
    elif name == "cbox+4096x": A = moved_cbox(shift=(4096, 0, 0))
    elif name == "cbox*1e4": A = moved_cbox(scale=1e4)
    elif name == "soup": A = arrays_of(soup_tris(400, 30, 1e-3, 3.0), 4)
    elif name == "soup+300": A = arrays_of(soup_tris(400, 30, 1e-3, 3.0) + 300.0, 4)
    elif name == "soup60": A = arrays_of(soup_tris(400, 30, 1e-3, 3.0)[:60], 4)
    elif name == "ground": A = arrays_of(ground_tris(), 4)
    elif name == "needles": A = arrays_of(needle_tris(), 4)
    elif name == "duplicates": A = arrays_of(np.repeat(soup_tris(100, 36, 0.1, 1.0), 4, axis=0), 4)
    elif name == "concentric": A = arrays_of(concentric_tris(), 4)
    elif name == "flat": A = arrays_of(flat_tris(), 2)
    elif name == "degenerate": A = arrays_of(degenerate_tris(), 4)
    elif name == "transformed": A = transformed_cbox()
    else: raise KeyError(name)
    return rc.Case(name, A, accels, per_pair=True)


def zero_area(c):
    """the triangles whose float32 corners span no area"""
    t = c.tri.astype(np.float64)
    return (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) == 0).all(1)


# -------------------------------------------------------------------------------------------------- rays
def make_rays(c, seed):
    rng = np.random.default_rng(seed)
    T = c.tri.astype(np.float64)
    good = np.nonzero(~zero_area(c))[0]
    nrm = np.zeros_like(T[:, 0]); nrm[good] = rc.unit(np.cross(T[good, 1] - T[good, 0], T[good, 2] - T[good, 0]))
    diag = float(np.linalg.norm(c.hi - c.lo))
    o, d, lim = [], [], []
    for k in range(N_AIMED):
        i = good[rng.integers(len(good))]
        b = 0.1 + 0.7 * rng.dirichlet((1.0, 1.0, 1.0))                      # all three >= 0.1
        P = b[0] * T[i, 0] + b[1] * T[i, 1] + b[2] * T[i, 2]
        while True:
            w = rc.unit(rng.standard_normal(3))
            if abs(nrm[i] @ w) >= 0.3:
                break
        dist = diag * 10.0 ** rng.uniform(-3.0, 0.0)
        org = (P + dist * w).astype(np.float32).astype(np.float64)
        o.append(org); d.append(rc.unit(P - org))
        lim.append((0.0, 1e30) if k % 10 > 1 else (0.0, 2.0 * dist) if k % 10 == 0 else (0.0, 0.5 * dist))
    rays = rc.mk(o, d)
    rays[:, 3] = [a for a, _ in lim]; rays[:, 7] = [b for _, b in lim]
    ro = rng.uniform(c.lo - 0.5 * diag, c.hi + 0.5 * diag, (N_RANDOM, 3))
    return np.concatenate([rays, rc.mk(ro, rc.unit(rng.standard_normal((N_RANDOM, 3))))])


class Batch:
    def __init__(self, name, seed):
        self.name, self.case = name, case(name)
        self.rays = make_rays(self.case, seed)
        self.ref = rc.Ref(self.case, self.rays)
        self.decided = self.ref.decided_hit | self.ref.decided_miss

    @functools.cached_property
    def ref_brute(self):
        """the same facts with the bounds of the brute-force walk (ray_cases.Case.brute_planes)"""
        return rc.Ref(self.case, self.rays, brute=True)

    def ref_of(self, accel):
        return self.ref_brute if accel == "brute" else self.ref

    def __repr__(self):
        return f"{self.name}[{len(self.rays)}]"


@functools.lru_cache(None)
def batch(name):
    """the case's rays with their float64 facts: computed once per process, never modified"""
    return Batch(name, 2000 + CASES.index(name))


# ------------------------------------------------------------------------------------ surface interaction
def interaction_facts(ref, rows, k, rotated=False):
    """What surface_interact (csrc/scene.h) must report for a hit of ray rows[i] on triangle k[i] -> (p64, bound on |p - p64| per
    coordinate, the float64 unit normal of the world triangle, bound on |ng - n64| per component).
      p   the kernel interpolates the corners with the barycentrics it computed: p = p0 w0 + p1 u + p2 v, w0 = 1 - u - v.  Against the float64
          point o + t64 d = p0 + u64 e1 + v64 e2 that is e1 du + e2 dv — with du, dv inside the pair's own bounds (ray_cases.pair_bounds), whose
          last term is |U.d| x the t bound: the point moves along d by the error of t — plus the roundings of w0 and of the five operations of the
          interpolation, 8 g max |corner coordinate|.  rotated (slots the brute-force builder rotated): the corners are taken in another order and
          both barycentrics carry the symmetric margin M: 2 M x the widest edge, per coordinate.
      ng  normalize(cross(p1 - p0, p2 - p0)) in float32 on the host (zdr_api.cpp, world_records): each edge one rounding, each component of the
          cross product two products and a difference of size <= 2 |ea| |eb|, the normalisation a sum, a root and a quotient:
          g (16 L^2 / |e1 x e2| + 4) with L the longest edge.  The sign is the winding of the WORLD corners."""
    c = ref.case
    T = c.tri.astype(np.float64)[k]; r = ref.rays[rows].astype(np.float64)
    p64 = r[:, 0:3] + ref.t[rows, k][:, None] * r[:, 4:7]
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    big = 8.0 * rc.G32 * np.abs(T).max(1) + 2.0 ** -48 * (np.abs(r[:, 0:3]) + np.abs(ref.t[rows, k][:, None] * r[:, 4:7]))     # (the second term: the float64 point's own rounding, where every corner has an exact 0)
    if rotated:
        m = 2.0 * ref.m[rows, k].astype(np.float64) + 4.0 * rc.G32
        pb = 2.0 * m[:, None] * np.maximum(np.maximum(np.abs(e1), np.abs(e2)), np.abs(e2 - e1)) + big
    else:
        pb = np.abs(e1) * ref.bu[rows, k].astype(np.float64)[:, None] + np.abs(e2) * ref.bv[rows, k].astype(np.float64)[:, None] + big
    n = np.cross(e1, e2); area2 = np.linalg.norm(n, axis=1)
    L2 = np.maximum(np.maximum((e1 * e1).sum(1), (e2 * e2).sum(1)), ((e2 - e1) ** 2).sum(1))
    return p64, pb, n / area2[:, None], rc.G32 * (16.0 * L2 / area2 + 4.0)


def ratio(err, bound):
    """err / bound; 0 where both are zero (a coordinate every corner has as exactly 0 is reproduced exactly)"""
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / bound)


def mirror_interaction(b):
    """the float32 mirror's barycentrics of every decided hit, interpolated as surface_interact does, in float32 -> worst |p - p64| / bound"""
    _, u32, v32 = rc.mirror32(b.case, b.rays)
    rows = np.nonzero(b.ref.decided_hit)[0]
    k = np.where(b.ref.state == rc.HIT, b.ref.t, np.inf).argmin(1)[rows]
    u, v = u32[rows, k][:, None], v32[rows, k][:, None]
    T = b.case.tri[k]
    f = np.float32
    p32 = T[:, 0] * (f(1.0) - u - v) + T[:, 1] * u + T[:, 2] * v
    assert p32.dtype == np.float32
    p64, pb, _, _ = interaction_facts(b.ref, rows, k)
    return float(ratio(np.abs(p32.astype(np.float64) - p64), pb).max()), len(rows)


# ------------------------------------------------------------------------------------------ measurements
def mirror_ratios(b):
    """The float32 mirror of the records (ray_cases.mirror32) against the per-pair bounds, over EVERY pair with a finite bound ->
    (worst |dt| / Bt, worst |du| / Bu, worst |dv| / Bv, worst |du| or |dv| on pairs with |u|, |v| <= NEAR)"""
    t32, u32, v32 = rc.mirror32(b.case, b.rays)
    r = b.ref
    with np.errstate(all="ignore"):
        okt = np.isfinite(r.B) & np.isfinite(r.t) & np.isfinite(t32)
        rt = np.where(okt, np.abs(t32.astype(np.float64) - r.t) / r.B, 0.0)
        oku = okt & np.isfinite(r.bu) & np.isfinite(r.bv) & np.isfinite(r.u) & np.isfinite(u32) & np.isfinite(v32)
        du, dv = np.abs(u32.astype(np.float64) - r.u), np.abs(v32.astype(np.float64) - r.v)      # (r.u, r.v are float32 roundings of float64: 6e-8 of them, inside C1)
        ru, rv = np.where(oku, du / r.bu, 0.0), np.where(oku, dv / r.bv, 0.0)
        near = oku & (np.abs(r.u) <= rc.NEAR) & (np.abs(r.v) <= rc.NEAR)
        e = float(np.maximum(du, dv)[near].max()) if near.any() else 0.0
    return float(rt.max()), float(ru.max()), float(rv.max()), e


def old_rule_ratio(b):
    """worst |dt| of the mirror over the pairs with |n.d| > 0.1 and |u|, |v| <= 2, divided by the fixed rule
    1e-5 |t64| + 5e-6 max(1, max |coordinate| / 10), and by the per-pair bound"""
    t32, _, _ = rc.mirror32(b.case, b.rays)
    r = b.ref
    with np.errstate(all="ignore"):
        ok = (r.c > 0.1) & (np.abs(r.u) <= 2) & (np.abs(r.v) <= 2) & np.isfinite(r.t) & np.isfinite(t32) & np.isfinite(r.B)
        dt = np.abs(t32.astype(np.float64) - r.t)
        old = rc.T_REL * np.abs(r.t) + b.case.t_abs
    return float((dt / old)[ok].max()), float((dt / r.B)[ok].max())


def table():
    out = ["per-pair bounds of tests/ray_cases.py against the float32 mirror of the plane records (IEEE float32 on the CPU; no GPU involved)",
           f"CA = {rc.CA:g}  CD = {rc.CD:g}  CM = {rc.CM:g}  C1 = {rc.C1:g}  C2 = {rc.C2:g}   (operation counts: tests/ray_cases.py)", "",
           f"{'case':12s} {'tris':>5s} {'rays':>5s} {'decided':>8s} {'hits':>6s} {'misses':>7s} {'|dt|/Bt':>8s} {'|du|/Bu':>8s} {'|dv|/Bv':>8s} {'worst |du|,|dv| near':>21s}"]
    c0 = rc.Case("cbox", geometry.assemble(cbox_models()), ("brute", "bvh"), per_pair=True)      # the Cornell box at the origin, for comparison only
    b0 = object.__new__(Batch); b0.name, b0.case = "cbox", c0
    b0.rays = make_rays(c0, 1999); b0.ref = rc.Ref(c0, b0.rays); b0.decided = b0.ref.decided_hit | b0.ref.decided_miss
    rows = []
    for b in [b0] + [batch(name) for name in CASES]:
        name = b.name
        rt, ru, rv, e = mirror_ratios(b)
        rows.append((name, old_rule_ratio(b)))
        out.append(f"{name:12s} {len(b.case.tri):5d} {len(b.rays):5d} {b.decided.mean():8.3f} {b.ref.decided_hit.mean():6.3f} {b.ref.decided_miss.mean():7.3f} "
                   f"{rt:8.3f} {ru:8.3f} {rv:8.3f} {e:21.3e}")
    out += ["", "surface interaction: |p - p64| of the mirror's barycentrics, interpolated in float32, over its bound (interaction_facts), worst per case",
            "  ".join(f"{name} {mirror_interaction(batch(name))[0]:.3f}" for name in ("cbox+1000", "transformed", "soup+300", "ground"))]
    out += ["", "the fixed rule |dt| <= 1e-5 |t64| + 5e-6 max(1, max |coordinate| / 10) against the per-pair bound: worst ratio of the mirror over the pairs",
            "with |n.d| > 0.1 and |u|, |v| <= 2 (the Cornell box at the origin for comparison)", f"{'case':12s} {'fixed rule':>10s} {'per-pair':>9s}"]
    for name, (a, n) in rows:
        out.append(f"{name:12s} {a:10.2f} {n:9.3f}")
    return "\n".join(out)


if __name__ == "__main__":
    print(table())
