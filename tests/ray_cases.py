"""Rays that random draws never produce, and a float64 reference that judges EVERY one of them (tests/test_ray_cases_host.py on the
CPU mirror of the walk, tests/test_gpu_ray_cases.py on the kernels).

Scenes: the Cornell box (brute force and BVH), terrain_arrays(n=14), and a TOWER — n right triangles (0,0,z) (1,0,z) (0,1,z) at
z = 0.01 k under a 1 x 1 cap at z = 42: a ray along z at (0.9, 0.9) is inside every box and outside every triangle, enters every node
and keeps more entries pending than the LDS part of the traversal stack holds (4096 triangles: 18 entries; the control of 64 triangles
stays within 8, inside the LDS part of either layout — with the cap in the tree a tower of 512 reaches 15, one of 128 reaches 12).

Reference: pairs64 is Moeller-Trumbore in float64 over the float32 corners the scene holds, written from the definition; it shares
nothing with oracle/ or with the plane-form records of the kernels.

Admissibility instead of a budget of disagreements.  A ray / triangle pair is DECIDED when the float64 facts leave no room:
  hit    min(u, v, 1 - u - v) > BARY_MARGIN and t further than the t bound inside (tmin, tmax)
  miss   one of them beyond its margin on the failing side (or the ray parallel to the plane, non-finite, or tmin >= tmax)
and OPEN otherwise.  An answer is admissible when no decided fact contradicts it (check_closest / check_any).  Nothing is averaged and
no share of the rays is exempt.
  t bound      |t - t64| <= 1e-5 |t64| + 5e-6 (x max|coordinate| / 10 for the tower): the bound of tests/test_gpu_trace.py, check_closest.
               Its derivation — the numerator n.p0 - n.o cancels to an ABSOLUTE error of an ulp of the coordinates — divides by n.d
               with unit n and d, i.e. it presumes a ray that is not grazing.  A pair with 0 < |n.d| < C0 has both margins scaled by
               C0 / |n.d|, and the families keep only rays whose grazing pairs are decided misses even so (drop_grazing): every hit
               the tests judge is held to the bound as stated.
  BARY_MARGIN  4 x the largest |u32 - u64|, |v32 - v64| of the float32 mirror of the records (test_bvh_emulation.tri_tuv) over the
               non-grazing pairs of all families (measure_margin; profiles/ray_cases_margins.txt): the factor covers the one ulp of
               v_rcp_f32 and the fma contraction that the mirror lacks.  It comes from the mirror and the reference, never from
               what a GPU returned.  The error of a barycentric grows with its size (the hit point is o + t d, and u is linear in
               it), so the largest errors sit on pairs whose point lies 50 triangle widths beside the triangle (|u| ~ 90: 4.5e-5),
               where no margin below 1/2 can change the verdict.  The margin is therefore taken from the pairs with
               |u64|, |v64| <= NEAR = 2, the only ones it can decide, and the host test asserts that the error over ALL pairs
               stays below 1e-3 — far from the 1/2 by which a pair beyond NEAR is outside.

PER-PAIR BOUNDS (Case(..., per_pair=True): the scenes of tests/geometry_cases.py, away from the origin, of mixed scale, transformed).
Both rules above are rules of thumb for a scene of unit-sized triangles around the origin; the plane form's error follows the RECORD:
t = (N.w - N.o) / (N.d) cancels numbers of the size |N.w| + sum |N_k o_k|, and u = U.p + U.w numbers of the size |coordinate| / edge.
In this mode every pair carries bounds of its own, computed in float64 from the float32 record the builder made (pair_bounds); a pair
is a decided hit / miss when t is outside its bound of (tmin, tmax) and u, v, w are outside theirs, no grazing rule, no share exempt.
The constants are operation counts of tri_test / pair_test / hit_barycentrics (csrc/accel.h), to first order in g = 2^-24 (the unit
roundoff of float32, half an ulp; the reference's own error, 2^-53 of the same sums, is a 5e8-th of it):
  t    |t - t64| <= g (CA (|N.w| + sum |N_k o_k|) + |t64| CD sum |N_k d_k|) / |N.d| + g CM |t64|
       CA = 4  each N_k: 1 rounding of the float64 record to float32; the term N.x o.x then passes a product and two fma: 3 more (N.y: 2,
               N.z: 1).  N.w: its rounding to float32, 1.  The subtraction is counted under CM.
       CD = 4  the same four for N.d.  Where the ray grazes the plane the sum cancels and the error of the denominator is an ulp of
               sum |N_k d_k|, not of |N.d|: a shorthand "4 |t64|" for the relative part is this term with the ratio sum |N_k d_k| / |N.d| taken as 1,
               its least value.  A pair with 2 CD g sum |N_k d_k| >= |N.d| has no bound (the sign of the float32 denominator is open).
       CM = 4  the subtraction N.w - no: 1; v_rcp_f32: one ulp = 2 g; the product with it: 1.
  u    |u - u64| <= g (C1 (sum |U_k p_k| + |U.w|) + C2 sum |U_k| (|o_k| + 2 |d_k t|)) + |U.d| x the t bound, v likewise
       C1 = 5  U_k: the record's rounding, 1; U.x p.x then a product, two more terms and the sum with U.w: 4.  (U.w: 2.)
       C2 = 1  on a sum that already counts p = o + t d both ways: one fma (|p_k| <= |o_k| + |d_k t|) or a product and a sum.
       the last term: the float32 point is o + t32 d, the float64 one o + t64 d.
  w    1 - (u + v) (tri_test), or a record of its own (the third edge of the brute-force walk's single triangles, the outer edges of a
       quad's partner; a rotated slot's u is the input triangle's w): |w - w64| <= Bu + Bv + g (5 + |u + v| + |w|) =: M covers both,
       and M >= Bu, Bv is the margin all three barycentrics are decided with — it holds for a slot the brute-force builder rotated.
       A barycentric REPORTED for a rotated slot is 1 - u' - v' of two computed ones: check_closest(rotated=True) allows 2 M + 4 g.
  quads  the brute-force walk tests the second triangle of a merged quad with the plane of the first (Case.brute_planes): Ref(brute=True)
       bounds such a pair with the first triangle's N and adds the distance between the two planes, over |n.d|, to its t bound.
The mirror (mirror32, IEEE division instead of v_rcp_f32, no fma) stays within these on every pair of every case
(tests/test_geometry_cases_host.py, profiles/geometry_cases_margins.txt); nothing here comes from what a GPU returned.
"""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # (run as a script: python tests/ray_cases.py prints the table of profiles/ray_cases_margins.txt)
    sys.path.insert(0, ROOT)

import test_bvh_emulation as emu
from zdr_amd import _native, geometry
from zdr_amd.scenes import cbox_models, random_rays, terrain_arrays

T_REL, T_ABS = 1e-5, 5e-6
C0 = 0.1                       # |n.d| (unit n, unit d) below which a pair counts as grazing
BARY_MARGIN = 1.9e-5           # 4 x 4.71e-6 measured (profiles/ray_cases_margins.txt), rounded up; test_ray_cases_host.py holds it to the measurement
NEAR = 2.0                     # the margin is measured on pairs with |u64|, |v64| <= NEAR (see BARY_MARGIN above)
G32 = 2.0 ** -24                # unit roundoff of float32
CA, CD, CM, C1, C2 = 4.0, 4.0, 4.0, 5.0, 1.0      # per-pair bounds: the operation counts of the module docstring
MISS, OPEN, HIT = 0, 1, 2
FAMILIES = ("axis", "in_plane", "features", "intervals", "tower", "nonfinite")


# ------------------------------------------------------------------------------------------------ scenes
def tower_arrays(n):
    z = (0.01 * np.arange(n)).astype(np.float32)
    v = np.zeros((3 * n + 4, 8), np.float32)
    v[:, 7] = 1.0
    v[1:3 * n:3, 0] = 1.0; v[2:3 * n:3, 1] = 1.0
    v[:3 * n, 2] = np.repeat(z, 3)
    v[3 * n:, :3] = [[0, 0, 42], [1, 0, 42], [1, 1, 42], [0, 1, 42]]
    t = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    cap = np.array([[1, 2, 3], [0, 1, 3]], np.int32) + 3 * n      # split along x + y = 1: (0.9, 0.9) is inside the first, (0.2, 0.2) inside the second
    return geometry.from_arrays(v, np.concatenate([t, cap]), [0, n, n + 2], None, [[0, 0, 0], [1, 1, 1]])      # (the cap is the scene's light, as the terrain's quad)


class Case:
    def __init__(self, name, A, accels, per_pair=False):
        self.name, self.A, self.accels, self.per_pair = name, A, accels, per_pair
        if per_pair:               # world corners as the scene holds them: M v in float32, left to right (zdr_api.cpp, xform_point)
            self.tri = np.ascontiguousarray(emu.world_triangles(A))
        else:
            assert (A.inst_xform == np.eye(4, dtype=np.float32).reshape(16)).all()      # world corners = the float32 vertices as they are
            self.tri = np.ascontiguousarray(A.verts[A.tris][:, :, :3])
        self.t_abs = T_ABS * max(1.0, float(np.abs(self.tri).max()) / 10.0)
        self.lo, self.hi = self.tri.reshape(-1, 3).min(0).astype(np.float64), self.tri.reshape(-1, 3).max(0).astype(np.float64)
        self.tri_inst = np.repeat(np.arange(A.ninst), np.diff(A.inst_tri_begin))

    def tri_of(self, inst_prim):
        """(n, 2) {inst, prim} as the kernels report them -> index of the input triangle, -1 for a miss"""
        ip = np.asarray(inst_prim)
        hit = ip[:, 0] >= 0
        return np.where(hit, self.A.inst_tri_begin[np.where(hit, ip[:, 0], 0)] + ip[:, 1], -1)

    @functools.cached_property
    def rec_in(self):
        """(T, 12) float64: the builder's float32 plane records {N, U, V} in INPUT triangle order (unrotated corners: the BVH builder's)"""
        _, order, isect, _ = self.records
        out = np.empty(isect.shape, np.float64)
        out[order] = isect
        return out

    @functools.cached_property
    def brute_planes(self):
        """(rec_in with the plane N of a quad's SECOND triangle replaced by the first one's, (T,) how far the second triangle's corners lie
        off that plane): the brute-force walk tests a quad — two triangles the builder found in one plane to 5e-7 of the quad's size,
        zdr_api.cpp, find_quads — with ONE plane, so t of the second triangle is the float32 answer for the plane of the first.  Inside the
        second triangle the two planes are apart by at most the largest distance at its corners (linear in the point): in t that is
        dev / |n.d|, n the unit normal; it is added to the t bound of these triangles, for the brute-force walk only."""
        import test_brute_quads as bq
        nq, order, isect = bq.build(self.tri)
        rec, dev = self.rec_in.copy(), np.zeros(len(self.tri))
        for q in range(nq):
            a, b = order[2 * q], order[2 * q + 1]
            N = isect[2 * q, 0:4].astype(np.float64)
            rec[a, 0:4] = rec[b, 0:4] = N
            dev[b] = np.abs(self.tri[b].astype(np.float64) @ N[:3] - N[3]).max() / np.linalg.norm(N[:3])
        return rec, dev

    @functools.cached_property
    def records(self):
        """(nodes, order, isect, stack_entries) of the host's BVH builder: what the kernels walk"""
        nodes, order, isect = emu.build(self.A, _native.ACCEL_BVH)
        return nodes, order, isect, emu.STACK


@functools.lru_cache(None)
def case(name):
    if name == "cbox":
        return Case(name, geometry.assemble(cbox_models()), ("brute", "bvh"))
    if name == "terrain":
        return Case(name, terrain_arrays(n=14), ("bvh",))
    if name == "tower":
        return Case(name, tower_arrays(4096), ("bvh",))
    if name == "tower64":
        return Case(name, tower_arrays(64), ("bvh",))
    raise KeyError(name)


# --------------------------------------------------------------------------------------------- reference
def pairs64(tri, rays):
    """float64 Moeller-Trumbore of every ray (n, 8 {o, tmin, d, tmax}) with every triangle (T, 3, 3) -> t, u, v (u, v: the
    barycentrics of corners 1 and 2) and nd = n.d with n the unit normal cross(e1, e2) / |.|, each (n, T)."""
    tri = np.asarray(tri, np.float64); rays = np.asarray(rays, np.float64)
    p0, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    o, d = rays[:, None, 0:3], rays[:, None, 4:7]
    cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    dot = lambda a, b: a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]
    with np.errstate(all="ignore"):
        pv = cross(d, e2)
        det = dot(e1, pv)
        inv = 1.0 / det
        tv = o - p0
        u = dot(tv, pv) * inv
        qv = cross(tv, e1)
        v = dot(d, qv) * inv
        t = dot(e2, qv) * inv
        n = cross(e1, e2)
        nd = -det / np.sqrt(dot(n, n))                # e1 . (d x e2) = -d . (e1 x e2)
    return t, u, v, nd


def closest64(tri, rays):
    """-> (nearest triangle hit with tmin < t < tmax or -1, its t or inf, (t, u, v, nd) of every pair): the definition, no margins"""
    t, u, v, nd = pairs64(tri, rays)
    rays = np.asarray(rays, np.float64)
    with np.errstate(invalid="ignore"):
        hit = (nd != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > rays[:, None, 3]) & (t < rays[:, None, 7])
    tt = np.where(hit, t, np.inf)
    k = tt.argmin(1)
    best = tt[np.arange(len(k)), k]
    return np.where(np.isfinite(best), k, -1), best, (t, u, v, nd)


def any64(tri, rays):
    k, _, pairs = closest64(tri, rays)
    return k >= 0, pairs


def pair_bounds(rec, r, t, u, v, dev=None):
    """Per-pair error bounds of the plane form (module docstring) -> (Bt, Bu, Bv, M), each (n, T) float64.  rec: (T, 12) float64 holding
    the float32 records; r: (n, 8) float64 rays; t, u, v: the float64 facts of pairs64; dev: (T,) distance by which the plane of rec
    is not the triangle's own (Case.brute_planes).  Infinite where nothing can be bounded."""
    o, d = r[:, None, 0:3], r[:, None, 4:7]
    N, Nw = rec[None, :, 0:3], np.abs(rec[None, :, 3])
    with np.errstate(all="ignore"):
        nd = np.abs((N * d).sum(-1)); snd = np.abs(N * d).sum(-1); sno = np.abs(N * o).sum(-1)
        at = np.abs(t)
        Bt = G32 * (CA * (Nw + sno) + at * CD * snd) / nd + G32 * CM * at
        if dev is not None:
            Bt = Bt + dev[None, :] * np.sqrt((N * N).sum(-1)) / nd
        Bt = np.where(2.0 * CD * G32 * snd >= nd, np.inf, Bt)
        tt = np.where(np.isfinite(t), t, 0.0)[..., None]
        p = np.abs(o + tt * d); q = np.abs(o) + 2.0 * np.abs(tt * d)
        out = []
        for a in (4, 8):
            U = rec[None, :, a:a + 3]
            s1 = (np.abs(U) * p).sum(-1) + np.abs(rec[None, :, a + 3]); s2 = (np.abs(U) * q).sum(-1)
            out.append(G32 * (C1 * s1 + C2 * s2) + np.abs((U * d).sum(-1)) * Bt)
        Bu, Bv = out
        M = Bu + Bv + G32 * (5.0 + np.abs(u + v) + np.abs(1.0 - u - v))
        bad = ~np.isfinite(Bt) | ~np.isfinite(M)
        Bt, Bu, Bv, M = (np.where(bad, np.inf, x) for x in (Bt, Bu, Bv, M))
    return Bt, Bu, Bv, M


class Ref:
    """The float64 facts of a batch of rays against a scene, pair by pair."""

    def __init__(self, c, rays, margin=None, chunk=256, brute=False):
        """brute (per-pair bounds only): judge the brute-force walk, whose quads test their second triangle with the plane of the first"""
        margin = BARY_MARGIN if margin is None else margin
        rays = np.ascontiguousarray(rays, np.float32)
        n, T = rays.shape[0], c.tri.shape[0]
        self.case, self.rays = c, rays
        self.t = np.empty((n, T)); self.u = np.empty((n, T), np.float32); self.v = np.empty((n, T), np.float32); self.c = np.empty((n, T), np.float32)   # (u, v, c kept in float32: 6e-8 of a barycentric, against a margin of 2e-5)
        self.state = np.empty((n, T), np.int8)
        if c.per_pair:
            self.B, self.bu, self.bv, self.m = (np.empty((n, T), np.float32) for _ in range(4))     # (kept in float32, rounded UP: a bound may only grow)
            rec, dev = c.brute_planes if brute else (c.rec_in, None)
            flat =(rec[:, 0:3] == 0).all(1)                     # a zero-area triangle: N = 0, t = 0 x inf = NaN, never hit
        for a in range(0, n, chunk):
            r = rays[a:a + chunk].astype(np.float64)
            t, u, v, nd = pairs64(c.tri, r)
            tmin, tmax = r[:, None, 3], r[:, None, 7]
            with np.errstate(all="ignore"):
                cc = np.abs(nd) / np.sqrt((r[:, 4:7] ** 2).sum(1))[:, None]
                k = np.where(cc < C0, C0 / cc, 1.0)                      # grazing pairs: both margins grow with 1 / |n.d|
                inside = np.minimum(np.minimum(u, v), 1.0 - u - v)
                if c.per_pair:
                    B, Bu, Bv, mb = pair_bounds(rec, r, t, u, v, dev)
                    up = lambda x: np.nextafter(x.astype(np.float32), np.float32(np.inf))
                    s = slice(a, a + chunk)
                    self.B[s], self.bu[s], self.bv[s], self.m[s] = up(B), up(Bu), up(Bv), up(mb)
                    zero = flat[None, :] | ((rec[None, :, 0:3] * r[:, None, 4:7]) == 0).all(-1)      # every product of N.d exactly zero: t is infinite or NaN
                    hit = ~zero & (inside > mb) & (t - tmin > B) & (tmax - t > B)
                    miss = zero | (inside < -mb) | (t < tmin - B) | (t > tmax + B)
                else:
                    B = (T_REL * np.abs(t) + c.t_abs) * k
                    mb = margin * k
                    hit = (nd != 0) & (inside > mb) & (t - tmin > B) & (tmax - t > B)
                    miss = (nd == 0) | (inside < -mb) | (t < tmin - B) | (t > tmax + B)
            dead = ~np.isfinite(r[:, 0:3]).all(1) | ~np.isfinite(r[:, 4:7]).all(1) | (r[:, 4:7] == 0).all(1) | ~(r[:, 3] < r[:, 7])
            miss |= dead[:, None]                     # a ray of NaNs or infinities, without a direction or with an empty interval hits nothing
            st = np.where(miss, MISS, np.where(hit, HIT, OPEN)).astype(np.int8)
            s = slice(a, a + chunk)
            self.t[s], self.u[s], self.v[s], self.c[s], self.state[s] = t, u, v, cc, st
        self.dec_t = np.where(self.state == HIT, self.t, np.inf).min(1)          # the nearest decided hit
        if c.per_pair:                                                           # ... and the largest float32 t the nearest decided hit may come out with
            self.dec_hi = np.where(self.state == HIT, self.t + self.B, np.inf).min(1)
        live_t = np.where(self.state != MISS, self.t, np.inf)
        first = live_t.argmin(1)
        rows = np.arange(n)
        self.has_open = (self.state == OPEN).any(1)
        self.decided_miss = (self.state == MISS).all(1)
        self.decided_hit = (self.state[rows, first] == HIT) & ~self.decided_miss   # the nearest pair that is not a miss is a decided hit
        self.grazing = ((self.c < C0) & (self.state != MISS)).any(1)               # a grazing pair that may count: the ray is not kept

    def check_closest(self, tri_idx, t, uv=None, rows=None, rotated=False):
        """-> [(answer, reason, ray)] for the answers that a decided fact contradicts.  rows: the ray of this Ref each answer belongs to
        (default: answer i to ray i).  rotated (per-pair bounds only): the barycentrics come from slots the brute-force builder may have
        rotated (module docstring)."""
        tri_idx = np.asarray(tri_idx); t = np.asarray(t, np.float64)
        rows = np.arange(self.rays.shape[0]) if rows is None else np.asarray(rows)
        assert len(tri_idx) == len(t) == len(rows)
        k = np.where(tri_idx >= 0, tri_idx, 0)
        st, t64, dec = self.state[rows, k], self.t[rows, k], self.dec_t[rows]
        u64, v64 = self.u[rows, k], self.v[rows, k]
        with np.errstate(all="ignore"):
            if self.case.per_pair:
                b = self.B[rows, k].astype(np.float64)
                m2 = 2.0 * self.m[rows, k].astype(np.float64) + 4.0 * G32
                bu, bv = (m2, m2) if rotated else (self.bu[rows, k], self.bv[rows, k])
                nearer = self.dec_hi[rows] < t64 - b
            else:
                b = T_REL * np.abs(t64) + self.case.t_abs
                bu = bv = BARY_MARGIN
                nearer = dec < t64 - b
            hit = tri_idx >= 0
            why = np.zeros(len(t), np.int8)
            why[~hit & np.isfinite(dec)] = 1
            why[hit & (why == 0) & (st == MISS)] = 2
            why[hit & (why == 0) & ~(np.abs(t - t64) <= b)] = 3
            why[hit & (why == 0) & nearer] = 4
            if uv is not None:
                why[hit & (why == 0) & (st == HIT) & ~((np.abs(uv[:, 0] - u64) <= bu) & (np.abs(uv[:, 1] - v64) <= bv))] = 5
        text = {1: "miss, but a triangle is hit for certain at t = {dec:.9g}",
                2: "hit on triangle {k}, which is missed for certain (t64 {t64:.9g}, u {u:.3g}, v {v:.3g})",
                3: "t = {t:.9g} on triangle {k}, float64 {t64:.9g}: off by more than {b:.3g}",
                4: "hit on triangle {k} at {t64:.9g}, but another is hit for certain at {dec:.9g}",
                5: "barycentrics {uv} on triangle {k}, float64 ({u:.9g}, {v:.9g})"}
        return [(int(i), text[why[i]].format(dec=dec[i], k=tri_idx[i], t64=t64[i], u=u64[i], v=v64[i], t=t[i], b=b[i], uv=None if uv is None else uv[i].tolist()),
                 self.rays[rows[i]].tolist()) for i in np.nonzero(why)[0]]

    def check_any(self, occluded, rows=None):
        occ = np.asarray(occluded) != 0
        rows = np.arange(self.rays.shape[0]) if rows is None else np.asarray(rows)
        may, must = (self.state != MISS).any(1)[rows], (self.state == HIT).any(1)[rows]
        return [(int(i), "occluded, but every triangle is missed for certain" if occ[i] else "not occluded, but a triangle is hit for certain", self.rays[rows[i]].tolist())
                for i in np.nonzero((occ & ~may) | (~occ & must))[0]]

    def take(self, keep):
        r = object.__new__(Ref)
        r.case = self.case
        for name in ("rays", "t", "u", "v", "c", "state", "dec_t", "has_open", "decided_miss", "decided_hit", "grazing") + (("B", "bu", "bv", "m", "dec_hi") if self.case.per_pair else ()):
            setattr(r, name, getattr(self, name)[keep])
        return r


def mirror32(c, rays):
    """(t, u, v) of test_bvh_emulation.tri_tuv — the float32 mirror of the kernels' plane-form test on the builder's records — for
    every ray against every triangle, columns in INPUT triangle order like pairs64."""
    _, order, isect, _ = c.records
    q = [isect[None, :, k] for k in range(12)]
    rays = np.ascontiguousarray(rays, np.float32)
    out = [np.empty((rays.shape[0], isect.shape[0]), np.float32) for _ in range(3)]
    for a in range(0, rays.shape[0], 512):
        r = rays[a:a + 512]
        tuv = emu.tri_tuv(q, [r[:, None, k] for k in range(3)], [r[:, None, 4 + k] for k in range(3)])
        for dst, src in zip(out, tuv):
            dst[a:a + 512][:, order] = src
    return out


def ref_of_distinct(c, rays):
    """(Ref of the distinct rays among `rays`, the row of it each ray belongs to): a wave composition repeats a few rays many times"""
    rays = np.ascontiguousarray(rays, np.float32)
    uniq, inv = np.unique(rays.view(np.uint32), axis=0, return_inverse=True)      # by bit pattern: NaNs and the two zeros stay apart
    return Ref(c, np.ascontiguousarray(uniq).view(np.float32)), inv.reshape(-1)


# ---------------------------------------------------------------------------------------------- families
def mk(o, d, tmin=0.0, tmax=1e30):
    o = np.asarray(o, np.float64).reshape(-1, 3); d = np.asarray(d, np.float64).reshape(-1, 3)
    n = max(o.shape[0], d.shape[0])
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = o; r[:, 3] = tmin; r[:, 4:7] = d; r[:, 7] = tmax
    return r


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def axis_rays(c, seed):
    rng = np.random.default_rng(seed)
    dirs = []
    for a in range(3):                                   # two components exactly zero, in every sign combination
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    d = np.zeros(3); d[a] = s; d[(a + 1) % 3] = z1; d[(a + 2) % 3] = z2
                    dirs.append(d)
    for a in range(3):                                   # one component exactly zero
        for z in (0.0, -0.0):
            for s1 in (1.0, -1.0):
                for s2 in (1.0, -1.0):
                    d = np.zeros(3); d[a] = z
                    x = unit([s1 * rng.uniform(0.3, 1.0), s2 * rng.uniform(0.3, 1.0)])
                    d[(a + 1) % 3], d[(a + 2) % 3] = x
                    dirs.append(d)
    span = c.hi - c.lo
    verts = c.tri.reshape(-1, 3).astype(np.float64)
    generic = lambda: rng.uniform(c.lo - 0.1 * span, c.hi + 0.1 * span)
    o, d = [], []
    for dd in dirs:
        for _ in range(6):
            o.append(generic()); d.append(dd)
        for plane in (c.lo, c.hi):                       # exactly on a plane of the scene's box
            k = rng.integers(3); p = generic(); p[k] = plane[k]; o.append(p); d.append(dd)
        for _ in range(2):                               # one coordinate exactly a vertex's (a plane of its leaf's box)
            k = rng.integers(3); p = generic(); p[k] = verts[rng.integers(len(verts))][k]; o.append(p); d.append(dd)
        t = c.tri[rng.integers(len(c.tri))].astype(np.float64)   # in a triangle's plane, beside the triangle
        o.append(t[0] + 1.5 * (t[1] - t[0]) + 1.5 * (t[2] - t[0])); d.append(dd)
    return mk(o, d)


def aligned_triangles(c):
    """(triangle, axis) whose three corners share a coordinate exactly: its plane record has two zero components"""
    return [(i, k) for i, t in enumerate(c.tri) for k in range(3) if t[0, k] == t[1, k] == t[2, k]]


def in_plane_rays(c, seed):
    rng = np.random.default_rng(seed)
    o, d = [], []
    def fan(k, x, lo, hi, count):                        # rays inside the plane coordinate k = x, from points of the rectangle [lo, hi] in the other two
        for _ in range(count):
            p = np.zeros(3); p[k] = x
            p[(k + 1) % 3], p[(k + 2) % 3] = rng.uniform(lo, hi)
            phi = rng.uniform(0, 2 * np.pi)
            dd = np.zeros(3); dd[(k + 1) % 3], dd[(k + 2) % 3] = np.cos(phi), np.sin(phi)
            o.append(p); d.append(dd)
    other = lambda k: [(k + 1) % 3, (k + 2) % 3]
    if c.name == "cbox":
        for i, k in aligned_triangles(c):                # n.d = 0 exactly: the right wall
            t = c.tri[i].astype(np.float64)
            lo, hi = t[:, other(k)].min(0), t[:, other(k)].max(0)
            fan(k, t[0, k], lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), 60)
        # the planes y = const of the faces that are level to within the rounding of the mesh (box tops, light, floor, ceiling): d.y = 0
        n = np.cross(c.tri[:, 1] - c.tri[:, 0], c.tri[:, 2] - c.tri[:, 0]).astype(np.float64)
        level = np.abs(unit(n)[:, 1]) > 1 - 1e-5
        for i in np.nonzero(level)[0]:
            fan(1, float(c.tri[i, 0, 1]), np.array([c.lo[2], c.lo[0]]), np.array([c.hi[2], c.hi[0]]), 40)
    else:                                                # the tower: every triangle is parallel to every other
        for i in (0, 1, len(c.tri) // 2, len(c.tri) - 3):
            fan(2, float(c.tri[i, 0, 2]), np.array([-0.5, -0.5]), np.array([1.5, 1.5]), 50)
    return mk(o, d)


def features_of(c):
    """(point, size, adjacent triangles, kind) of every corner, every edge midpoint and three points of every diagonal of a merged quad"""
    T = c.tri.astype(np.float64)
    key = lambda p: tuple(np.asarray(p, np.float32).tolist())
    corners, edges = {}, {}
    for i, t in enumerate(T):
        for a in range(3):
            corners.setdefault(key(t[a]), []).append(i)
            ka, kb = sorted((key(t[a]), key(t[(a + 1) % 3])))
            edges.setdefault((ka, kb), []).append(i)
    out = []
    for p, adj in corners.items():
        t = T[adj[0]]
        size = min(np.linalg.norm(t[a] - t[(a + 1) % 3]) for a in range(3))
        out.append((np.array(p, np.float64), size, adj, "corner"))
    n = unit(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    for (a, b), adj in edges.items():
        a, b = np.array(a, np.float64), np.array(b, np.float64)
        out.append(((a + b) / 2, np.linalg.norm(b - a), adj, "edge"))
        if len(adj) == 2 and abs(n[adj[0]] @ n[adj[1]]) > 1 - 1e-6:          # coplanar neighbours: the brute-force walk merges them into a quad
            for f in (0.25, 0.5, 0.75):
                out.append((a + f * (b - a), np.linalg.norm(b - a), adj, "diagonal"))
    return out


def features_rays(c, seed):
    """eleven rays per feature: the exact one (tag 0), two bounded copies of it (tag 4) and eight (tags 3 and 2) aimed 1e-3 and 1e-2 of the feature's size to either side, along two directions of the
    first adjacent triangle's plane that are generic to its edges.  The origin sees every adjacent triangle at |n.d| >= 0.3."""
    rng = np.random.default_rng(seed)
    T = c.tri.astype(np.float64)
    nrm = unit(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    o, d, tags, lim = [], [], [], []
    for p, size, adj, _ in features_of(c):
        for _ in range(200):
            w = unit(rng.standard_normal(3))
            if np.abs(nrm[adj] @ w).min() >= 0.3:
                break
        else:
            continue
        org = p + rng.uniform(1.0, 2.5) * w
        t = T[adj[0]]
        e = unit(t[1] - t[0]); f = np.cross(nrm[adj[0]], e)
        ang = 0.37
        g1, g2 = np.cos(ang) * e + np.sin(ang) * f, -np.sin(ang) * e + np.cos(ang) * f
        o.append(org); d.append(unit(p - org)); tags.append(0)
        dist = np.linalg.norm(p - org)
        for tmin, tmax in ((0.0, 0.999 * dist), (1.001 * dist, 1e30)):       # the exact ray once more, ending just short of the feature and starting just behind it
            o.append(org); d.append(unit(p - org)); tags.append(4); lim.append((tmin, tmax))
        for g in (g1, g2):
            for k, eps in ((3, 1e-3), (3, -1e-3), (2, 1e-2), (2, -1e-2)):
                o.append(org); d.append(unit(p + eps * size * g - org)); tags.append(k)
    rays, tags = mk(o, d), np.array(tags)
    rays[tags == 4, 3] = [a for a, _ in lim]; rays[tags == 4, 7] = [b for _, b in lim]
    return rays, tags


def generic_hits(c, seed, count, cmin=0.3):
    """random rays whose nearest triangle is hit for certain, not at a grazing angle -> (rays, t*)"""
    span = c.hi - c.lo
    rays = random_rays(40 * count, c.lo - 0.05 * span, c.hi + 0.05 * span, seed=seed)
    ref = Ref(c, rays)
    first = np.where(ref.state == HIT, ref.t, np.inf).argmin(1)
    ok = ref.decided_hit & ~ref.has_open & (ref.c[np.arange(len(rays)), first] >= cmin) & (ref.dec_t > 0.05)
    pick = np.nonzero(ok)[0][:count]
    assert len(pick) == count
    return rays[pick], ref.dec_t[pick]


def intervals_rays(c, seed):
    rays, ts = generic_hits(c, seed, 60)
    out = []
    for r, t in zip(rays, ts):
        for tmin, tmax in ((0, t * (1 + 1e-3)), (0, t * (1 - 1e-3)), (t * (1 - 1e-3), 1e30), (t * (1 + 1e-3), 1e30), (t * (1 - 1e-3), t * (1 + 1e-3)),
                           (1, 1), (2, 1), (t * (1 + 1e-3), t * (1 - 1e-3)), (0, 0), (0, -1), (-1, 0), (0, np.inf), (t * (1 + 1e-3), np.inf)):
            q = r.copy(); q[3] = tmin; q[7] = tmax
            out.append(q)
    return np.array(out, np.float32)


def tower_long_ray(c, reverse=False):
    """the ray along z at (0.9, 0.9): inside every box of the tower, outside every triangle, into the cap at the far end"""
    return mk([0.9, 0.9, -1.0], [0, 0, 1])[0] if not reverse else mk([0.9, 0.9, 41.5], [0, 0, -1])[0]


def tower_rays(c, seed):
    n = len(c.tri) - 2
    mid = 0.01 * (n // 2 - 0.5)                          # half way up, between two triangles
    out = [tower_long_ray(c), tower_long_ray(c, True)]
    outside = [(0.9, 0.9), (0.6, 0.6), (0.95, 0.7), (0.75, 0.95), (0.55, 0.5), (0.98, 0.98), (0.3, 0.8), (0.85, 0.3)]
    inside = [(0.2, 0.2), (0.1, 0.6), (0.6, 0.1), (0.4, 0.4)]
    for x, y in outside + inside:
        for oz, s in ((-1.0, 1.0), (41.5, -1.0), (43.5, -1.0), (mid, 1.0), (mid, -1.0)):
            end = 0.01 * ((2 * n // 3 if s > 0 else n // 3) + 0.5)              # between two triangles, ahead of every origin
            for tx, ty in ((0, 0), (1e-4, 1e-4), (-1e-4, 1e-4), (1e-4, -1e-4), (-1e-4, -1e-4)):
                out.append(mk([x, y, oz], [tx, ty, s])[0])
                out.append(mk([x, y, oz], [tx, ty, s], 0.0, abs(end - oz))[0])   # ends inside the tower
    return np.array(out, np.float32)


def nonfinite_rays(c, seed):
    rays, _ = generic_hits(c, seed, 3)
    out = []
    for r in rays:
        for k in (0, 1, 2, 4, 5, 6):
            for x in (np.nan, np.inf, -np.inf):
                q = r.copy(); q[k] = x; out.append(q)
        for z in (0.0, -0.0):
            q = r.copy(); q[4:7] = z; out.append(q)
    return np.array(out, np.float32)


class Batch:
    def __init__(self, family, scene, rays, tags=None):
        self.family, self.scene, self.case = family, scene, case(scene)
        ref = Ref(self.case, rays)
        keep = ~ref.grazing                              # drop_grazing: see the module docstring
        self.dropped = int((~keep).sum())
        if family == "axis":                             # origins ON box planes and vertex coordinates are wanted, origins ON a triangle are not: those
            keep &= ~ref.has_open                        # rays would have their answer left open, and this family is to pin the walk down
        self.ref = ref.take(keep)
        self.rays = self.ref.rays
        self.tags = None if tags is None else tags[keep]

    def __repr__(self):
        return f"{self.family}/{self.scene}[{len(self.rays)}]"


PLAN = (("axis", ("cbox", "terrain", "tower")), ("in_plane", ("cbox", "tower")), ("features", ("cbox", "terrain")),
        ("intervals", ("cbox", "terrain")), ("tower", ("tower", "tower64")), ("nonfinite", ("cbox", "terrain", "tower")))
MAKERS = {"axis": axis_rays, "in_plane": in_plane_rays, "features": features_rays, "intervals": intervals_rays, "tower": tower_rays, "nonfinite": nonfinite_rays}


@functools.lru_cache(None)
def batches():
    """every family on every scene it is traced on, with its float64 facts: computed once per process, never modified"""
    out = []
    for fi, (family, scenes) in enumerate(PLAN):
        for si, scene in enumerate(scenes):
            made = MAKERS[family](case(scene), 1000 + 10 * fi + si)
            rays, tags = made if isinstance(made, tuple) else (made, None)
            out.append(Batch(family, scene, rays, tags))
    return tuple(out)


def measure_margin():
    """largest |u32 - u64|, |v32 - v64| of the float32 mirror over the non-grazing pairs of every batch -> {batch: (over the pairs with
    |u64|, |v64| <= NEAR, over all pairs)}"""
    out = {}
    for b in batches():
        if b.family == "nonfinite":
            continue
        _, u32, v32 = mirror32(b.case, b.rays)
        with np.errstate(all="ignore"):
            ok = (b.ref.c >= C0) & np.isfinite(b.ref.u) & np.isfinite(b.ref.v) & np.isfinite(u32) & np.isfinite(v32)
            near = ok & (np.abs(b.ref.u) <= NEAR) & (np.abs(b.ref.v) <= NEAR)
            e = np.maximum(np.abs(u32 - b.ref.u), np.abs(v32 - b.ref.v))
        out[repr(b)] = (float(e[near].max()) if near.any() else 0.0, float(e[ok].max()) if ok.any() else 0.0)   # (the tower's in-plane rays are parallel to every triangle)
    return out


def family_stats():
    """{family: (rays, share with an open pair, share of decided hits, share of decided misses, rays dropped as grazing)}"""
    out = {}
    for family in FAMILIES:
        bs = [b for b in batches() if b.family == family]
        n = sum(len(b.rays) for b in bs)
        out[family] = (n, sum(int(b.ref.has_open.sum()) for b in bs) / n, sum(int(b.ref.decided_hit.sum()) for b in bs) / n,
                       sum(int(b.ref.decided_miss.sum()) for b in bs) / n, sum(b.dropped for b in bs))
    return out


if __name__ == "__main__":      # the table of profiles/ray_cases_margins.txt
    import time
    t0 = time.time()
    m = measure_margin()
    for k, v in m.items():
        print(f"{k:28s} max |bary32 - bary64|: {v[0]:.3e} over pairs with |u64|, |v64| <= {NEAR:g}, {v[1]:.3e} over all")
    big = max(v[0] for v in m.values())
    print(f"largest {big:.3e}  x 4 = {4 * big:.3e}  BARY_MARGIN = {BARY_MARGIN:.3e}   (C0 = {C0}, float32 mirror against float64, no GPU involved)")
    for k, v in family_stats().items():
        print(f"{k:10s} rays {v[0]:5d}  open {v[1]:.4f}  decided hits {v[2]:.3f}  decided misses {v[3]:.3f}  dropped as grazing {v[4]}")
    print(f"{time.time() - t0:.1f} s")
