"""Reference of the texture-space feature buffers (include/zdr.h, zdr_scene_texel_aovs) in NumPy, from ``SceneArrays``: the instance
transforms and the inverse-transpose for the normals are applied as the host builder applies them (zdr_amd/csrc/zdr_api.cpp), then the
triangles of one material are rasterised into its texture by the semantics of the header.  Any float dtype: float64 is the truth the GPU
tests compare with, float32 follows the kernels' operations one by one and measures what float32 alone costs.  Besides the buffers it
returns the winners (the global triangle index g per texel, for coverage and for reach) and, for the comparison of the discrete
channels, the texels whose decision lies within ``tol`` pixels of flipping.  A helper, not a test; tests/test_texel_ref_host.py pins it."""
import numpy as np

EMPTY = -1
UNCERTAIN_TOL = 1e-4      # pixels


def world_triangles(arrays, dtype):
    """(P, Nn, UV, area, inst, g0): world corners (ntris, 3, 3), transformed normals (ntris, 3, 3), the float32 UVs (ntris, 3, 2), world
    areas, instance of every triangle — everything in input order, so the row index IS the global index g."""
    V = arrays.verts
    T = arrays.tris
    nt = T.shape[0]
    P = np.zeros((nt, 3, 3), dtype); Nn = np.zeros((nt, 3, 3), dtype); inst = np.zeros(nt, np.int64)
    for i in range(arrays.ninst):
        b, e = int(arrays.inst_tri_begin[i]), int(arrays.inst_tri_begin[i + 1])
        m = arrays.inst_xform[i].astype(dtype)
        a_, b_, c_, d_, e_, f_, g_, h_, i_ = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
        c00, c01, c02 = e_ * i_ - f_ * h_, f_ * g_ - d_ * i_, d_ * h_ - e_ * g_
        c10, c11, c12 = c_ * h_ - b_ * i_, a_ * i_ - c_ * g_, b_ * g_ - a_ * h_
        c20, c21, c22 = b_ * f_ - c_ * e_, c_ * d_ - a_ * f_, a_ * e_ - b_ * d_
        inv = dtype(1.0) / (a_ * c00 + b_ * c01 + c_ * c02)
        nm = [c00 * inv, c01 * inv, c02 * inv, c10 * inv, c11 * inv, c12 * inv, c20 * inv, c21 * inv, c22 * inv]
        v = V[T[b:e]].astype(dtype)                        # (n, 3, 8)
        x, y, z = v[..., 0], v[..., 1], v[..., 2]
        for r in range(3):
            P[b:e, :, r] = m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3]
            Nn[b:e, :, r] = nm[3 * r] * v[..., 5] + nm[3 * r + 1] * v[..., 6] + nm[3 * r + 2] * v[..., 7]
        inst[b:e] = i
    UV = V[T][..., 3:5].astype(np.float32)
    c = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).astype(dtype)
    area = (np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]).astype(dtype)) / dtype(2.0)).astype(dtype)
    return P, Nn, UV, area, inst


def pixel_space(UV, H, W, dtype):
    """(ntris, 3, 2): X = u (W - 1), Y = (1 - v) (H - 1) in ``dtype`` (float32: the product the kernels form)."""
    uv = UV.astype(dtype)
    out = np.empty(uv.shape, dtype)
    out[..., 0] = uv[..., 0] * dtype(W - 1)
    out[..., 1] = (dtype(1.0) - uv[..., 1]) * dtype(H - 1)
    return out


class Edge:
    """Side P -> Q with its endpoints in canonical (lexicographic) order, as the kernels store it."""
    def __init__(self, px, py, qx, qy, dtype):
        sw = (qx < px) or (qx == px and qy < py)
        self.ax, self.ay = (qx, qy) if sw else (px, py)
        bx, by = (px, py) if sw else (qx, qy)
        self.dx, self.dy = dtype(bx - self.ax), dtype(by - self.ay)
        self.sg = dtype(-1.0 if sw else 1.0)
        self.len = np.sqrt(np.float64(self.dx) ** 2 + np.float64(self.dy) ** 2)

    def __call__(self, x, y):
        return self.sg * (self.dx * (y - self.ay) - self.dy * (x - self.ax))


class Setup:
    def __init__(self, q, dtype):
        (x0, y0), (x1, y1), (x2, y2) = q
        self.e = (Edge(x1, y1, x2, y2, dtype), Edge(x2, y2, x0, y0, dtype), Edge(x0, y0, x1, y1, dtype))
        self.area2 = self.e[0](x0, y0)
        self.degenerate = not (self.area2 > 0 or self.area2 < 0)
        self.sgn = dtype(-1.0 if self.area2 < 0 else 1.0)
        self.abs2 = abs(self.area2)
        self.minx, self.maxx, self.miny, self.maxy = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)


def classify_points(S, x, y, dtype, tol=None):
    """(coverage, reach[, uncertain]) of the lattice points (x, y) (arrays of ``dtype``) for one triangle."""
    one = dtype(1.0)
    gaps = [S.minx - (x + one), (x - one) - S.maxx, S.miny - (y + one), (y - one) - S.maxy]     # > 0: separated along a box axis
    box = (gaps[0] <= 0) & (gaps[1] <= 0) & (gaps[2] <= 0) & (gaps[3] <= 0)
    sep = np.maximum(np.maximum(gaps[0], gaps[1]), np.maximum(gaps[2], gaps[3])).astype(np.float64)
    if S.degenerate:
        cov = np.zeros(x.shape, bool)
        unc = np.abs(sep) < tol if tol is not None else None
        return cov, box, unc
    c = [S.sgn * e(x, y) for e in S.e]
    cov = (c[0] >= 0) & (c[1] >= 0) & (c[2] >= 0)
    meets = box
    for e, ci in zip(S.e, c):
        r = abs(e.dx) + abs(e.dy)
        meets = meets & ~(ci + r < 0) & ~(ci - r > S.abs2)
        if tol is not None:
            sep = np.maximum(sep, np.maximum(-(ci + r), (ci - r) - S.abs2).astype(np.float64) / e.len)
    reach = cov | meets
    unc = None
    if tol is not None:
        inside = np.minimum(np.minimum(c[0] / S.e[0].len, c[1] / S.e[1].len), c[2] / S.e[2].len)   # the smallest distance to a side's line
        unc = (np.abs(inside) < tol) | (~cov & (np.abs(sep) < tol))
    return cov, reach, unc


def closest_barycentrics(q, x, y, dtype):
    """Barycentrics of the closest point of the closed triangle ``q`` to (x, y): the nearest of the closest points of its three sides."""
    n = x.shape[0]
    w = np.zeros((n, 3), dtype)
    best = np.full(n, np.inf, dtype)
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        ax, ay, bx, by = q[a][0], q[a][1], q[b][0], q[b][1]
        dx, dy = bx - ax, by - ay
        l2 = dx * dx + dy * dy
        t = ((x - ax) * dx + (y - ay) * dy) / l2 if l2 > 0 else np.zeros(n, dtype)
        t = np.minimum(np.maximum(t, dtype(0.0)), dtype(1.0)).astype(dtype)
        qx, qy = ax + t * dx, ay + t * dy
        d = (x - qx) * (x - qx) + (y - qy) * (y - qy)
        better = d < best
        best = np.where(better, d, best)
        w[better, a] = (dtype(1.0) - t)[better]; w[better, b] = t[better]; w[better, c] = 0
    return w


def texel_aovs_ref(arrays, slots, material, tex_hw, dtype=np.float64, tol=UNCERTAIN_TOL):
    """The buffers of material ``material`` at ``tex_hw`` = (H, W) under the slot table ``slots`` (one int or None per instance).
    Returns a dict: ``data`` (H, W, 16) in ``dtype``; ``cov_g`` and ``reach_g`` (H, W) int64, the winners, -1 = none; ``uncertain``
    (H, W) bool, the texels where some candidate triangle's deciding quantity — for coverage the smallest signed distance to the lines of
    its sides, for reach the largest separation along the five axes — lies within ``tol`` pixels of zero."""
    dtype = np.dtype(dtype).type
    H, W = int(tex_hw[0]), int(tex_hw[1])
    P, Nn, UV, area, inst = world_triangles(arrays, dtype)
    Q = pixel_space(UV, H, W, dtype)
    cov_g = np.full((H, W), EMPTY, np.int64); reach_g = np.full((H, W), EMPTY, np.int64)
    uncertain = np.zeros((H, W), bool)
    setups = {}
    for g in range(Q.shape[0]):
        if slots[inst[g]] is None or slots[inst[g]] != material or np.isnan(Q[g]).any():
            continue
        S = setups[g] = Setup(Q[g], dtype)
        fx0, fx1 = max(np.ceil(S.minx - dtype(1.0)), 0.0), min(np.floor(S.maxx + dtype(1.0)), float(W - 1))
        fy0, fy1 = max(np.ceil(S.miny - dtype(1.0)), 0.0), min(np.floor(S.maxy + dtype(1.0)), float(H - 1))
        if not (fx0 <= fx1 and fy0 <= fy1):
            continue
        ys, xs = np.mgrid[int(fy0):int(fy1) + 1, int(fx0):int(fx1) + 1]
        cov, reach, unc = classify_points(S, xs.astype(dtype), ys.astype(dtype), dtype, tol)
        win = (slice(int(fy0), int(fy1) + 1), slice(int(fx0), int(fx1) + 1))
        uncertain[win] |= unc
        cg, rg = cov_g[win], reach_g[win]                    # g rises: the first to arrive is the lowest
        cg[cov & (cg == EMPTY)] = g; rg[reach & (rg == EMPTY)] = g
    data = np.zeros((H, W, 16), dtype)
    data[..., 14:16] = -1
    winner = np.where(cov_g != EMPTY, cov_g, reach_g)
    for g in np.unique(winner[winner != EMPTY]):
        S, q = setups[g], Q[g]
        ys, xs = np.nonzero(winner == g)
        x, y = xs.astype(dtype), ys.astype(dtype)
        covered = cov_g[ys, xs] == g
        w = np.zeros((x.shape[0], 3), dtype); w[:, 0] = 1
        if not S.degenerate:
            if covered.any():
                e = [S.e[k](x[covered], y[covered]) for k in range(3)]
                s = (e[0] + e[1]) + e[2]
                ok = (s > 0) | (s < 0)
                wc = np.zeros((s.shape[0], 3), dtype); wc[:, 0] = 1
                for k in range(3):
                    wc[ok, k] = (e[k][ok] / s[ok])
                w[covered] = wc
            if (~covered).any():
                w[~covered] = closest_barycentrics(q, x[~covered], y[~covered], dtype)
        pos = (P[g, 0][None] * w[:, 0:1] + P[g, 1][None] * w[:, 1:2]) + P[g, 2][None] * w[:, 2:3]
        nrm = (Nn[g, 0][None] * w[:, 0:1] + Nn[g, 1][None] * w[:, 1:2]) + Nn[g, 2][None] * w[:, 2:3]
        ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
        size = dtype(0.0) if S.degenerate else np.sqrt(area[g] / (dtype(0.5) * S.abs2))
        data[ys, xs, 4:7] = nrm / ln[:, None]
        data[ys, xs, 7] = size
        data[ys, xs, 8:11] = pos
        data[ys, xs, 11] = covered
        data[ys, xs, 12] = 1
        data[ys, xs, 14] = inst[g]
        data[ys, xs, 15] = material
    return {"data": data, "cov_g": cov_g, "reach_g": reach_g, "uncertain": uncertain}


def bilinear_touched(arrays, slots, material, tex_hw, per_triangle, seed=0):
    """(H, W) bool: the texels that ``per_triangle`` random bilinear lookups on every triangle of the material touch with a non-zero
    weight, by tex_footprint of csrc/scene.h in float64 (CLAMP addressing included)."""
    H, W = int(tex_hw[0]), int(tex_hw[1])
    _, _, UV, _, inst = world_triangles(arrays, np.float64)
    rng = np.random.default_rng(seed)
    touched = np.zeros((H, W), bool)
    for g in range(UV.shape[0]):
        if slots[inst[g]] is None or slots[inst[g]] != material or np.isnan(UV[g]).any():
            continue
        b = rng.random((per_triangle, 2))
        flip = b.sum(1) > 1
        b[flip] = 1 - b[flip]
        uv = UV[g, 0].astype(np.float64) * (1 - b[:, :1] - b[:, 1:]) + UV[g, 1].astype(np.float64) * b[:, :1] + UV[g, 2].astype(np.float64) * b[:, 1:]
        px, py = uv[:, 0] * (W - 1), (1 - uv[:, 1]) * (H - 1)
        ix, iy = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)
        ox, oy = px - ix, py - iy
        for dx, wx in ((0, 1 - ox), (1, ox)):
            for dy, wy in ((0, 1 - oy), (1, oy)):
                hit = (wx * wy) != 0
                inside = (ix + dx >= 0) & (ix + dx <= W - 1) & (iy + dy >= 0) & (iy + dy <= H - 1)   # UVs outside [0, 1]: not modelled
                sel = hit & inside
                touched[(iy + dy)[sel], (ix + dx)[sel]] = True
    return touched
