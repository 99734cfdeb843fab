"""Reference of the bounced light (include/zdr.h, zdr_scene_texel_bounce) in NumPy, for any float dtype: float64 is the truth the GPU
tests compare with, float32 measures what float32 alone costs (tests/texel_bounce_cases.py turns that into the bars).

Built on what exists: ``sample_light``, ``make_onb`` and ``light_table`` of tests/texel_lighting_ref.py, the draws of the oracle's sampler
dump (bit for bit the kernels' numbers), ``OracleScene.trace_closest`` and ``trace_any`` for the segments, the world triangles of
tests/texel_ref.py — the float32 corners, normals and UVs of the host's records — for the interaction (checked against the oracle's
``light_rows("interact")`` in tests/test_texel_bounce_ref_host.py), the origin offset of Waechter & Binder as tests/light_cases.py has
it, and a bilinear lookup per read_bsdf.  The float32 world corners, the draws, the materials, the map and its tables are data both
dtypes share; everything computed from them is computed in ``dtype``.

It returns the walks sample by sample and vertex by vertex in the fields of the dump's layout, the texel buffer, and the NEAR flags: a
sample-vertex is near when a discrete decision up to and including it lies within TOL of flipping — the list of texel_lighting_ref
(u_pick x n, u_prim x T, cos_light against 1e-4, c against 0, make_onb's branch) plus both facing tests against 1e-4.  With ``hits=``
it skips the closest-hit traces and shades the hits it is given.  A helper, not a test."""
import ctypes as C

import numpy as np

import oracle
import texel_lighting_ref as LR
import texel_ref as R

TOL = LR.TOL
F_SHADED, F_LIT, F_FREE, F_ADDED, F_ON = 1, 2, 4, 8, 16


def draws(kind, xs, ys, seed, spp, samples, K, tables=None):
    """(len(xs), len(samples), 2 + 7 K) float32: the sampler dump with nvert = K and rr_depth = K (no roulette draw)"""
    L = oracle.lib()
    if tables is not None:
        L = LR.private_sampler()
        pmj, bn = (np.ascontiguousarray(tables[0], np.uint32), np.ascontiguousarray(tables[1], np.uint16))
        LR._PRIVATE["tables"] = (pmj, bn)
        L.zdro_set_pmj02bn_tables(pmj.ctypes.data_as(C.POINTER(C.c_uint32)), pmj.shape[0], pmj.shape[1],
                                  bn.ctypes.data_as(C.POINTER(C.c_uint16)), bn.shape[0], bn.shape[1])
    n = 2 + 7 * K
    out = np.zeros((len(xs), len(samples), n), np.float32)
    buf = np.zeros(2 + 8 * K, np.float32)
    for k, (x, y) in enumerate(zip(xs, ys)):
        for j, s in enumerate(samples):
            got = L.zdro_sampler_dump(kind, int(x), int(y), int(seed) & 0xFFFFFFFF, int(spp), int(s), K, K, buf.ctypes.data_as(C.POINTER(C.c_float)))
            assert got == n, (got, n)
            out[k, j] = buf[:n]
    return out


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(a, dtype):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (a / np.sqrt(_dot(a, a))[..., None]).astype(dtype)


def cosine_lobe(u, dtype):
    """(r cos phi, r sin phi, sqrt(1 - u.x)): the cosine lobe of ggx_sample (csrc/microfacet.h)"""
    ux, uy = u[:, 0].astype(dtype), u[:, 1].astype(dtype)
    r, phi = np.sqrt(ux), dtype(2.0) * dtype(np.pi) * uy
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(dtype(1.0) - ux)], -1).astype(dtype)


def to_world(n, local, dtype):
    t, b = LR.make_onb(n, dtype)
    return (local[:, 0:1] * t + local[:, 1:2] * b + local[:, 2:3] * n).astype(dtype)


def offset_ray_origin(p, n):
    """offset_ray_origin (csrc/scene.h; Waechter & Binder), a float32 operation: p and n are rounded to float32 first"""
    p32, n32 = np.asarray(p, np.float32), np.asarray(n, np.float32)
    of_i = (np.float32(256.0) * n32).astype(np.int64)                 # truncation, as (int)
    bits = p32.view(np.int32).astype(np.int64) + np.where(p32 < 0, -of_i, of_i)
    p_i = ((bits + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32).view(np.float32)
    return np.where(np.abs(p32) < np.float32(1.0 / 32.0), p32 + np.float32(1.0 / 65536.0) * n32, p_i).astype(np.float32)


def read_bsdf(mat, uv, dtype):
    """read_bsdf (csrc/scene.h): bilinear, clamp addressing, texel (x, y) at x + w y, v flipped; mat (h, w, 4) float32 -> (N, 3)"""
    h, w = mat.shape[:2]
    px, py = uv[:, 0] * dtype(w - 1), (dtype(1.0) - uv[:, 1]) * dtype(h - 1)
    ix, iy = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)
    ox, oy = (px - ix).astype(dtype)[:, None], (py - iy).astype(dtype)[:, None]
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    m = mat[..., :3].astype(dtype)
    c00, c01, c10, c11 = m[y0, x0], m[y1, x0], m[y0, x1], m[y1, x1]
    a, b = c00 + oy * (c01 - c00), c10 + oy * (c11 - c10)
    return (a + ox * (b - a)).astype(dtype)


class Geometry:
    """the float32 records of the host, as arrays in ``dtype``"""
    def __init__(self, arrays, dtype):
        P, Nn, UV, _, inst = R.world_triangles(arrays, np.float32)
        self.P, self.N, self.UV = P.astype(dtype), Nn.astype(dtype), UV.astype(dtype)
        c = np.cross(self.P[:, 1] - self.P[:, 0], self.P[:, 2] - self.P[:, 0]).astype(dtype)
        self.ng = _normalize(c, dtype)
        self.begin = np.asarray(arrays.inst_tri_begin, np.int64)
        self.dtype = dtype

    def interact(self, inst, prim, u, v):
        """surface_interact at (inst, prim, u, v): p, uv, ns, ng"""
        d = self.dtype
        g = self.begin[inst] + prim
        w1, w2 = u.astype(d)[:, None], v.astype(d)[:, None]
        w0 = d(1.0) - w1 - w2
        p = self.P[g, 0] * w0 + self.P[g, 1] * w1 + self.P[g, 2] * w2
        uv = self.UV[g, 0] * w0 + self.UV[g, 1] * w1 + self.UV[g, 2] * w2
        ns = _normalize((self.N[g, 0] * w0 + self.N[g, 1] * w1 + self.N[g, 2] * w2).astype(d), d)
        return p.astype(d), uv.astype(d), ns, self.ng[g]


def _rays(o, d, tmin, tmax):
    rays = np.zeros((o.shape[0], 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = tmin; rays[:, 4:7] = d; rays[:, 7] = tmax
    return rays


def texel_bounce_ref(arrays, oscene, texel_data, materials, slots, *, spp, bounces, seed=0, samples=None, sampler="cmj", env=None,
                     dtype=np.float64, tables=None, hits=None):
    """The walks and the buffer of include/zdr.h, zdr_scene_texel_bounce, for the sample points ``texel_data`` (H, W, 16), the
    ``materials`` (a list of (h, w, 4) float32 arrays) and the slot table ``slots`` (one entry per instance, None = no material).
    Returns a dict.  Per sample (N = shaded texels x samples of the range, texel-major): ``queries`` (N, 3) int32 {x, y, s}, ``nvert``
    (N,), ``surface`` (N,) 0 / 1.  Per sample and vertex (N, K, ...): ``inst``, ``prim``, ``uv`` (N, K, 2), ``flags``, ``beta`` (N, K, 3),
    ``add`` (N, K, 3), ``near`` (N, K) bool, cumulative along the walk.  ``data`` (H, W, 4) in ``dtype``: the texel buffer, every
    texel's adds summed with s ascending and, within s, k ascending.
    ``hits``: a dict with ``nvert`` (N,), ``inst``, ``prim`` (N, K) and ``uv`` (N, K, 2) for the same N samples in the same order —
    segment k then hits what it says (or nothing, k >= nvert) and no closest-hit ray is traced."""
    dtype = np.dtype(dtype).type
    K = int(bounces)
    texel_data = np.asarray(texel_data)
    H, W = texel_data.shape[:2]
    begin, end = (0, spp) if samples is None else samples
    S = np.arange(begin, end)
    nrm_all, pos_all = texel_data[..., 4:7], texel_data[..., 8:11]
    shade = (texel_data[..., 12] == 1) & ~np.isnan(nrm_all).any(-1) & ~np.isnan(pos_all).any(-1)
    ys, xs = np.nonzero(shade)
    T, ns_ = ys.shape[0], S.shape[0]
    N = T * ns_
    out = {"data": np.zeros((H, W, 4), dtype),
           "queries": np.stack([np.repeat(xs, ns_), np.repeat(ys, ns_), np.tile(S, T)], -1).astype(np.int32).reshape(N, 3),
           "nvert": np.zeros(N, np.int64), "surface": np.zeros(N, np.int64),
           "inst": np.full((N, K), -1, np.int64), "prim": np.full((N, K), -1, np.int64), "uv": np.zeros((N, K, 2), dtype),
           "flags": np.zeros((N, K), np.int64), "beta": np.zeros((N, K, 3), dtype), "add": np.zeros((N, K, 3), dtype),
           "near": np.zeros((N, K), bool)}
    if N == 0:
        return out
    slot_of_inst = np.array([-1 if k is None else int(k) for k in slots], np.int64)
    mats = [np.asarray(m, np.float32) for m in materials]
    geo = Geometry(arrays, dtype)
    lights = LR.light_table(arrays, dtype)
    u = draws(LR.SAMPLER_KINDS[sampler], xs, ys, seed, spp, S, K, tables).reshape(N, 2 + 7 * K)
    n = np.repeat(nrm_all[ys, xs].astype(dtype), ns_, axis=0); p = np.repeat(pos_all[ys, xs].astype(dtype), ns_, axis=0)
    near = np.abs(np.abs(n[:, 0]).astype(np.float64) - np.abs(n[:, 2])) < TOL          # make_onb's branch
    direction = to_world(n, cosine_lobe(u[:, 0:2], dtype), dtype)
    org, tmin = p.copy(), 1e-4
    beta = np.ones((N, 3), dtype)
    alive = np.ones(N, bool)
    for k in range(K):
        uk = u[:, 2 + 7 * k: 9 + 7 * k]
        alive = alive & ~np.isnan(direction).any(1)
        inst = np.zeros(N, np.int64); prim = np.zeros(N, np.int64); hu = np.zeros(N, np.float32); hv = np.zeros(N, np.float32)
        idx = np.nonzero(alive)[0]
        if hits is None:
            ip, bt = oscene.trace_closest(_rays(org[idx], direction[idx], tmin, 1e30))
            got = ip[:, 0] >= 0
            inst[idx] = np.where(got, ip[:, 0], 0); prim[idx] = np.where(got, ip[:, 1], 0)
            hu[idx] = np.where(got, bt[:, 0], 0); hv[idx] = np.where(got, bt[:, 1], 0)
            hit = np.zeros(N, bool); hit[idx] = got
        else:
            hit = alive & (np.asarray(hits["nvert"]) > k)
            inst = np.where(hit, np.asarray(hits["inst"])[:, k], 0).astype(np.int64); prim = np.where(hit, np.asarray(hits["prim"])[:, k], 0).astype(np.int64)
            hu = np.where(hit, np.asarray(hits["uv"])[:, k, 0], 0).astype(np.float32); hv = np.where(hit, np.asarray(hits["uv"])[:, k, 1], 0).astype(np.float32)
        alive = alive & hit
        ip_, iuv, ins, ing = geo.interact(inst, prim, hu, hv)
        with np.errstate(invalid="ignore"):
            f1, f2 = _dot(-direction, ing), _dot(-direction, ins)
            near = near | (alive & ((np.abs(f1 - 1e-4) < TOL) | (np.abs(f2 - 1e-4) < TOL)))
            front = ~((f1 < 1e-4) | (f2 < 1e-4))
        slot = slot_of_inst[inst]
        shaded = alive & front & (slot >= 0)
        if k == 0:
            out["surface"] = shaded.astype(np.int64)
        for m, mat in enumerate(mats):
            sel = np.nonzero(shaded & (slot == m))[0]
            if sel.size:
                beta[sel] = (beta[sel] * read_bsdf(mat, iuv[sel], dtype)).astype(dtype)
        walking = shaded
        # one light sample
        u6 = np.zeros((N, 6), np.float32); u6[:, 2:6] = uk[:, 0:4]
        wi, dist, pdf, ev, near_l = LR.sample_light(lights, env, ip_, u6, dtype)
        with np.errstate(invalid="ignore"):
            c = _dot(ins, wi)
            near = near | (walking & (near_l | (np.abs(c) < TOL)))
            lit = walking & (c > 0) & (ev > 0).any(1)
        free = lit.copy()
        idx = np.nonzero(lit)[0]
        if idx.size:
            free[idx] = ~oscene.trace_any(_rays(ip_[idx], wi[idx], 1e-4, dist[idx])).astype(bool)
        add = np.zeros((N, 3), dtype)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            add[free] = ((beta[free] * ev[free]) * (c[free] / np.maximum(pdf[free], dtype(1e-4)))[:, None]).astype(dtype)
        added = free & np.isfinite(add).all(1)
        add[~added] = 0
        # the next segment
        on = np.zeros(N, bool)
        nd = direction
        if k + 1 < K:
            wl = cosine_lobe(uk[:, 5:7], dtype)
            nd = to_world(ins, wl, dtype)
            with np.errstate(invalid="ignore"):
                g1 = _dot(nd, ing)
                near = near | (walking & ((np.abs(np.abs(ins[:, 0]).astype(np.float64) - np.abs(ins[:, 2])) < TOL) |
                                          (np.abs(g1 - 1e-4) < TOL) | (np.abs(wl[:, 2] - 1e-4) < TOL)))
                on = walking & ~((g1 < 1e-4) | (wl[:, 2] < 1e-4))
        out["nvert"] = np.where(hit, k + 1, out["nvert"])
        out["inst"][:, k] = np.where(hit, inst, -1); out["prim"][:, k] = np.where(hit, prim, -1)
        out["uv"][:, k, 0] = np.where(hit, hu, 0); out["uv"][:, k, 1] = np.where(hit, hv, 0)
        out["flags"][:, k] = np.where(hit, shaded * F_SHADED + lit * F_LIT + free * F_FREE + added * F_ADDED + on * F_ON, 0)
        out["beta"][:, k] = np.where(hit[:, None], beta, 0); out["add"][:, k] = add
        out["near"][:, k] = near
        alive = on
        direction = nd
        org = offset_ray_origin(ip_, ing).astype(dtype); tmin = 0.0
    acc = np.zeros((T, 3), dtype)
    per = out["add"].reshape(T, ns_, K, 3)
    for j in range(ns_):                                              # s ascending and, within s, k ascending
        for k in range(K):
            acc = (acc + per[:, j, k]).astype(dtype)
    out["data"][ys, xs, :3] = acc * (dtype(1.0) / dtype(spp))
    out["data"][ys, xs, 3] = out["surface"].reshape(T, ns_).sum(1).astype(dtype) / dtype(spp)
    return out


def parse_dump(rows, K):
    """the (n, 4 + 12 K) float32 rows of zdr_texel_bounce_dump as the fields of ``texel_bounce_ref``"""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    bits = rows.view(np.int32)
    v = rows[:, 4:].reshape(n, K, 12); vb = bits[:, 4:].reshape(n, K, 12)
    nvert = bits[:, 0].astype(np.int64)
    have = np.arange(K)[None, :] < nvert[:, None]
    return {"nvert": nvert, "surface": rows[:, 1].astype(np.int64), "inst": np.where(have, vb[..., 0], -1).astype(np.int64),
            "prim": np.where(have, vb[..., 1], -1).astype(np.int64), "uv": v[..., 2:4].copy(), "flags": vb[..., 4].astype(np.int64),
            "beta": v[..., 5:8].copy(), "add": v[..., 8:11].copy()}


def signature_equal(a, b):
    """(N,) bool: two sets of walks agree in nvert and in the triangle and the flags at every vertex"""
    return (a["nvert"] == b["nvert"]) & (a["inst"] == b["inst"]).all(1) & (a["prim"] == b["prim"]).all(1) & (a["flags"] == b["flags"]).all(1)


def triangles_equal(a, b):
    """(N,) bool: nvert and the triangle at every vertex agree"""
    return (a["nvert"] == b["nvert"]) & (a["inst"] == b["inst"]).all(1) & (a["prim"] == b["prim"]).all(1)
