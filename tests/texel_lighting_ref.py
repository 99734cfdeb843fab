"""Reference of the texture-space lighting (include/zdr.h, zdr_scene_texel_lighting) in NumPy, for any float dtype: float64 is the truth
the GPU tests compare with, float32 measures what float32 alone costs (tests/texel_lighting_cases.py turns that into the bars).

What it is given: the sample points — an (H, W, 16) buffer in the layout of zdr_scene_texel_aovs, from tests/texel_ref.py — the scene as
``SceneArrays`` (the light table is formed from it as the host forms it: the lights are the instances with a positive emission
component, in instance order, their triangles in input order, world corners in float32), the draws of ``oracle.sampler_dump`` (bit for
bit the kernels' numbers), visibility from ``OracleScene.trace_any`` and, for a scene with an environment map, the map and its
importance-sampling tables as zdr_amd/envmap.py builds them.  The float32 world corners, the draws, the map and the tables are data
both dtypes share; everything computed from them is computed in ``dtype``.

Besides the buffer it returns the UNCERTAIN texels: those with a sample whose discrete decision could flip under float32 rounding —
u_pick x n or u_prim x T within TOL of an integer, cos_light within TOL of 1e-4, c = n . wi within TOL of 0 — or whose normal sits on
make_onb's branch, |n.x| - |n.z| within TOL of 0.  A helper, not a test; tests/test_texel_lighting_ref_host.py pins it."""
import numpy as np

import oracle
import texel_ref as R

TOL = 1e-5
SAMPLER_KINDS = {"cmj": oracle.SAMPLER_CMJ, "pmj02bn": oracle.SAMPLER_PMJ02BN}


def light_table(arrays, dtype, emissions=None):
    """[(corners (T, 3, 3), ng (T, 3), area (T,), emission (3,))] per light, in ``dtype``, from the float32 world corners"""
    dtype = np.dtype(dtype).type
    P = R.world_triangles(arrays, np.float32)[0].astype(dtype)
    em = np.asarray(arrays.inst_emission if emissions is None else emissions, np.float32).reshape(-1, 3)
    lights = []
    for i in range(arrays.ninst):
        if not (em[i] > 0).any():
            continue
        b, e = int(arrays.inst_tri_begin[i]), int(arrays.inst_tri_begin[i + 1])
        c = np.cross(P[b:e, 1] - P[b:e, 0], P[b:e, 2] - P[b:e, 0]).astype(dtype)
        ln = np.sqrt((c * c).sum(1)).astype(dtype)
        lights.append((P[b:e], (c / ln[:, None]).astype(dtype), (ln / dtype(2.0)).astype(dtype), em[i].astype(dtype)))
    return lights


_PRIVATE = {}


def private_sampler():
    """A second instance of the oracle's library, loaded from a copy of its file: the pmj02bn tables are state of the library, which
    other tests set on the shared instance, so draws that need tables of their own take them here and leave the shared ones alone."""
    if "lib" not in _PRIVATE:
        import ctypes as C
        import shutil
        import tempfile
        with tempfile.NamedTemporaryFile(suffix=".so") as f:
            shutil.copyfile(oracle.build(), f.name)
            L = C.CDLL(f.name)                                        # (the mapping outlives the file)
        L.zdro_sampler_dump.restype = C.c_int
        L.zdro_sampler_dump.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.zdro_set_pmj02bn_tables.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.POINTER(C.c_uint16), C.c_int, C.c_int]
        _PRIVATE["lib"] = L
    return _PRIVATE["lib"]


def draws(kind, xs, ys, seed, spp, samples, tables=None):
    """(len(xs), len(samples), 6) float32: u_ao.xy, u_pick, u_prim, u_pt.xy — floats 0..5 of the sampler dump with one vertex.
    ``tables``: (pmj uint32 [nsets][nsamples][2], blue noise uint16 [ntex][res][res]) for pmj02bn, set on a private instance of the oracle"""
    import ctypes as C
    L = oracle.lib()
    if tables is not None:
        L = private_sampler()
        pmj, bn = (np.ascontiguousarray(tables[0], np.uint32), np.ascontiguousarray(tables[1], np.uint16))
        _PRIVATE["tables"] = (pmj, bn)                                # (kept alive: the library may keep the pointers)
        L.zdro_set_pmj02bn_tables(pmj.ctypes.data_as(C.POINTER(C.c_uint32)), pmj.shape[0], pmj.shape[1],
                                  bn.ctypes.data_as(C.POINTER(C.c_uint16)), bn.shape[0], bn.shape[1])
    out = np.zeros((len(xs), len(samples), 6), np.float32)
    buf = np.zeros(10, np.float32)
    for k, (x, y) in enumerate(zip(xs, ys)):
        for j, s in enumerate(samples):
            n = L.zdro_sampler_dump(kind, int(x), int(y), int(seed) & 0xFFFFFFFF, int(spp), int(s), 1, 2, buf.ctypes.data_as(C.POINTER(C.c_float)))
            assert n >= 6
            out[k, j] = buf[:6]
    return out


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(a, dtype):
    return (a / np.sqrt(_dot(a, a))[..., None]).astype(dtype)


def make_onb(n, dtype):
    """(tangent, binormal) of make_onb (csrc/scene.h) for normals (..., 3)"""
    zero = np.zeros(n.shape[:-1], dtype)
    first = np.abs(n[..., 0]) > np.abs(n[..., 2])
    b = np.where(first[..., None], np.stack([-n[..., 1], n[..., 0], zero], -1), np.stack([zero, -n[..., 2], n[..., 1]], -1)).astype(dtype)
    b = _normalize(b, dtype)
    t = _normalize(np.cross(b, n).astype(dtype), dtype)
    return t, b


def alias_sample(prob, alias, n, u, offset, dtype):
    """sample_alias_table (csrc/scene.h): -> (index, remapped u); ``offset`` may be an array"""
    un = u * dtype(n)
    i = np.clip(un.astype(np.int64), 0, n - 1)
    ur = (un - np.floor(un)).astype(dtype)
    pr = prob[i + offset].astype(dtype)
    take = ur < pr
    with np.errstate(divide="ignore", invalid="ignore"):
        uu = np.where(take, ur / pr, (ur - pr) / (dtype(1.0) - pr)).astype(dtype)
    return np.where(take, i, alias[i + offset].astype(np.int64)), uu


def env_lookup(tex, u, v, dtype):
    """env_lookup (csrc/scene.h): bilinear between texel centres, clamp to edge; tex (H, W, 4) float32 -> (..., 3)"""
    H, W = tex.shape[:2]
    x, y = u * dtype(W) - dtype(0.5), v * dtype(H) - dtype(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(dtype)[..., None], (y - y0f).astype(dtype)[..., None]
    x0 = np.clip(x0f.astype(np.int64), 0, W - 1); x1 = np.clip(x0f.astype(np.int64) + 1, 0, W - 1)
    y0 = np.clip(y0f.astype(np.int64), 0, H - 1); y1 = np.clip(y0f.astype(np.int64) + 1, 0, H - 1)
    t = tex[..., :3].astype(dtype)
    top = t[y0, x0] + (t[y0, x1] - t[y0, x0]) * fx
    bot = t[y1, x0] + (t[y1, x1] - t[y1, x0]) * fx
    return (top + (bot - top) * fy).astype(dtype)


def sample_light(lights, env, origin, u, dtype):
    """sample_light (csrc/scene.h) for origins (N, 3) and draws u (N, 6).  ``env``: None or (tex, alias_prob, alias_idx, pdf, map_w, map_h).
    -> wi (N, 3), dist, pdf, eval (N, 3), near (N,) bool: a discrete decision of the sample lies within TOL of flipping"""
    N = origin.shape[0]
    env_count = 0 if env is None else 1
    n = env_count + len(lights)
    wi = np.zeros((N, 3), dtype); wi[:, 2] = 1
    dist = np.zeros(N, dtype); pdf = np.ones(N, dtype); ev = np.zeros((N, 3), dtype); near = np.zeros(N, bool)
    if n == 0:
        return wi, dist, pdf, ev, near
    pick = u[:, 2].astype(dtype) * dtype(n)
    near |= np.abs(pick - np.rint(pick)) < TOL
    idx = np.clip(pick.astype(np.int64), 0, n - 1)
    if env is not None:
        tex, prob, alias, epdf, mw, mh = env
        sel = np.nonzero(idx < env_count)[0]
        if sel.size:
            iy, uy = alias_sample(prob, alias, mh, u[sel, 5].astype(dtype), 0, dtype)
            ix, ux = alias_sample(prob, alias, mw, u[sel, 4].astype(dtype), mh + iy * mw, dtype)
            uvx = ((ix.astype(dtype) + ux) / dtype(mw)).astype(dtype); uvy = ((iy.astype(dtype) + uy) / dtype(mh)).astype(dtype)
            pi = dtype(np.pi)
            phi, theta = dtype(2.0) * pi * (dtype(1.0) - uvx), pi * uvy
            st = np.sin(theta)
            wi[sel] = _normalize(np.stack([np.sin(phi) * st, np.cos(theta), np.cos(phi) * st], -1).astype(dtype), dtype)
            dist[sel] = dtype(1e30)
            sn = np.sin(pi * uvy)
            with np.errstate(divide="ignore"):
                inv_s = np.where(sn > 0, dtype(1.0) / sn, dtype(0.0)).astype(dtype)
            pdf[sel] = epdf[iy * mw + ix].astype(dtype) * (inv_s / (dtype(2.0) * pi * pi * dtype(n)))
            ev[sel] = env_lookup(tex, uvx, uvy, dtype)
    for l, (P, ng, area, em) in enumerate(lights):
        sel = np.nonzero(idx == l + env_count)[0]
        if not sel.size:
            continue
        T = P.shape[0]
        up = u[sel, 3].astype(dtype) * dtype(T)
        near[sel] |= np.abs(up - np.rint(up)) < TOL
        prim = np.clip(up.astype(np.int64), 0, T - 1)
        ux, uy = u[sel, 4].astype(dtype), u[sel, 5].astype(dtype)
        lo = ux < uy                                                  # sample_uniform_triangle
        a = np.where(lo, dtype(0.5) * ux, dtype(-0.5) * uy + ux); b = np.where(lo, dtype(-0.5) * ux + uy, dtype(0.5) * uy)
        c = dtype(1.0) - a - b
        p = (P[prim, 0] * a[:, None] + P[prim, 1] * b[:, None] + P[prim, 2] * c[:, None]).astype(dtype)
        dp = (p - origin[sel]).astype(dtype)
        d2 = _dot(dp, dp)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = (dp / np.sqrt(d2)[:, None]).astype(dtype)
            cos_light = -_dot(ng[prim], w)
            pdf[sel] = d2 / (dtype(n * T) * area[prim] * cos_light)
        near[sel] |= np.abs(cos_light - 1e-4) < TOL
        wi[sel] = w
        dist[sel] = dtype(0.9999) * np.sqrt(d2)
        ev[sel] = np.where((cos_light > dtype(1e-4))[:, None], em[None, :], dtype(0.0))
    return wi, dist, pdf, ev, near


def trace_any(oscene, o, d, tmin, tmax):
    rays = np.zeros((o.shape[0], 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = tmin; rays[:, 4:7] = d; rays[:, 7] = tmax
    return oscene.trace_any(rays).astype(bool)


def texel_lighting_ref(arrays, oscene, texel_data, *, spp, seed=0, samples=None, max_distance=None, sampler="cmj", env=None, emissions=None,
                       dtype=np.float64, tables=None):
    """The buffer of include/zdr.h, zdr_scene_texel_lighting, for the sample points ``texel_data`` (H, W, 16).  Returns a dict: ``data``
    (H, W, 4) in ``dtype``; ``uncertain`` (H, W) bool; ``lit`` (H, W) int: how many samples of the texel added light; ``var`` (H, W, 4)
    float64: the sample variance of every channel's per-sample values (for the statistical tests).  ``tables``: as ``draws`` takes them."""
    dtype = np.dtype(dtype).type
    texel_data = np.asarray(texel_data)
    H, W = texel_data.shape[:2]
    begin, end = (0, spp) if samples is None else samples
    S = np.arange(begin, end)
    nrm_all, pos_all = texel_data[..., 4:7], texel_data[..., 8:11]
    shade = (texel_data[..., 12] == 1) & ~np.isnan(nrm_all).any(-1) & ~np.isnan(pos_all).any(-1)
    ys, xs = np.nonzero(shade)
    K, ns = ys.shape[0], S.shape[0]
    out = {"data": np.zeros((H, W, 4), dtype), "uncertain": np.zeros((H, W), bool), "lit": np.zeros((H, W), np.int64), "var": np.zeros((H, W, 4))}
    if K == 0:
        return out
    u = draws(SAMPLER_KINDS[sampler], xs, ys, seed, spp, S, tables).reshape(K * ns, 6)
    n = np.repeat(nrm_all[ys, xs].astype(dtype), ns, axis=0); p = np.repeat(pos_all[ys, xs].astype(dtype), ns, axis=0)
    near = np.abs(np.abs(n[:, 0]).astype(np.float64) - np.abs(n[:, 2])) < TOL
    # openness
    t, b = make_onb(n, dtype)
    r, phi = np.sqrt(u[:, 0].astype(dtype)), dtype(2.0) * dtype(np.pi) * u[:, 1].astype(dtype)
    lx, ly, lz = r * np.cos(phi), r * np.sin(phi), np.sqrt(dtype(1.0) - u[:, 0].astype(dtype))
    d = (lx[:, None] * t + ly[:, None] * b + lz[:, None] * n).astype(dtype)
    ok = ~np.isnan(d).any(1)
    occ = np.zeros(K * ns, bool)
    occ[ok] = trace_any(oscene, p[ok], d[ok], 1e-4, 1e30 if max_distance is None else max_distance)
    opn = (~occ).astype(dtype)
    # irradiance
    wi, dist, pdf, ev, near_l = sample_light(light_table(arrays, dtype, emissions), env, p, u, dtype)
    near |= near_l
    with np.errstate(invalid="ignore"):
        c = _dot(n, wi)
        near |= np.abs(c) < TOL
        lit = (c > 0) & (ev > 0).any(1)
    idx = np.nonzero(lit)[0]
    lit[idx] = ~trace_any(oscene, p[idx], wi[idx], 1e-4, dist[idx])
    add = np.zeros((K * ns, 3), dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        add[lit] = (ev[lit] * (c[lit] / np.maximum(pdf[lit], dtype(1e-4)))[:, None]).astype(dtype)
    fin = np.isfinite(add).all(1)
    add[~fin] = 0; lit &= fin
    per = np.concatenate([add, opn[:, None]], 1).reshape(K, ns, 4)
    acc = np.zeros((K, 4), dtype)
    for j in range(ns):                                               # in sample order
        acc = (acc + per[:, j]).astype(dtype)
    out["data"][ys, xs, :3] = acc[:, :3] * (dtype(1.0) / dtype(spp))
    out["data"][ys, xs, 3] = acc[:, 3] / dtype(spp)
    out["uncertain"][ys, xs] = near.reshape(K, ns).any(1)
    out["lit"][ys, xs] = lit.reshape(K, ns).sum(1)
    if ns > 1:
        out["var"][ys, xs] = per.astype(np.float64).var(axis=1, ddof=1)
    return out
