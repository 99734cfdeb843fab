"""Reference of the adjoint of the texture-space lighting (include/zdr.h, zdr_scene_texel_lighting_backward) in NumPy, for any float dtype,
built from the helpers of tests/texel_lighting_ref.py: the same draws, the same sample_light, the same light table (with ``emissions=``),
visibility from ``OracleScene.trace_any``.  float64 is the truth the GPU tests compare with; float32 measures what float32 alone costs
(tests/texel_lighting_grad_cases.py turns that into the bars).

Every accepted sample of a shaded texel t forms term[ch] = (d_out[t][ch] / spp) * w, w = c / max(pdf, 1e-4); a sample of mesh light l adds
it to the row of l's instance, a sample of the environment map adds k * term to the four taps of the map's bilinear lookup.  Besides the
two gradients the reference returns, per entry, the sum of |terms| and the number of terms — what any summation order can cost is bounded
by the first — and the UNCERTAIN texels: those of the forward reference, and in addition those with an environment sample whose alias
table decisions (cell index, accept or alias) lie within TOL of flipping.  A helper, not a test; tests/test_texel_lighting_grad_ref_host.py
pins it by linearity."""
import numpy as np

import texel_lighting_ref as LR

TOL = LR.TOL


def _alias_near(prob, n, u, offset, dtype):
    """whether sample_alias_table's two decisions for u lie within TOL of flipping"""
    un = u * dtype(n)
    i = np.clip(un.astype(np.int64), 0, n - 1)
    ur = (un - np.floor(un)).astype(dtype)
    return (np.abs(un - np.rint(un)) < TOL) | (np.abs(ur - prob[i + offset].astype(dtype)) < TOL)


def env_sample_uv(env, u, dtype):
    """the map coordinates of sample_light's environment branch for draws u (N, 6) -> u (N,), v (N,), near (N,)"""
    _, prob, alias, _, mw, mh = env
    iy, uy = LR.alias_sample(prob, alias, mh, u[:, 5].astype(dtype), 0, dtype)
    near = _alias_near(prob, mh, u[:, 5].astype(dtype), 0, dtype)
    ix, ux = LR.alias_sample(prob, alias, mw, u[:, 4].astype(dtype), mh + iy * mw, dtype)
    near |= _alias_near(prob, mw, u[:, 4].astype(dtype), mh + iy * mw, dtype)
    return ((ix.astype(dtype) + ux) / dtype(mw)).astype(dtype), ((iy.astype(dtype) + uy) / dtype(mh)).astype(dtype), near


def env_taps(shape, u, v, dtype):
    """env_lookup's footprint: -> (y (N, 4), x (N, 4), k (N, 4)) in the order (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy"""
    H, W = shape[:2]
    x, y = u * dtype(W) - dtype(0.5), v * dtype(H) - dtype(0.5)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(dtype), (y - y0f).astype(dtype)
    x0 = np.clip(x0f.astype(np.int64), 0, W - 1); x1 = np.clip(x0f.astype(np.int64) + 1, 0, W - 1)
    y0 = np.clip(y0f.astype(np.int64), 0, H - 1); y1 = np.clip(y0f.astype(np.int64) + 1, 0, H - 1)
    one = dtype(1.0)
    k = np.stack([(one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy], 1).astype(dtype)
    return np.stack([y0, y0, y1, y1], 1), np.stack([x0, x1, x0, x1], 1), k


def light_instances(arrays, emissions=None):
    em = np.asarray(arrays.inst_emission if emissions is None else emissions, np.float32).reshape(-1, 3)
    return [i for i in range(arrays.ninst) if (em[i] > 0).any()]


def texel_lighting_grad_ref(arrays, oscene, texel_data, d_out, *, spp, seed=0, samples=None, sampler="cmj", env=None, emissions=None,
                            dtype=np.float64, tables=None):
    """The adjoint of ``texel_lighting_ref``'s irradiance for the cotangent ``d_out`` (H, W, 4; float 3 is ignored).  Returns a dict:
    ``d_emission`` (ninst, 3) and ``d_env`` (the map's (h, w, 4), alpha 0; None without a map) in ``dtype``; ``abs_emission``, ``abs_env``:
    the sums of |terms| per entry, float64; ``n_emission`` (ninst,), ``n_env`` (h, w): the number of terms per row / texel;
    ``uncertain`` (H, W) bool; ``lit_env``, ``lit_mesh`` (H, W) int: the accepted samples per texel of either kind."""
    dtype = np.dtype(dtype).type
    texel_data = np.asarray(texel_data)
    H, W = texel_data.shape[:2]
    begin, end = (0, spp) if samples is None else samples
    S = np.arange(begin, end)
    nrm_all, pos_all = texel_data[..., 4:7], texel_data[..., 8:11]
    shade = (texel_data[..., 12] == 1) & ~np.isnan(nrm_all).any(-1) & ~np.isnan(pos_all).any(-1)
    ys, xs = np.nonzero(shade)
    K, ns = ys.shape[0], S.shape[0]
    ninst = arrays.ninst
    out = {"d_emission": np.zeros((ninst, 3), dtype), "abs_emission": np.zeros((ninst, 3)), "n_emission": np.zeros(ninst, np.int64),
           "d_env": None, "abs_env": None, "n_env": None, "uncertain": np.zeros((H, W), bool),
           "lit_env": np.zeros((H, W), np.int64), "lit_mesh": np.zeros((H, W), np.int64)}
    if env is not None:
        eh, ew = env[0].shape[:2]
        out["d_env"] = np.zeros((eh, ew, 4), dtype); out["abs_env"] = np.zeros((eh, ew, 4)); out["n_env"] = np.zeros((eh, ew), np.int64)
    if K == 0:
        return out
    u = LR.draws(LR.SAMPLER_KINDS[sampler], xs, ys, seed, spp, S, tables).reshape(K * ns, 6)
    n = np.repeat(nrm_all[ys, xs].astype(dtype), ns, axis=0); p = np.repeat(pos_all[ys, xs].astype(dtype), ns, axis=0)
    near = np.abs(np.abs(n[:, 0]).astype(np.float64) - np.abs(n[:, 2])) < TOL
    lights = LR.light_table(arrays, dtype, emissions)
    insts = light_instances(arrays, emissions)
    env_count = 0 if env is None else 1
    nl = env_count + len(lights)
    # the acceptance test of the forward, replayed
    wi, dist, pdf, ev, near_l = LR.sample_light(lights, env, p, u, dtype)
    near |= near_l
    with np.errstate(invalid="ignore"):
        c = LR._dot(n, wi)
        near |= np.abs(c) < TOL
        lit = (c > 0) & (ev > 0).any(1)
    idx = np.nonzero(lit)[0]
    lit[idx] = ~LR.trace_any(oscene, p[idx], wi[idx], 1e-4, dist[idx])
    w = np.zeros(K * ns, dtype)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        w[lit] = (c[lit] / np.maximum(pdf[lit], dtype(1e-4))).astype(dtype)
        lit &= np.isfinite(ev * w[:, None]).all(1)
    g = np.repeat(np.asarray(d_out)[ys, xs, :3].astype(dtype), ns, axis=0)
    term = ((g * (dtype(1.0) / dtype(spp))).astype(dtype) * w[:, None]).astype(dtype)
    pick = np.zeros(K * ns, np.int64)
    if nl:
        pick = np.clip((u[:, 2].astype(dtype) * dtype(nl)).astype(np.int64), 0, nl - 1)
    is_env = lit & (pick < env_count)
    for l, inst in enumerate(insts):
        sel = np.nonzero(lit & (pick == l + env_count))[0]
        for ch in range(3):
            acc = dtype(0.0)
            for v in term[sel, ch]:                                   # in sample order, in ``dtype``
                acc = dtype(acc + v)
            out["d_emission"][inst, ch] = acc
        out["abs_emission"][inst] = np.abs(term[sel].astype(np.float64)).sum(0)
        out["n_emission"][inst] = sel.size
    if env is not None:
        all_env = np.nonzero(pick < env_count)[0]                   # (accepted or not: a flipped decision could have made one accepted)
        uu, vv, near_e = env_sample_uv(env, u[all_env], dtype)
        near[all_env] |= near_e
        keep = is_env[all_env]
        sel, uu, vv = all_env[keep], uu[keep], vv[keep]
        ty, tx, k = env_taps(env[0].shape, uu, vv, dtype)
        for m in range(4):
            add = (k[:, m, None] * term[sel]).astype(dtype)
            for ch in range(3):
                np.add.at(out["d_env"][..., ch], (ty[:, m], tx[:, m]), add[:, ch])
                np.add.at(out["abs_env"][..., ch], (ty[:, m], tx[:, m]), np.abs(add[:, ch].astype(np.float64)))
            np.add.at(out["n_env"], (ty[:, m], tx[:, m]), 1)
    out["uncertain"][ys, xs] = near.reshape(K, ns).any(1)
    out["lit_env"][ys, xs] = is_env.reshape(K, ns).sum(1)
    out["lit_mesh"][ys, xs] = (lit & ~is_env).reshape(K, ns).sum(1)
    return out
