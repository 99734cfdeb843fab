"""Reference of the adjoint of the bounced light (include/zdr.h, zdr_scene_texel_bounce_backward) in NumPy, for any float dtype, on GIVEN
hits and decisions: per sample and vertex the instance, the triangle and the barycentrics as ``texel_bounce_ref(hits=)`` takes them, and
the SHADED and ADDED flags.  Nothing is traced.  At every shaded vertex the uv comes from ``Geometry.interact``, the albedo a_k from
``read_bsdf`` and the weight w_k from ``sample_light`` of tests/texel_lighting_ref.py with the draws of the oracle's sampler dump; then

    Q_{n+1} = 0,  Q_k = A_k w_k + a_{k+1} Q_{k+1},  d a_k = gamma beta_{k-1} Q_k,  gamma = d_out[t].rgb / spp,

d a_k goes to the four taps of vertex k's lookup, and an accepted vertex whose sample came from the front of a mesh light adds
gamma beta_k c / max(pdf, 1e-4) to the row of the light's instance.  float64 is the truth the GPU tests compare with; float32, with every
target's terms added in ascending and in descending order, measures what float32 alone costs (MARGINS below).

``bake_eval`` is the polynomial itself: the bake as a function of float64 — or complex, for a complex-step derivative — materials and
emissions with the same records.  tests/test_texel_bounce_grad_ref_host.py pins the gradient by it.  A helper, not a test."""
import functools

import numpy as np

import texel_bounce_cases as BC
import texel_bounce_ref as BR
import texel_deep_cases as DC
import texel_lighting_grad_ref as LG
import texel_lighting_ref as LR

FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
COT_SEED = 23

# Per case (d_materials, d_emission): the larger error against float64 of the float32 reference with every target's terms added in
# ascending and in descending order, for the cotangent ``cotangent(name)`` on the float64 reference's own walks, rounded up in the third
# digit (python tools/texel_bounce_grad_margins.py; profiles/texel_bounce_grad_margins.txt; no GPU involved).
MARGINS = {
    "cbox_k1": (4.51e-07, 7.06e-08),
    "cbox_k3": (8.31e-07, 1.06e-07),
    "multi_k3": (3.00e-06, 5.99e-07),
    "env_k2": (1.23e-05, 0.0),
    "cbox_pmj02bn_k2": (1.36e-06, 7.92e-08),
    "cbox_k3_range": (7.26e-07, 4.51e-08),
    # BC.EDGE_CASES
    "hall_k2": (7.27e-06, 1.48e-07),
    "cbox_k8": (6.36e-07, 5.33e-08),
    "cbox_k8_pmj02bn": (8.31e-07, 4.99e-08),
    "cbox_wave": (1.70e-07, 6.42e-08),
    "cbox_wave_one": (6.12e-09, 3.15e-10),
    "cbox_wave_ragged": (8.35e-08, 1.05e-08),
    "cbox_wide": (3.80e-06, 7.76e-07),
    "tiny_1x1": (1.34e-05, 1.22e-07),
    "tiny_3x6": (1.57e-06, 1.68e-07),
    "tiny_4x5": (1.29e-06, 7.45e-08),
    "tiny_multi": (4.37e-06, 2.13e-07),
    "cbox_k3_nan": (8.31e-07, 1.13e-07),
    "env_lit_k2": (8.50e-06, 2.02e-07),
    **DC.BOUNCE_GRAD_MARGINS,                                         # BC.DEEP_CASES
}


def taps(h, w, uv):
    """read_bsdf's footprint at uv (N, 2) in a (h, w) material: -> (flat texel index (N, 4), weight (N, 4)) in the order c00, c01, c10, c11
    of csrc/scene.h — (1-ox)(1-oy), (1-ox) oy, ox (1-oy), ox oy — in uv's dtype; taps that the clamp puts on one texel stay two entries"""
    d = uv.dtype.type
    px, py = uv[:, 0] * d(w - 1), (d(1.0) - uv[:, 1]) * d(h - 1)
    ix, iy = np.trunc(px).astype(np.int64), np.trunc(py).astype(np.int64)
    ox, oy = (px - ix).astype(d), (py - iy).astype(d)
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    one = d(1.0)
    idx = np.stack([x0 + w * y0, x0 + w * y1, x1 + w * y0, x1 + w * y1], 1)
    k = np.stack([(one - ox) * (one - oy), (one - ox) * oy, ox * (one - oy), ox * oy], 1).astype(d)
    return idx, k


def records(arrays, texel_data, slots, hits, *, spp, bounces, seed=0, samples=None, sampler="cmj", env=None, tables=None, dtype=np.float64):
    """What the walks of ``hits`` — ``nvert`` (N,), ``inst``, ``prim``, ``flags`` (N, K), ``uv`` (N, K, 2), in the order of
    ``texel_bounce_ref``'s rows — leave per sample and vertex, in ``dtype``: ``shaded``, ``added`` (N, K) bool from the flags; ``slot`` (N, K)
    the material (-1: none); ``tuv`` (N, K, 2) the texture coordinates; ``ws`` (N, K) = c / max(pdf, 1e-4) of the vertex's light sample
    (0 where the vertex is not shaded); ``ev`` (N, K, 3) the sample's L.eval with the scene's own emissions; ``light`` (N, K) the
    instance of the mesh light the sample took from its front (-1: the environment, a back face or no sample).  And ``ys``, ``xs`` (T,) the
    shaded texels, ``ns`` the samples per texel, ``shape`` (H, W), ``spp``, ``ninst``."""
    dtype = np.dtype(dtype).type
    K = int(bounces)
    texel_data = np.asarray(texel_data)
    H, W = texel_data.shape[:2]
    begin, end = (0, spp) if samples is None else samples
    S = np.arange(begin, end)
    nrm_all, pos_all = texel_data[..., 4:7], texel_data[..., 8:11]
    shade = (texel_data[..., 12] == 1) & ~np.isnan(nrm_all).any(-1) & ~np.isnan(pos_all).any(-1)
    ys, xs = np.nonzero(shade)
    T, ns = ys.shape[0], S.shape[0]
    N = T * ns
    nvert, flags = np.asarray(hits["nvert"]), np.asarray(hits["flags"])
    assert nvert.shape == (N,) and flags.shape == (N, K), (nvert.shape, flags.shape, N, K)
    have = np.arange(K)[None, :] < nvert[:, None]
    rec = {"ys": ys, "xs": xs, "ns": ns, "shape": (H, W), "spp": int(spp), "ninst": int(arrays.ninst), "K": K,
           "shaded": have & ((flags & BR.F_SHADED) != 0), "added": have & ((flags & BR.F_ADDED) != 0),
           "slot": np.full((N, K), -1, np.int64), "tuv": np.zeros((N, K, 2), dtype), "ws": np.zeros((N, K), dtype),
           "ev": np.zeros((N, K, 3), dtype), "light": np.full((N, K), -1, np.int64)}
    assert not (rec["added"] & ~rec["shaded"]).any()
    slot_of_inst = np.array([-1 if k is None else int(k) for k in slots], np.int64)
    geo = BR.Geometry(arrays, dtype)
    lights = LR.light_table(arrays, dtype)
    insts = np.array(LG.light_instances(arrays), np.int64)
    env_count = 0 if env is None else 1
    nl = env_count + len(lights)
    u = BR.draws(LR.SAMPLER_KINDS[sampler], xs, ys, seed, spp, S, K, tables).reshape(N, 2 + 7 * K)
    for k in range(K):
        sel = np.nonzero(rec["shaded"][:, k])[0]
        if not sel.size:
            continue
        inst, prim = np.asarray(hits["inst"])[sel, k].astype(np.int64), np.asarray(hits["prim"])[sel, k].astype(np.int64)
        hu, hv = np.asarray(hits["uv"])[sel, k, 0].astype(np.float32), np.asarray(hits["uv"])[sel, k, 1].astype(np.float32)
        ip, iuv, ins, _ = geo.interact(inst, prim, hu, hv)
        rec["slot"][sel, k] = slot_of_inst[inst]
        rec["tuv"][sel, k] = iuv
        u6 = np.zeros((sel.size, 6), np.float32); u6[:, 2:6] = u[sel, 2 + 7 * k: 6 + 7 * k]
        wi, _, pdf, ev, _ = LR.sample_light(lights, env, ip, u6, dtype)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            ws = (BR._dot(ins, wi) / np.maximum(pdf, dtype(1e-4))).astype(dtype)
        rec["ws"][sel, k] = np.where(rec["added"][sel, k], ws, dtype(0.0))   # (a vertex that is not accepted carries no weight)
        rec["ev"][sel, k] = ev
        if nl:
            pick = np.clip((u6[:, 2].astype(dtype) * dtype(nl)).astype(np.int64), 0, nl - 1)
            mesh = (pick >= env_count) & (ev > 0).any(1)              # eval is the emission iff the sample left the light's front
            rec["light"][sel, k] = np.where(mesh, insts[np.clip(pick - env_count, 0, max(len(insts) - 1, 0))] if len(insts) else -1, -1)
    assert (rec["slot"][rec["shaded"]] >= 0).all()
    return rec


def _albedo(rec, materials, dtype, lookup):
    a = np.zeros(rec["shaded"].shape + (3,), dtype)
    for m, mat in enumerate(materials):
        for k in range(rec["K"]):
            sel = np.nonzero(rec["shaded"][:, k] & (rec["slot"][:, k] == m))[0]
            if sel.size:
                a[sel, k] = lookup(mat, rec["tuv"][sel, k])
    return a


def _weights(rec, emissions, dtype):
    """(N, K, 3): A_k w_k with the emissions ``emissions`` (ninst, 3) in place of the scene's own on the mesh lights"""
    ev = rec["ev"].astype(dtype)
    if emissions is not None:
        em = np.asarray(emissions).astype(dtype)
        ev = np.where((rec["light"] >= 0)[..., None], em[np.maximum(rec["light"], 0)], ev)
    return (ev * rec["ws"].astype(dtype)[..., None] * rec["added"][..., None]).astype(dtype)


def bake_eval(rec, materials, emissions=None):
    """The polynomial: (H, W, 3) irradiance = (1 / spp) sum over s, k of A_k beta_k w_k for ``materials`` (float64 or complex (h, w, 4)
    arrays) and ``emissions`` (None: the scene's own), with the records' hits, draws and decisions"""
    cplx = any(np.iscomplexobj(m) for m in materials) or (emissions is not None and np.iscomplexobj(emissions))
    dtype = np.complex128 if cplx else np.float64

    def lookup(mat, uv):
        idx, k = taps(mat.shape[0], mat.shape[1], uv.astype(np.float64))
        flat = np.asarray(mat)[..., :3].reshape(-1, 3).astype(dtype)
        return (flat[idx] * k[..., None]).sum(1)
    a = _albedo(rec, materials, dtype, lookup)
    w = _weights(rec, emissions, dtype)
    beta = np.ones((a.shape[0], 3), dtype)
    E = np.zeros((a.shape[0], 3), dtype)
    for k in range(rec["K"]):
        beta = np.where(rec["shaded"][:, k, None], beta * a[:, k], beta)
        E = E + beta * w[:, k]
    out = np.zeros(rec["shape"] + (3,), dtype)
    out[rec["ys"], rec["xs"]] = E.reshape(len(rec["ys"]), rec["ns"], 3).sum(1) / rec["spp"]
    return out


def _ordered_sum(n, target, value, dtype, order):
    """sums value[i] into out[target[i]] (n entries), in ``dtype``: ``order`` None — in float64, then rounded; "asc" / "desc" — one term
    after the other in the order of the rows / in the reverse order, every partial sum rounded to ``dtype``"""
    out = np.zeros(n, dtype)
    if target.size == 0:
        return out
    if order is None:
        acc = np.zeros(n, np.float64)
        np.add.at(acc, target, value.astype(np.float64))
        return acc.astype(dtype)
    if order == "desc":
        target, value = target[::-1], value[::-1]
    by = np.argsort(target, kind="stable")
    t, v = target[by], value[by].astype(dtype)
    first = np.r_[True, t[1:] != t[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(t.size), 0))
    rank = np.arange(t.size) - start
    rounds = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[rounds], np.arange(int(rank.max()) + 2))
    for r in range(len(bounds) - 1):                                  # round r: the r-th term of every target, all targets distinct
        sel = rounds[bounds[r]:bounds[r + 1]]
        out[t[sel]] = (out[t[sel]] + v[sel]).astype(dtype)
    return out


def texel_bounce_grad_ref(rec, materials, d_out, *, emissions=None, order=None):
    """The adjoint for the cotangent ``d_out`` (H, W, 4; float 3 and the texels that are not shaded are never read) in the records'
    dtype.  Returns ``d_materials``, a list of dense (h, w, 4) arrays (channel 3 stays 0), ``d_emission`` (ninst, 3), ``read``, a list of
    (h, w) bool — the texels a shaded vertex reads —, and ``n_terms``.  ``order``: see _ordered_sum."""
    dtype = rec["ws"].dtype.type
    K, T, ns = rec["K"], len(rec["ys"]), rec["ns"]
    a = _albedo(rec, materials, dtype, lambda mat, uv: BR.read_bsdf(np.asarray(mat, np.float32), uv, dtype))
    w = _weights(rec, emissions, dtype)
    g = np.repeat(np.asarray(d_out)[rec["ys"], rec["xs"], :3].astype(dtype), ns, axis=0)
    gamma = (g * (dtype(1.0) / dtype(rec["spp"]))).astype(dtype)
    N = T * ns
    with np.errstate(over="ignore", invalid="ignore"):
        Q = np.zeros((N, K, 3), dtype)
        q, a_next = np.zeros((N, 3), dtype), np.zeros((N, 3), dtype)
        for k in range(K - 1, -1, -1):
            q = (w[:, k] + a_next * q).astype(dtype)
            Q[:, k] = q
            a_next = a[:, k]
        da = np.zeros((N, K, 3), dtype)
        bprev = gamma.copy()                                          # gamma beta_{k-1}
        eterm = np.zeros((N, K, 3), dtype)
        for k in range(K):
            da[:, k] = (bprev * Q[:, k]).astype(dtype)
            bprev = np.where(rec["shaded"][:, k, None], bprev * a[:, k], bprev).astype(dtype)
            eterm[:, k] = (bprev * rec["ws"][:, k, None]).astype(dtype)   # gamma beta_k c / max(pdf, 1e-4)
    push = rec["shaded"] & np.isfinite(da).all(-1)                    # a term that is not finite is dropped
    d_materials, read = [], []
    n_terms = 0
    for m, mat in enumerate(materials):
        h, wd = mat.shape[:2]
        tg, val = [[] for _ in range(3)], [[] for _ in range(3)]
        rd = np.zeros(h * wd, bool)
        nn, kk = np.nonzero(push & (rec["slot"] == m))                # rows: sample-major, vertices ascending within a sample
        rn, rk = np.nonzero(rec["shaded"] & (rec["slot"] == m))
        if rn.size:
            rd[taps(h, wd, rec["tuv"][rn, rk])[0].reshape(-1)] = True
        dm = np.zeros((h, wd, 4), dtype)
        if nn.size:
            idx, kw = taps(h, wd, rec["tuv"][nn, kk])
            for ch in range(3):
                v = (kw * da[nn, kk, ch][:, None]).astype(dtype)
                dm[..., ch] = _ordered_sum(h * wd, idx.reshape(-1), v.reshape(-1), dtype, order).reshape(h, wd)
            n_terms += idx.size
        d_materials.append(dm); read.append(rd.reshape(h, wd))
    d_emission = np.zeros((rec["ninst"], 3), dtype)
    nn, kk = np.nonzero(rec["added"] & (rec["light"] >= 0) & np.isfinite(eterm).all(-1))
    for ch in range(3):
        d_emission[:, ch] = _ordered_sum(rec["ninst"], rec["light"][nn, kk], eterm[nn, kk, ch], dtype, order)
    return {"d_materials": d_materials, "d_emission": d_emission, "read": read, "n_terms": n_terms + nn.size}


# ------------------------------------------------------------------------------------ the cases of tests/texel_bounce_cases.py
def cotangent(name):
    """the case's seeded cotangent (H, W, 4) float32, uniform in [-1, 1): NaN in channel 3 and in every texel that is not shaded"""
    H, W = BC.case(name)[2]
    rng = np.random.default_rng(COT_SEED)
    g = rng.uniform(-1.0, 1.0, (H, W, 4)).astype(np.float32)
    g[..., 3] = np.nan
    g[~BC.reached(name)] = np.nan
    return g


def case_records(name, hits, dtype="float64", K=None, samples=None):
    make, slots, _, _, spp, case_K, env, _ = BC.case(name)
    pmj = name in BC.SAMPLERS
    return records(make(), BC.points(name), slots, hits, spp=spp, bounces=case_K if K is None else K, seed=BC.SEED,
                   samples=BC.RANGES.get(name) if samples is None else samples, sampler="pmj02bn" if pmj else "cmj", env=env() if env else None,
                   tables=BC.pmj_tables(name) if pmj else None, dtype=np.dtype(dtype).type)


@functools.lru_cache(None)
def reference_records(name, dtype="float64"):
    """the records of the free-running float64 reference's own walks (BC.reference), in ``dtype``; shared: read-only"""
    return case_records(name, BC.reference(name), dtype)


@functools.lru_cache(None)
def reference_grad(name):
    """the float64 gradient on the float64 reference's own walks for ``cotangent(name)``; shared: read-only"""
    return texel_bounce_grad_ref(reference_records(name), BC.materials(name), cotangent(name))


def light_rows(name):
    return LG.light_instances(BC.case(name)[0]())


def margin(name):
    """((error d_materials, error d_emission), (largest |entry| d_materials, d_emission)) of the float32 reference, the larger of both
    summation orders, against float64"""
    ref = reference_grad(name)
    r32 = reference_records(name, "float32")
    em, ee = 0.0, 0.0
    for order in ("asc", "desc"):
        g = texel_bounce_grad_ref(r32, BC.materials(name), cotangent(name), order=order)
        em = max([em] + [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(g["d_materials"], ref["d_materials"])])
        ee = max(ee, float(np.abs(g["d_emission"].astype(np.float64) - ref["d_emission"]).max()))
    return (em, ee), scales(ref)


def scales(grad):
    return max(float(np.abs(d).max()) for d in grad["d_materials"]), float(np.abs(grad["d_emission"]).max())


def bars(name, grad=None):
    """(bar of d_materials, bar of d_emission): max(4 x margin, 4 float32 ulps of the case's largest entry)"""
    sm, se = scales(reference_grad(name) if grad is None else grad)
    return max(4.0 * MARGINS[name][0], FLOOR_ULPS * EPS32 * sm), max(4.0 * MARGINS[name][1], FLOOR_ULPS * EPS32 * se)


def table_lines(names=None):
    lines = [f"float32 reference of the adjoint against the float64 reference (tests/texel_bounce_grad_ref.py; no GPU involved), seed {BC.SEED}, "
             f"cotangent seed {COT_SEED}: the larger error of ascending and descending summation per target"]
    for name in (BC.CASES if names is None else names):
        (em, ee), (sm, se) = margin(name)
        lines.append(f"  {name:16s} terms {reference_grad(name)['n_terms']:7d}  d_materials: largest entry {sm:.4e} error {em:.3e} ({em / sm:.2e} of it)  "
                     f"d_emission: largest entry {se:.4e} error {ee:.3e}" + (f" ({ee / se:.2e} of it)" if se > 0 else ""))
    return lines
