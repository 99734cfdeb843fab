"""Reference of the adjoint of the bounced light in the environment map (include/zdr.h, zdr_scene_texel_bounce_backward_env) in NumPy, for
any float dtype, on GIVEN hits and decisions — built on ``texel_bounce_grad_ref.records`` (the walks' records: shaded, added, albedo
lookups, ws = c / max(pdf, 1e-4)), ``texel_lighting_grad_ref.env_sample_uv`` / ``env_taps`` (where an environment sample reads the map)
and ``texel_bounce_ref.draws``.  Nothing is traced.

An accepted vertex k whose light sample came from the map forms term = (gamma beta_k) ws, gamma = d_out[t].rgb / spp, and adds k_m term to
the four taps of the map's bilinear lookup.  float64 is the truth the GPU tests compare with; float32, with every map texel's terms added
in ascending and in descending order, measures what float32 alone costs (MARGINS below).

``bake_eval`` is the bake as a function of the MAP with the same records: an environment sample takes L.eval from a bilinear lookup of
the map it is given.  The bake is linear in the map, so <d_out, eval(env + delta) - eval(env)> = <d_env, delta> exactly;
tests/test_texel_bounce_envgrad_host.py pins the gradient by it.  A helper, not a test."""
import functools

import numpy as np

import texel_bounce_env_cases as EC
import texel_bounce_grad_ref as GR
import texel_bounce_ref as BR
import texel_deep_cases as DC
import texel_lighting_grad_ref as LG
import texel_lighting_ref as LR

FLOOR_ULPS = 4
EPS32 = 2.0 ** -24
COT_SEED = 23

# Per case: the larger error against float64 of the float32 reference with every map texel's terms added in ascending and in descending
# order, for the cotangent ``cotangent(name)`` on the float64 reference's own walks, rounded up in the third digit
# (python tools/texel_bounce_envgrad_margins.py; profiles/texel_bounce_envgrad_margins.txt; no GPU involved).
MARGINS = {
    "env_k2": 4.01e-08,
    "env_lit_k2": 1.90e-08,
    "env_k2_pmj02bn": 2.20e-08,
    "env_k2_range": 3.56e-08,
    "env_k3": 4.02e-08,
    "env_wave": 5.80e-09,
    "env_wave_ragged": 5.02e-09,
    "env_sky": 1.76e-07,
}
DEEP_MARGINS = DC.BOUNCE_ENVGRAD_MARGINS      # the same for EC.DEEP_CASES (tests/texel_deep_cases.py): a table of its own, as the cases are


def margin_of(name):
    """the table's margin of a case of EC.CASES or of EC.DEEP_CASES"""
    return MARGINS[name] if name in MARGINS else DEEP_MARGINS[name]


def env_records(arrays, texel_data, slots, hits, *, spp, bounces, seed=0, samples=None, sampler="cmj", env, tables=None, dtype=np.float64):
    """``texel_bounce_grad_ref.records`` and, per sample and vertex, what the environment branch of the vertex's light sample reads:
    ``is_env`` (N, K) bool — the vertex is shaded and its light sample went to the map (accepted or not) — and ``euv`` (N, K, 2), the
    map coordinates of that sample in ``dtype``."""
    dtype = np.dtype(dtype).type
    rec = GR.records(arrays, texel_data, slots, hits, spp=spp, bounces=bounces, seed=seed, samples=samples, sampler=sampler, env=env, tables=tables, dtype=dtype)
    K, N = rec["K"], rec["shaded"].shape[0]
    begin, end = (0, spp) if samples is None else samples
    u = BR.draws(LR.SAMPLER_KINDS[sampler], rec["xs"], rec["ys"], seed, spp, np.arange(begin, end), K, tables).reshape(N, 2 + 7 * K)
    nl = 1 + len(LR.light_table(arrays, dtype))
    rec["is_env"] = np.zeros((N, K), bool)
    rec["euv"] = np.zeros((N, K, 2), dtype)
    for k in range(K):
        sel = np.nonzero(rec["shaded"][:, k])[0]
        if not sel.size:
            continue
        u6 = np.zeros((sel.size, 6), np.float32); u6[:, 2:6] = u[sel, 2 + 7 * k: 6 + 7 * k]
        pick = np.clip((u6[:, 2].astype(dtype) * dtype(nl)).astype(np.int64), 0, nl - 1)
        uu, vv, _ = LG.env_sample_uv(env, u6, dtype)
        rec["is_env"][sel, k] = pick < 1
        rec["euv"][sel, k, 0], rec["euv"][sel, k, 1] = uu, vv
    rec["env_shape"] = tuple(env[0].shape[:2])
    return rec


def accepted_env(rec):
    """(N, K) bool: the accepted environment samples"""
    return rec["added"] & rec["is_env"]


def cells(rec):
    """(N, K) int: the merge's cell key (cy + 1)(env_w + 1) + (cx + 1) of every sample's footprint, and cx, cy (base texel in -1 .. W - 1)"""
    eh, ew = rec["env_shape"]
    d = rec["euv"].dtype.type
    cx = np.clip(np.floor(rec["euv"][..., 0] * d(ew) - d(0.5)).astype(np.int64), -1, ew - 1)
    cy = np.clip(np.floor(rec["euv"][..., 1] * d(eh) - d(0.5)).astype(np.int64), -1, eh - 1)
    return (cy + 1) * (ew + 1) + (cx + 1), cx, cy


def _betas(rec, materials, dtype, lookup):
    """(N, K, 3): beta_k, the product of the albedos of the shaded vertices up to and including k"""
    a = GR._albedo(rec, materials, dtype, lookup)
    beta = np.ones((a.shape[0], 3), dtype)
    out = np.zeros(a.shape, dtype)
    for k in range(rec["K"]):
        beta = np.where(rec["shaded"][:, k, None], (beta * a[:, k]).astype(dtype), beta)
        out[:, k] = beta
    return out


def texel_bounce_envgrad_ref(rec, materials, d_out, *, order=None):
    """The adjoint for the cotangent ``d_out`` (H, W, 4; float 3 and the texels that are not shaded are never read) in the records' dtype.
    Returns ``d_env`` (h, w, 4; alpha stays 0), ``read`` (h, w) bool — the map texels an accepted environment sample's footprint touches —,
    ``count`` (h, w) — the terms per map texel —, ``n_samples`` — the accepted environment samples whose term is finite — and ``n_terms``.
    ``order``: see texel_bounce_grad_ref._ordered_sum."""
    dtype = rec["ws"].dtype.type
    eh, ew = rec["env_shape"]
    ns = rec["ns"]
    beta = _betas(rec, materials, dtype, lambda mat, uv: BR.read_bsdf(np.asarray(mat, np.float32), uv, dtype))
    g = np.repeat(np.asarray(d_out)[rec["ys"], rec["xs"], :3].astype(dtype), ns, axis=0)
    gamma = (g * (dtype(1.0) / dtype(rec["spp"]))).astype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        term = ((gamma[:, None, :] * beta).astype(dtype) * rec["ws"][..., None]).astype(dtype)
    take = accepted_env(rec) & np.isfinite(term).all(-1)              # a term that is not finite is dropped
    nn, kk = np.nonzero(take)                                         # rows: sample-major, vertices ascending within a sample
    d_env = np.zeros((eh, ew, 4), dtype)
    read = np.zeros(eh * ew, bool)
    count = np.zeros(eh * ew, np.int64)
    if nn.size:
        ty, tx, kw = LG.env_taps((eh, ew), rec["euv"][nn, kk, 0], rec["euv"][nn, kk, 1], dtype)
        flat = (ty * ew + tx).reshape(-1)
        read[flat] = True
        count = np.bincount(flat, minlength=eh * ew)
        for ch in range(3):
            v = (kw * term[nn, kk, ch][:, None]).astype(dtype)
            d_env[..., ch] = GR._ordered_sum(eh * ew, flat, v.reshape(-1), dtype, order).reshape(eh, ew)
    return {"d_env": d_env, "read": read.reshape(eh, ew), "count": count.reshape(eh, ew), "n_samples": int(nn.size), "n_terms": int(4 * nn.size)}


def bake_eval(rec, materials, env_tex):
    """The bake as a function of the map: (H, W, 3) float64 irradiance = (1 / spp) sum over s, k of A_k beta_k L.eval_k ws_k with the
    records' hits, draws and decisions, where an environment sample's L.eval is the bilinear lookup of ``env_tex`` (h, w, 3|4) and a mesh
    light's is the records' own"""
    dtype = np.float64
    tex = np.asarray(env_tex, dtype)[..., :3].reshape(-1, 3)
    eh, ew = rec["env_shape"]

    def lookup(mat, uv):
        idx, k = GR.taps(mat.shape[0], mat.shape[1], uv.astype(np.float64))
        flat = np.asarray(mat)[..., :3].reshape(-1, 3).astype(dtype)
        return (flat[idx] * k[..., None]).sum(1)
    beta = _betas(rec, materials, dtype, lookup)
    ev = rec["ev"].astype(dtype).copy()
    nn, kk = np.nonzero(rec["is_env"])
    if nn.size:
        ty, tx, kw = LG.env_taps((eh, ew), rec["euv"][nn, kk, 0].astype(dtype), rec["euv"][nn, kk, 1].astype(dtype), dtype)
        ev[nn, kk] = (tex[ty * ew + tx] * kw[..., None]).sum(1)
    E = (beta * ev * (rec["ws"].astype(dtype) * rec["added"])[..., None]).sum(1)
    out = np.zeros(rec["shape"] + (3,), dtype)
    out[rec["ys"], rec["xs"]] = E.reshape(len(rec["ys"]), rec["ns"], 3).sum(1) / rec["spp"]
    return out


def wave_groups(rec, name):
    """How the kernel's waves see the accepted environment samples (with a finite term this reference cannot tell apart: all of them):
    per (wave, trip, vertex index) the number of samples and of distinct cells.  -> list of (samples, distinct cells, largest number of
    samples in one cell).  Texels are taken in row-major order (the kernel's list may order them differently: the per-wave figures are
    those of one possible order, the per-texel ones do not depend on it)."""
    shift = EC.lanes_shift(name)
    lanes = 1 << shift
    per_wave = EC.WAVE // lanes
    key, _, _ = cells(rec)
    acc = accepted_env(rec)
    T, ns, K = len(rec["ys"]), rec["ns"], rec["K"]
    key, acc = key.reshape(T, ns, K), acc.reshape(T, ns, K)
    out = []
    for t0 in range(0, T, per_wave):
        for trip in range((ns + lanes - 1) // lanes):
            s0, s1 = trip * lanes, min((trip + 1) * lanes, ns)
            for k in range(K):
                m = acc[t0:t0 + per_wave, s0:s1, k]
                if m.any():
                    _, counts = np.unique(key[t0:t0 + per_wave, s0:s1, k][m], return_counts=True)
                    out.append((int(m.sum()), int(counts.size), int(counts.max())))
    return out


def expected_groups(rec, name):
    """the header's word 2 for the row-major order of the texels: per (wave, trip, vertex index) min(cells, rounds) merged groups plus the
    samples of the cells beyond the rounds — cells are taken in the order of their first lane"""
    shift = EC.lanes_shift(name)
    lanes = 1 << shift
    per_wave = EC.WAVE // lanes
    key, _, _ = cells(rec)
    acc = accepted_env(rec)
    T, ns, K = len(rec["ys"]), rec["ns"], rec["K"]
    key, acc = key.reshape(T, ns, K), acc.reshape(T, ns, K)
    groups = 0
    for t0 in range(0, T, per_wave):
        for trip in range((ns + lanes - 1) // lanes):
            s0, s1 = trip * lanes, min((trip + 1) * lanes, ns)
            for k in range(K):
                m = acc[t0:t0 + per_wave, s0:s1, k].reshape(-1)
                kk = key[t0:t0 + per_wave, s0:s1, k].reshape(-1)[m]
                seen = []
                for c in kk:
                    if c not in seen:
                        seen.append(c)
                merged = seen[:EC.MERGE_ROUNDS]
                groups += len(merged) + int(sum(1 for c in kk if c not in merged))
    return groups


# ------------------------------------------------------------------------------------ the cases of tests/texel_bounce_env_cases.py
def cotangent(name):
    """the case's seeded cotangent (H, W, 4) float32, uniform in [-1, 1): NaN in channel 3 and in every texel that is not shaded"""
    H, W = EC.case(name)["hw"]
    rng = np.random.default_rng(COT_SEED)
    g = rng.uniform(-1.0, 1.0, (H, W, 4)).astype(np.float32)
    g[..., 3] = np.nan
    g[~EC.reached(name)] = np.nan
    return g


def case_records(name, hits, dtype="float64", K=None, samples=None):
    c = EC.case(name)
    return env_records(c["make"](), EC.points(name), c["slots"], hits, spp=c["spp"], bounces=c["K"] if K is None else K, seed=EC.SEED,
                       samples=c["samples"] if samples is None else samples, sampler=EC.sampler(name), env=EC.env(name), tables=EC.tables(name),
                       dtype=np.dtype(dtype).type)


@functools.lru_cache(None)
def reference_records(name, dtype="float64"):
    """the records of the free-running float64 reference's own walks (EC.reference), in ``dtype``; shared: read-only"""
    return case_records(name, EC.reference(name), dtype)


@functools.lru_cache(None)
def reference_grad(name):
    """the float64 gradient on the float64 reference's own walks for ``cotangent(name)``; shared: read-only"""
    return texel_bounce_envgrad_ref(reference_records(name), EC.materials(name), cotangent(name))


def margin(name):
    """(error, largest |entry|) of the float32 reference, the larger of both summation orders, against float64"""
    ref = reference_grad(name)
    r32 = reference_records(name, "float32")
    e = 0.0
    for order in ("asc", "desc"):
        g = texel_bounce_envgrad_ref(r32, EC.materials(name), cotangent(name), order=order)
        e = max(e, float(np.abs(g["d_env"].astype(np.float64) - ref["d_env"]).max()))
    return e, scale(ref)


def scale(grad):
    return float(np.abs(grad["d_env"]).max())


def bar(name, grad=None):
    """max(4 x margin, 4 float32 ulps of the case's largest entry): the rule of texel_bounce_grad_ref.bars"""
    return max(4.0 * margin_of(name), FLOOR_ULPS * EPS32 * scale(reference_grad(name) if grad is None else grad))


def table_lines(names=None):
    lines = [f"float32 reference of the adjoint in the environment map against the float64 reference (tests/texel_bounce_envgrad_ref.py; no GPU involved), "
             f"seed {EC.SEED}, cotangent seed {COT_SEED}: the larger error of ascending and descending summation"]
    for name in (EC.CASES if names is None else names):
        e, s = margin(name)
        rec = reference_records(name)
        per_k = accepted_env(rec).sum(0)
        lines.append(f"  {name:16s} walks {rec['shaded'].shape[0]:5d}  accepted environment samples per vertex {[int(v) for v in per_k]}  map texels with a term "
                     f"{int(reference_grad(name)['read'].sum()):4d}  d_env: largest entry {s:.4e} error {e:.3e} ({e / s:.2e} of it)")
    return lines
