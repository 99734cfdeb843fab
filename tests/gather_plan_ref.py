"""Reference of the gather plan (include/zdr.h, zdr_gather_plan_*) in NumPy: ``plan_ref`` enumerates the entries of the three filters in
float32, operation for operation as the header states them, and lays them out as CSR rows; ``apply_ref`` sums the rows, in float32 in
the header's order (sixteen sub-sums, then the tree) or plainly in float64.

Built on tests/texel_mip_ref.py (the pyramid's layout) and tests/texel_aniso_ref.py (the probes), neither of which is modified.  One
operation of the enumeration is not IEEE: the level fraction f = log2f(mantissa), which the kernels take from the GPU's own log2f and
whose last bit differs from NumPy's.  ``plan_ref`` therefore takes the function as ``log2`` (float32 array -> float32 array): the host
tests leave NumPy's, the GPU tests hand in the GPU's (read back through zdr_texel_gather_mip, which returns f itself for a view and an
image made for that), so that the weights can be compared bit for bit.  A helper, not a test; tests/test_gather_plan_host.py pins it."""
import numpy as np

import texel_aniso_ref as AR
import texel_mip_ref as MR

F = np.float32
FILTERS = ("bilinear", "mip", "aniso")


def numpy_log2(m):
    return np.log2(m.astype(F)).astype(F)


def level_split32(s, L, log2=numpy_log2):
    """(l0 int64, f float32) of s (float32), as the kernels split it: s = max(s, 1), NaN -> 1; the exponent and the mantissa from the bits"""
    s = np.asarray(s, F)
    with np.errstate(invalid="ignore"):
        s = np.where(s > 1, s, F(1.0)).astype(F)
    b = s.view(np.uint32)
    l0 = (b >> 23).astype(np.int64) - 127
    m = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(F)
    f = np.zeros(s.shape, F)
    k = np.nonzero((m != 1) & (l0 < L))[0]
    if k.size:
        f[k] = np.fmin(np.asarray(log2(m[k]), F), F(1.0))
    top = l0 >= L
    return np.where(top, L, l0), np.where(top, F(0.0), f).astype(F)


def taps32(X, Y, w, h):
    """tf_taps (csrc/texel_filter.h) in float32: ((i00, i01, i10, i11) int64, tx, ty); a NaN or an infinity ends inside the level, as in the kernels"""
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = (X - F(0.5)).astype(F), (Y - F(0.5)).astype(F)
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = (fx - x0f).astype(F), (fy - y0f).astype(F)
        x0 = np.fmin(np.fmax(x0f, F(-1.0)), F(w)).astype(np.int64)
        y0 = np.fmin(np.fmax(y0f, F(-1.0)), F(h)).astype(np.int64)
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    return (ya * w + xa, ya * w + xb, yb * w + xa, yb * w + xb), tx, ty


def rows_of(res, filter, levels=0):
    """(P0, P): the rows of level 0 and of the whole plan; the packed pyramid counts one pixel where it has no level"""
    p0 = int(res[0]) * int(res[1])
    if filter == "bilinear":
        return p0, p0
    return p0, p0 + max(sum(w * h for w, h, _ in MR.layout(res, levels)[1:]), 1)


def plan_ref(view, fp, res, filter, footprint=1.0, max_aniso=8, levels=0, log2=numpy_log2):
    """The plan of one gather: a dict with ``p0``, ``rows``, ``nnz``, the entries in entry-id order (``id_row``, ``id_texel``,
    ``id_weight``) and the CSR layout (``row_start`` (rows + 1,) int64, ``texel`` (nnz,) int64, ``weight`` (nnz,) float32, ``row`` (nnz,)).
    ``view``: (..., 8); ``fp``: the footprint buffer (..., 4), read for "aniso" only."""
    assert filter in FILTERS
    w, h = int(res[0]), int(res[1])
    v = np.asarray(view, F).reshape(-1, 8)
    n = v.shape[0]
    p0, rows = rows_of(res, filter, levels)
    lay = MR.layout(res, levels) if filter != "bilinear" else [(w, h, None)]
    L = len(lay) - 1
    on = (v[:, 0] != 0) & ~np.isnan(v[:, 0])
    fpt = F(footprint)
    N, l0, fr = np.ones(n, np.int64), np.zeros(n, np.int64), np.zeros(n, F)
    ax, ay = np.zeros(n, F), np.zeros(n, F)
    with np.errstate(invalid="ignore", over="ignore"):
        if filter == "mip":
            l0, fr = level_split32((v[:, 6] * fpt).astype(F), L, log2)
        elif filter == "aniso":
            f4 = np.asarray(fp, F).reshape(-1, 4)
            N, s = AR.probes(f4, footprint, max_aniso, F)
            l0, fr = level_split32((s.astype(F) * F(1.0)).astype(F), L, log2)
            ax, ay = f4[:, 0], f4[:, 1]
    one = F(1.0)
    parts = []                                                       # (texel, slot, row, weight)
    for i in range(int(N[on].max()) if on.any() else 0):
        k = np.nonzero(on & (N > i))[0]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            fN = N[k].astype(F)
            inv_n = (one / fN).astype(F)
            X, Y = v[k, 2], v[k, 3]
            if filter == "aniso":
                ti = ((2 * i + 1 - N[k]).astype(F) / (F(2.0) * fN).astype(F)).astype(F)
                tf = (ti * fpt).astype(F)
                X, Y = (X + (tf * ax[k]).astype(F)).astype(F), (Y + (tf * ay[k]).astype(F)).astype(F)
            for upper in (0, 1):
                lev = l0[k] + upper
                sel = np.ones(k.size, bool) if not upper else fr[k] != 0
                share = (one - fr[k]).astype(F) if not upper else fr[k]
                for l in np.unique(lev[sel]):
                    j = np.nonzero(sel & (lev == l))[0]
                    wl, hl, off = lay[int(l)]
                    idx, tx, ty = taps32(np.ldexp(X[j], -int(l)).astype(F), np.ldexp(Y[j], -int(l)).astype(F), wl, hl)
                    ux, uy = (one - tx).astype(F), (one - ty).astype(F)
                    first = 0 if l == 0 else p0 + off
                    for tap, (ix, wt) in enumerate(zip(idx, (ux * uy, tx * uy, ux * ty, tx * ty))):
                        wgt = ((((wt.astype(F) * share[j]).astype(F) * inv_n[j]).astype(F)) * v[k[j], 0]).astype(F)
                        parts.append((k[j], np.full(j.size, (i * 2 + upper) * 4 + tap, np.int64), first + ix, wgt))
    if parts:
        texel, slot, row, weight = (np.concatenate([p[c] for p in parts]) for c in range(4))
        order = np.lexsort((slot, texel))                            # entry-id order: texel-major, then the kernel's tap order
        texel, row, weight = texel[order], row[order], weight[order]
    else:
        texel, row, weight = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F)
    assert row.size == 0 or (row.min() >= 0 and row.max() < rows)
    by_row = np.argsort(row, kind="stable")
    row_start = np.searchsorted(row[by_row], np.arange(rows + 1), side="left").astype(np.int64)
    return {"p0": p0, "rows": rows, "nnz": int(row.size), "id_row": row, "id_texel": texel, "id_weight": weight,
            "row_start": row_start, "texel": texel[by_row], "weight": weight[by_row], "row": row[by_row]}


def sum16(p):
    """one row, (R, C) float32 products in entry order -> (C,) float32: sixteen sub-sums s_j over k = j, j + 16, ..., then the tree"""
    p = np.asarray(p, F)
    s = np.zeros((16,) + p.shape[1:], F)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, p.shape[0], 16):
            c = p[k0:k0 + 16]
            s[:c.shape[0]] = (s[:c.shape[0]] + c).astype(F)
        for half in (8, 4, 2, 1):
            s = (s[:half] + s[half:2 * half]).astype(F)
    return s[0]


def apply_ref(plan, d_color, dtype=np.float32):
    """the row sums of a plan, (rows, 4) in ``dtype``: float32 in the header's order (the product rounded, then the add), float64 plain.
    What zdr_gather_plan_apply adds into d_image (rows < p0 that are not empty) and writes to d_pyramid (rows >= p0)."""
    dtype = np.dtype(dtype).type
    g = np.asarray(d_color).reshape(-1, 4)
    rows, row, texel = plan["rows"], plan["row"], plan["texel"]
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype is np.float64:
            out = np.zeros((rows, 4), np.float64)
            np.add.at(out, row, plan["weight"].astype(np.float64)[:, None] * g[texel].astype(np.float64))
            return out
        prod = (plan["weight"][:, None] * g[texel].astype(F)).astype(F)
        pos = np.arange(row.size) - plan["row_start"][row]
        j, step = pos % 16, pos // 16
        S = np.zeros((rows, 16, 4), F)
        for st in range(int(step.max()) + 1 if row.size else 0):       # (a (row, j) pair occurs once per step: the indexed add is safe)
            k = np.nonzero(step == st)[0]
            S[row[k], j[k]] = (S[row[k], j[k]] + prod[k]).astype(F)
        for half in (8, 4, 2, 1):
            S = (S[:, :half] + S[:, half:2 * half]).astype(F)
    return S[:, 0]


def counts(plan):
    return np.diff(plan["row_start"])
