"""Reference of the prefiltered gather (include/zdr.h: zdr_image_pyramid, zdr_image_pyramid_backward, zdr_texel_gather_mip,
zdr_texel_gather_mip_backward) in NumPy, for any float dtype: float64 is the truth the GPU tests compare with, float32 — the header's
operation order step by step — is what the pyramid and its adjoint must equal bit for bit, and measures what float32 alone costs the
gather (tests/texel_project_cases.py, ``linear_bar``'s rule, turns that into the bars).

The per-level bilinear sample is ``texel_project_ref.taps`` / ``gather_ref`` on a view whose X, Y are scaled by 2^-level (exact in
either dtype).  A helper, not a test; tests/test_texel_mip_ref_host.py pins it."""
import numpy as np

import texel_project_ref as PR

F32 = np.float32


def layout(res, levels=0):
    """[(width, height, offset in pixels of the packed buffer; None for level 0)], level 0 first"""
    w, h = int(res[0]), int(res[1])
    out, off = [(w, h, None)], 0
    while (w > 1 or h > 1) and (levels <= 0 or len(out) - 1 < levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h, off))
        off += w * h
    return out


def pack(levels):
    """the levels >= 1 of a list [level 0, level 1, ...] one after another: (pixels, 4); one row of zeros if there is none"""
    if len(levels) == 1:
        return np.zeros((1, 4), levels[0].dtype)
    return np.concatenate([v.reshape(-1, 4) for v in levels[1:]], 0)


def unpack(packed, res, levels=0):
    """the list [None, level 1, ...] of a packed buffer"""
    packed = np.asarray(packed).reshape(-1, 4)
    return [None] + [packed[off:off + w * h].reshape(h, w, 4) for w, h, off in layout(res, levels)[1:]]


def pyramid_ref(image, levels=0, dtype=np.float64):
    """[level 0 .. level L] in ``dtype``: ((a00 + a01) + (a10 + a11)) * 0.25 over the border-continued finer level"""
    dtype = np.dtype(dtype).type
    out = [np.asarray(image).astype(dtype)]
    for w, h, _ in layout((out[0].shape[1], out[0].shape[0]), levels)[1:]:
        f = out[-1]
        hf, wf = f.shape[:2]
        y0, x0 = 2 * np.arange(h), 2 * np.arange(w)
        y1, x1 = np.minimum(y0 + 1, hf - 1), np.minimum(x0 + 1, wf - 1)
        with np.errstate(invalid="ignore", over="ignore"):
            top = (f[y0][:, x0] + f[y0][:, x1]).astype(dtype)
            bot = (f[y1][:, x0] + f[y1][:, x1]).astype(dtype)
            out.append(((top + bot).astype(dtype) * dtype(0.25)).astype(dtype))
    return out


def coef(w, h, dtype):
    """(h, w): 0.25 m(y, x), m = 2 per axis at the last index of an odd size"""
    mx, my = np.ones(w, dtype), np.ones(h, dtype)
    if w & 1:
        mx[-1] = 2
    if h & 1:
        my[-1] = 2
    return (dtype(0.25) * (my[:, None] * mx[None, :])).astype(dtype)


def pyramid_adjoint_ref(G, res, levels=0, dtype=np.float64):
    """what zdr_image_pyramid_backward ADDS to d_image, (height, width, 4) in ``dtype``; G: [None, G_1 .. G_L] or the packed buffer"""
    dtype = np.dtype(dtype).type
    lay = layout(res, levels)
    if not isinstance(G, list):
        G = unpack(G, res, levels)
    L = len(lay) - 1
    if L == 0:
        return np.zeros((int(res[1]), int(res[0]), 4), dtype)
    T = G[L].astype(dtype)
    for l in range(L - 1, -1, -1):
        w, h, _ = lay[l]
        ys, xs = np.arange(h) >> 1, np.arange(w) >> 1
        up = (coef(w, h, dtype)[..., None] * T[ys][:, xs]).astype(dtype)
        T = up if l == 0 else (G[l].astype(dtype) + up).astype(dtype)
    return T


def level_split(scale, footprint, L, dtype=np.float64):
    """(l0 int64, f ``dtype``) of each scale: s = max(scale footprint, 1), NaN -> 1; l0 = its binary exponent, f = log2 of the mantissa in
    [1, 2) (0 by selection where it is 1, at most 1); l0 >= L: (L, 0)"""
    dtype = np.dtype(dtype).type
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.asarray(scale).astype(dtype) * dtype(F32(footprint))).astype(dtype)
        s = np.where(s > 1, s, dtype(1.0)).astype(dtype)
    mant, e = np.frexp(np.where(np.isinf(s), dtype(1.0), s))
    l0 = np.where(np.isinf(s), 1 << 20, e.astype(np.int64) - 1)
    m = (mant * dtype(2.0)).astype(dtype)
    f = np.where(m == 1, dtype(0.0), np.minimum(np.log2(m).astype(dtype), dtype(1.0))).astype(dtype)
    top = l0 >= L
    return np.where(top, L, l0), np.where(top, dtype(0.0), f).astype(dtype)


def _level_views(view, footprint, L, dtype):
    """per texel: on, visible, l0, f, and a function level -> (texel indices that sample it as lower / upper level, their sub-view)"""
    v = np.asarray(view).reshape(-1, 8)
    on = (v[:, 0] != 0) & ~np.isnan(v[:, 0])
    l0, f = level_split(v[:, 6], footprint, L, dtype)

    def sub(k, l):
        s = np.zeros((k.size, 1, 8), np.float64)
        s[:, 0, 0] = 1.0
        s[:, 0, 2] = np.ldexp(v[k, 2].astype(np.float64), -l); s[:, 0, 3] = np.ldexp(v[k, 3].astype(np.float64), -l)
        return s
    return v, on, l0, f, sub


def gather_mip_ref(image, view, footprint=1.0, levels=0, dtype=np.float64, pyramid=None):
    """zdr_texel_gather_mip in ``dtype``: (H, W, 4).  ``pyramid``: the list of levels to read (default: ``pyramid_ref`` in ``dtype``)"""
    dtype = np.dtype(dtype).type
    image = np.asarray(image)
    pyr = pyramid_ref(image, levels, dtype) if pyramid is None else pyramid
    L = len(pyr) - 1
    v, on, l0, f, sub = _level_views(view, footprint, L, dtype)
    lo, hi = np.zeros((on.size, 4), dtype), np.zeros((on.size, 4), dtype)
    for l in range(L + 1):
        k = np.nonzero(on & (l0 == l))[0]
        if k.size:
            lo[k] = PR.gather_ref(pyr[l], sub(k, l), dtype)[:, 0]
        k = np.nonzero(on & (l0 + 1 == l) & (f != 0))[0]
        if k.size:
            hi[k] = PR.gather_ref(pyr[l], sub(k, l), dtype)[:, 0]
    out = np.zeros((on.size, 4), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where((f != 0)[:, None], (lo + ((hi - lo).astype(dtype) * f[:, None]).astype(dtype)).astype(dtype), lo)
        k = np.nonzero(on)[0]
        out[k] = (v[k, 0].astype(dtype)[:, None] * c[k]).astype(dtype)
    return out.reshape(np.asarray(view).shape[:-1] + (4,))


def scatter_mip_ref(d_color, view, res, footprint=1.0, levels=0, dtype=np.float64):
    """zdr_texel_gather_mip_backward into zero buffers, in ``dtype``, the additions of each tap in texel order:
    (d_image (height, width, 4), [None, d_level_1 .. d_level_L])"""
    dtype = np.dtype(dtype).type
    lay = layout(res, levels)
    L = len(lay) - 1
    v, on, l0, f, sub = _level_views(view, footprint, L, dtype)
    g = np.asarray(d_color).reshape(-1, 4).astype(dtype)
    vis = v[:, 0].astype(dtype)
    out = [np.zeros((h * w, 4), dtype) for w, h, _ in lay]
    one = dtype(1.0)
    for l, (w, h, _) in enumerate(lay):
        for k, share in ((np.nonzero(on & (l0 == l))[0], lambda k: (one - f[k]).astype(dtype)), (np.nonzero(on & (l0 + 1 == l) & (f != 0))[0], lambda k: f[k])):
            if not k.size:
                continue
            _, _, idx, tx, ty = PR.taps(sub(k, l), (w, h), dtype)
            ux, uy = one - tx, one - ty
            for i, wt in zip(idx, (ux * uy, tx * uy, ux * ty, tx * ty)):
                np.add.at(out[l], i, ((((wt.astype(dtype) * share(k)).astype(dtype) * vis[k]).astype(dtype))[:, None] * g[k]).astype(dtype))
    return out[0].reshape(int(res[1]), int(res[0]), 4), [None] + [o.reshape(h, w, 4) for o, (w, h, _) in zip(out[1:], lay[1:])]


def gather_mip_adjoint_ref(d_color, view, res, footprint=1.0, levels=0, dtype=np.float64):
    """the full image gradient into a zero image: the scatter followed by the pyramid adjoint, (height, width, 4) in ``dtype``"""
    dtype = np.dtype(dtype).type
    d_image, G = scatter_mip_ref(d_color, view, res, footprint, levels, dtype)
    return (d_image + pyramid_adjoint_ref(G, res, levels, dtype)).astype(dtype)


def linear_bar(r32, r64, floor_ulps=4, eps32=2.0 ** -24):
    """the rule of ``texel_project_cases.linear_bar`` on a float32 and a float64 reference result: 4 x the float32 reference's own error,
    floor ``floor_ulps`` float32 ulps of the float64 result's largest value"""
    with np.errstate(invalid="ignore"):
        err = float(np.nanmax(np.abs(np.asarray(r32, np.float64) - r64)))
    return max(4.0 * err, floor_ulps * eps32 * float(np.nanmax(np.abs(r64))))
