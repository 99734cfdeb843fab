"""Reference of the anisotropic gather (include/zdr.h: zdr_texel_footprint, zdr_texel_gather_aniso, zdr_texel_gather_aniso_backward) in
NumPy, for any float dtype: float64 is the truth the GPU tests compare with, float32 — the header's operation order step by step —
measures what float32 alone costs (tests/texel_aniso_cases.py turns that into the bars).

Built on tests/texel_project_ref.py (the camera frame, the shaded rule, the bilinear taps) and tests/texel_mip_ref.py (the pyramid, the
level split, the per-level sample), neither of which is modified.  A probe is the mip gather's trilinear sample at a shifted position;
the probes of a texel are added in order.  The scatter adds in (texel, probe, lower taps, upper taps) order.  ``truth_ref`` is the
quality yardstick: the mean of the image over the texel's own square patch, supersampled and projected point by point.
A helper, not a test; tests/test_texel_aniso_ref_host.py pins it."""
import numpy as np

import texel_mip_ref as MR
import texel_project_ref as PR

F32 = np.float32
NEAR = 1e-4                     # how close to a switch of N or of a clamp a texel is exempt


def _normalize(a, dtype):
    return (a / np.sqrt(PR._dot(a, a))[..., None]).astype(dtype)


def make_onb(n, dtype):
    """(tangent, binormal) of the kernels' make_onb (csrc/scene.h) for normals (N, 3)"""
    zero = np.zeros_like(n[:, 0])
    b = np.where((np.abs(n[:, 0]) > np.abs(n[:, 2]))[:, None], np.stack([-n[:, 1], n[:, 0], zero], -1), np.stack([zero, -n[:, 2], n[:, 1]], -1)).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        b = _normalize(b, dtype)
        t = _normalize(PR._cross(b, n).astype(dtype), dtype)
    return t, b


def jacobian(p, frame, res, dtype):
    """positions (N, 3) -> z, gX, gY (N, 3): the derivatives of the view buffer's X, Y with respect to the world position"""
    o, fwd, right, upp, tan, aspect = (np.asarray(a).astype(dtype) for a in frame)
    half_w, half_h = dtype(0.5) * dtype(res[0]), dtype(0.5) * dtype(res[1])
    v = (p - o).astype(dtype)
    z, a, b = PR._dot(v, fwd), PR._dot(v, right), PR._dot(v, upp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        zz = (z * z).astype(dtype)
        gX = ((right * z[:, None] - fwd * a[:, None]).astype(dtype) * (half_w / (tan * zz))[:, None]).astype(dtype)
        gY = (-((upp * z[:, None] - fwd * b[:, None]).astype(dtype) * (half_h / ((tan * aspect) * zz))[:, None])).astype(dtype)
    return z, gX, gY


def ellipse(m00, m01, m10, m11, dtype):
    """(N, 4): major e (2 floats), minor, major of the 2 x 2 matrices M, in the header's operation order"""
    half = dtype(0.5)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P, Q, R = (m00 * m00 + m01 * m01).astype(dtype), (m10 * m10 + m11 * m11).astype(dtype), (m00 * m10 + m01 * m11).astype(dtype)
        hd = (half * (P - Q)).astype(dtype)
        d = np.sqrt(hd * hd + R * R).astype(dtype)
        major = np.sqrt(half * (P + Q) + d).astype(dtype)
        minor = np.where(major == 0, dtype(0.0), np.abs(m00 * m11 - m01 * m10) / major).astype(dtype)
        first = P >= Q
        ex, ey = np.where(first, hd + d, R).astype(dtype), np.where(first, R, half * (Q - P) + d).astype(dtype)
        el = np.sqrt(ex * ex + ey * ey).astype(dtype)
        ex, ey = np.where(el == 0, dtype(1.0), ex / el).astype(dtype), np.where(el == 0, dtype(0.0), ey / el).astype(dtype)
        out = np.stack([major * ex, major * ey, minor, major], -1).astype(dtype)
    return out


def footprint_ref(points, camera, res, dtype=np.float64, rotate=0.0):
    """zdr_texel_footprint in ``dtype`` for the sample points ``points`` (H, W, 16): (H, W, 4).  ``rotate``: turn (t1, t2) by that angle
    in the tangent plane first — the ellipse must not depend on it"""
    dtype = np.dtype(dtype).type
    points = np.asarray(points)
    H, W = points.shape[:2]
    out = np.zeros((H, W, 4), dtype)
    ys, xs = np.nonzero(PR.shaded(points))
    if ys.size == 0:
        return out
    n, p, ts = points[ys, xs, 4:7].astype(dtype), points[ys, xs, 8:11].astype(dtype), points[ys, xs, 7].astype(dtype)
    z, gX, gY = jacobian(p, PR.camera_frame(camera, res), res, dtype)
    t1, t2 = make_onb(n, dtype)
    if rotate:
        c, s = dtype(np.cos(rotate)), dtype(np.sin(rotate))
        t1, t2 = (c * t1 + s * t2).astype(dtype), (c * t2 - s * t1).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        m = [(ts * PR._dot(g, t)).astype(dtype) for g in (gX, gY) for t in (t1, t2)]
    e = ellipse(*m, dtype)
    keep = (z > 0) & np.isfinite(e).all(-1)
    out[ys[keep], xs[keep]] = e[keep]
    return out


def probes(fp, footprint, max_aniso, dtype=np.float64):
    """(N int64, s ``dtype``) of footprint rows (..., 4), flattened: the header's "Probes of a texel" """
    dtype = np.dtype(dtype).type
    f = np.asarray(fp).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        A, B = (f[:, 3].astype(dtype) * dtype(F32(footprint))).astype(dtype), (f[:, 2].astype(dtype) * dtype(F32(footprint))).astype(dtype)
        wide = A > 1
        Bp = np.fmax(np.fmax(B, (A / dtype(max_aniso)).astype(dtype)), dtype(1.0)).astype(dtype)
        q = np.ceil((A / Bp).astype(dtype) - dtype(0.125))
        N = np.where(q >= 1, np.where(q <= max_aniso, q, max_aniso), 1)
    N = np.where(wide, np.nan_to_num(N, nan=1.0), 1).astype(np.int64)
    return N, np.where(wide, Bp, dtype(1.0)).astype(dtype)


def exempt(fp, footprint=1.0, max_aniso=8):
    """(...) bool, in float64: texels within NEAR of a switch — A / B' - 0.125 of an integer, or one of the clamps (A against 1, B against
    1, B against A / max_aniso) relatively"""
    f = np.asarray(fp, np.float64)
    shape = f.shape[:-1]
    f = f.reshape(-1, 4)
    A, B = f[:, 3] * float(F32(footprint)), f[:, 2] * float(F32(footprint))
    with np.errstate(invalid="ignore", divide="ignore"):
        Bp = np.fmax(np.fmax(B, A / max_aniso), 1.0)
        q = A / Bp - 0.125
        near = np.abs(A - 1.0) <= NEAR
        wide = A > 1
        near |= wide & (np.abs(q - np.rint(q)) <= NEAR)
        near |= wide & (np.abs(B - 1.0) <= NEAR)
        near |= wide & (np.abs(B - A / max_aniso) <= NEAR * np.maximum(np.abs(B), A / max_aniso))
    return near.reshape(shape)


def _setup(view, fp, footprint, max_aniso, L, dtype):
    v, f = np.asarray(view).reshape(-1, 8), np.asarray(fp).reshape(-1, 4)
    on = (v[:, 0] != 0) & ~np.isnan(v[:, 0])
    N, s = probes(f, footprint, max_aniso, dtype)
    l0, fr = MR.level_split(s, 1.0, L, dtype)
    return v, f, on, N, l0, fr


def _probe_xy(v, f, k, i, N, footprint, dtype):
    """X_i, Y_i in ``dtype`` of the texels k"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(2 * i + 1 - N[k]).astype(dtype) / (dtype(2.0) * N[k].astype(dtype))).astype(dtype)
        tf = (t * dtype(F32(footprint))).astype(dtype)
        X = (v[k, 2].astype(dtype) + (tf * f[k, 0].astype(dtype)).astype(dtype)).astype(dtype)
        Y = (v[k, 3].astype(dtype) + (tf * f[k, 1].astype(dtype)).astype(dtype)).astype(dtype)
    return X, Y


def _sub(X, Y, l):
    s = np.zeros((X.size, 1, 8), np.float64)
    s[:, 0, 0] = 1.0
    s[:, 0, 2] = np.ldexp(X.astype(np.float64), -l); s[:, 0, 3] = np.ldexp(Y.astype(np.float64), -l)
    return s


def gather_aniso_ref(image, view, fp, footprint=1.0, max_aniso=8, levels=0, dtype=np.float64, pyramid=None):
    """zdr_texel_gather_aniso in ``dtype``: (H, W, 4)"""
    dtype = np.dtype(dtype).type
    pyr = MR.pyramid_ref(np.asarray(image), levels, dtype) if pyramid is None else pyramid
    L = len(pyr) - 1
    v, f, on, N, l0, fr = _setup(view, fp, footprint, max_aniso, L, dtype)
    acc = np.zeros((on.size, 4), dtype)
    for i in range(int(N[on].max()) if on.any() else 0):
        k = np.nonzero(on & (N > i))[0]
        X, Y = _probe_xy(v, f, k, i, N, footprint, dtype)
        lo, hi = np.zeros((k.size, 4), dtype), np.zeros((k.size, 4), dtype)
        for l in range(L + 1):
            j = np.nonzero(l0[k] == l)[0]
            if j.size:
                lo[j] = PR.gather_ref(pyr[l], _sub(X[j], Y[j], l), dtype)[:, 0]
            j = np.nonzero((l0[k] + 1 == l) & (fr[k] != 0))[0]
            if j.size:
                hi[j] = PR.gather_ref(pyr[l], _sub(X[j], Y[j], l), dtype)[:, 0]
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.where((fr[k] != 0)[:, None], (lo + ((hi - lo).astype(dtype) * fr[k, None]).astype(dtype)).astype(dtype), lo)
            acc[k] = c if i == 0 else (acc[k] + c).astype(dtype)
    out = np.zeros((on.size, 4), dtype)
    k = np.nonzero(on)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        inv_n = (dtype(1.0) / N[k].astype(dtype)).astype(dtype)
        out[k] = (v[k, 0].astype(dtype)[:, None] * (acc[k] * inv_n[:, None]).astype(dtype)).astype(dtype)
    return out.reshape(np.asarray(view).shape[:-1] + (4,))


def scatter_aniso_ref(d_color, view, fp, res, footprint=1.0, max_aniso=8, levels=0, dtype=np.float64):
    """zdr_texel_gather_aniso_backward into zero buffers, in ``dtype``, the additions in (texel, probe, lower taps, upper taps) order:
    (d_image (height, width, 4), [None, d_level_1 .. d_level_L])"""
    dtype = np.dtype(dtype).type
    lay = MR.layout(res, levels)
    L = len(lay) - 1
    v, f, on, N, l0, fr = _setup(view, fp, footprint, max_aniso, L, dtype)
    g = np.asarray(d_color).reshape(-1, 4).astype(dtype)
    vis = v[:, 0].astype(dtype)
    one = dtype(1.0)
    adds = [[] for _ in lay]                                         # per level: (order key, pixel index, value (n, 4))
    for i in range(int(N[on].max()) if on.any() else 0):
        k = np.nonzero(on & (N > i))[0]
        X, Y = _probe_xy(v, f, k, i, N, footprint, dtype)
        inv_n = (one / N[k].astype(dtype)).astype(dtype)
        for l, (w, h, _) in enumerate(lay):
            for upper, j, share in ((0, np.nonzero(l0[k] == l)[0], lambda j: (one - fr[k[j]]).astype(dtype)),
                                    (1, np.nonzero((l0[k] + 1 == l) & (fr[k] != 0))[0], lambda j: fr[k[j]])):
                if not j.size:
                    continue
                _, _, idx, tx, ty = PR.taps(_sub(X[j], Y[j], l), (w, h), dtype)
                ux, uy = one - tx, one - ty
                for tap, (ix, wt) in enumerate(zip(idx, (ux * uy, tx * uy, ux * ty, tx * ty))):
                    val = (((((wt.astype(dtype) * share(j)).astype(dtype) * inv_n[j]).astype(dtype) * vis[k[j]]).astype(dtype))[:, None] * g[k[j]]).astype(dtype)
                    adds[l].append((((k[j] * 32 + i) * 2 + upper) * 4 + tap, ix, val))
    out = []
    for (w, h, _), a in zip(lay, adds):
        o = np.zeros((h * w, 4), dtype)
        if a:
            key, ix, val = np.concatenate([x[0] for x in a]), np.concatenate([x[1] for x in a]), np.concatenate([x[2] for x in a])
            order = np.argsort(key, kind="stable")
            np.add.at(o, ix[order], val[order])
        out.append(o.reshape(h, w, 4))
    return out[0], [None] + out[1:]


def gather_aniso_adjoint_ref(d_color, view, fp, res, footprint=1.0, max_aniso=8, levels=0, dtype=np.float64):
    """the full image gradient into a zero image: the scatter followed by the pyramid adjoint, (height, width, 4) in ``dtype``"""
    dtype = np.dtype(dtype).type
    d_image, G = scatter_aniso_ref(d_color, view, fp, res, footprint, max_aniso, levels, dtype)
    return (d_image + MR.pyramid_adjoint_ref(G, res, levels, dtype)).astype(dtype)


def truth_ref(image, points, camera, res, sub=8):
    """The quality yardstick, float64: per texel the mean of the image — nearest pixel, the image continued by its border — over the
    texel's own patch, a square of side texel_size in its tangent plane, ``sub`` x ``sub`` points projected one by one: (H, W, 4), zeros
    where the texel is not shaded"""
    points, image = np.asarray(points), np.asarray(image, np.float64)
    H, W = points.shape[:2]
    h, w = image.shape[:2]
    out = np.zeros((H, W, 4))
    ys, xs = np.nonzero(PR.shaded(points))
    n, p, ts = points[ys, xs, 4:7].astype(np.float64), points[ys, xs, 8:11].astype(np.float64), points[ys, xs, 7].astype(np.float64)
    t1, t2 = make_onb(n, np.float64)
    frame = PR.camera_frame(camera, res)
    offs = (np.arange(sub) + 0.5) / sub - 0.5
    acc = np.zeros((ys.size, 4))
    for u in offs:
        for v in offs:
            q = p + (u * ts)[:, None] * t1 + (v * ts)[:, None] * t2
            _, _, _, X, Y = PR.project(q, frame, res, np.float64)
            xi, yi = np.clip(np.floor(np.nan_to_num(X)), 0, w - 1).astype(np.int64), np.clip(np.floor(np.nan_to_num(Y)), 0, h - 1).astype(np.int64)
            acc += image[yi, xi]
    out[ys, xs] = acc / (sub * sub)
    return out
