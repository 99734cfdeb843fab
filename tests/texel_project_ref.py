"""Reference of the texture-space views (include/zdr.h: zdr_scene_texel_view, zdr_texel_gather, zdr_texel_gather_backward) in NumPy, for
any float dtype: float64 is the truth the GPU tests compare with, float32 — the header's operation order step by step — measures what
float32 alone costs (tests/texel_project_cases.py turns that into the bars).

What it is given: the sample points — an (H, W, 16) buffer in the layout of zdr_scene_texel_aovs, from tests/texel_ref.py — a camera as
(fov, origin, target, up), the image size, and visibility from ``OracleScene.trace_any``.  The camera's frame is formed in float32 the
way the host forms it (csrc/zdr_api.cpp, camera_frame) and is data both dtypes share, like the points; everything computed from them
is computed in ``dtype``.

Besides the buffer ``view_ref`` returns the UNCERTAIN texels: those whose answer for the ray to o differs from the answer for any of
the four rays to o +- 1e-4 dist right, o +- 1e-4 dist upp; those whose X or Y lies within 1e-3 pixel of the frustum's border; those with
|z| < 1e-4.  A helper, not a test; tests/test_texel_project_ref_host.py pins it."""
import numpy as np

import texel_lighting_ref as LR

F32 = np.float32
BORDER_TOL = 1e-3
Z_TOL = 1e-4
JIGGLE = 1e-4


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def camera_tuple(camera):
    if isinstance(camera, (tuple, list)):
        return camera
    return (camera.fov, tuple(camera.origin), tuple(camera.target), tuple(camera.up))


def camera_frame(camera, res):
    """(o, fwd, right, upp, tan, aspect) in float32, operation by operation as the host's camera_frame and make_render_cfg"""
    fov, origin, target, up = camera_tuple(camera)
    o, tg, up = np.asarray(origin, F32), np.asarray(target, F32), np.asarray(up, F32)

    def normalize(a):
        return (a * (F32(1.0) / np.sqrt(_dot(a, a)))).astype(F32)
    fwd = normalize(tg - o)
    right = normalize(_cross(fwd, up).astype(F32))
    upp = _cross(right, fwd).astype(F32)
    tan = F32(np.tan(np.float64(F32(0.5) * F32(fov))))
    aspect = F32(res[1]) / F32(res[0])
    return o, fwd, right, upp, tan, aspect


def shaded(points):
    points = np.asarray(points)
    return (points[..., 12] == 1) & ~np.isnan(points[..., 4:7]).any(-1) & ~np.isnan(points[..., 8:11]).any(-1)


def project(p, frame, res, dtype):
    """positions (N, 3) -> z, dist, wi (N, 3), X, Y in ``dtype`` (X, Y 0 where z <= 0), in the header's operation order"""
    o, fwd, right, upp, tan, aspect = (np.asarray(a).astype(dtype) for a in frame)
    half_w, half_h = dtype(0.5) * dtype(res[0]), dtype(0.5) * dtype(res[1])
    v, w = (p - o).astype(dtype), (o - p).astype(dtype)
    z, dist = _dot(v, fwd), np.sqrt(_dot(v, v))
    with np.errstate(divide="ignore", invalid="ignore"):
        wi = (w / dist[:, None]).astype(dtype)
        X = ((_dot(v, right) / z / tan + dtype(1.0)) * half_w).astype(dtype)
        Y = ((-_dot(v, upp) / z / (tan * aspect) + dtype(1.0)) * half_h).astype(dtype)
    front = z > 0
    return z, dist, wi, np.where(front, X, dtype(0.0)), np.where(front, Y, dtype(0.0))


def _segments_free(oscene, p, target):
    """the any-hit answer for the segments p -> target, interval (1e-4, |target - p|); float64 in, the rays are float32 as the oracle takes them"""
    w = target - p
    d = np.sqrt(_dot(w, w))
    return ~LR.trace_any(oscene, p, w / d[:, None], 1e-4, d)


def view_ref(points, camera, res, oscene, dtype=np.float64):
    """The view buffer for the sample points ``points`` (H, W, 16).  Returns a dict: ``data`` (H, W, 8) in ``dtype``; ``uncertain``,
    ``front``, ``inside`` (H, W) bool"""
    dtype = np.dtype(dtype).type
    points = np.asarray(points)
    H, W = points.shape[:2]
    frame = camera_frame(camera, res)
    ys, xs = np.nonzero(shaded(points))
    out = {"data": np.zeros((H, W, 8), dtype), "uncertain": np.zeros((H, W), bool), "front": np.zeros((H, W), bool), "inside": np.zeros((H, W), bool)}
    if ys.size == 0:
        return out
    n, p, ts = points[ys, xs, 4:7].astype(dtype), points[ys, xs, 8:11].astype(dtype), points[ys, xs, 7].astype(dtype)
    z, dist, wi, X, Y = project(p, frame, res, dtype)
    front = z > 0
    inside = front & (X >= 0) & (X < dtype(res[0])) & (Y >= 0) & (Y < dtype(res[1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(front, ts * (dtype(0.5) * dtype(res[0])) / (frame[4].astype(dtype) * z), dtype(0.0)).astype(dtype)
    o64, right64, upp64 = frame[0].astype(np.float64), frame[2].astype(np.float64), frame[3].astype(np.float64)
    idx = np.nonzero(inside)[0]
    visible = np.zeros(ys.size, bool)
    unc = np.abs(z) < Z_TOL
    if idx.size:
        free = LR.trace_any(oscene, p[idx], wi[idx], 1e-4, dist[idx]) == 0
        visible[idx] = free
        p64, d64 = p[idx].astype(np.float64), dist[idx].astype(np.float64)
        for axis in (right64, upp64):
            for sign in (1.0, -1.0):
                other = _segments_free(oscene, p64, o64[None, :] + sign * JIGGLE * d64[:, None] * axis[None, :])
                unc[idx] |= other != free
    for c, size in ((X, res[0]), (Y, res[1])):
        unc |= front & ((np.abs(c) < BORDER_TOL) | (np.abs(c - size) < BORDER_TOL))
    data = np.stack([visible.astype(dtype), _dot(n, wi), X, Y, z, dist, scale, np.zeros_like(z)], -1).astype(dtype)
    out["data"][ys, xs] = data
    out["uncertain"][ys, xs] = unc
    out["front"][ys, xs] = front
    out["inside"][ys, xs] = inside
    return out


def taps(view, res, dtype):
    """(visible (N,), [(index (N,), weight (N,)) x 4], (i00, i01, i10, i11, tx, ty)) of a view buffer (..., 8), flattened"""
    dtype = np.dtype(dtype).type
    w, h = int(res[0]), int(res[1])
    v = np.asarray(view).reshape(-1, 8)
    vis = v[:, 0].astype(dtype)
    on = (v[:, 0] != 0) & ~np.isnan(v[:, 0])
    X, Y = np.where(on, v[:, 2], 0.5).astype(dtype), np.where(on, v[:, 3], 0.5).astype(dtype)
    fx, fy = X - dtype(0.5), Y - dtype(0.5)
    x0f, y0f = np.floor(fx), np.floor(fy)
    tx, ty = (fx - x0f).astype(dtype), (fy - y0f).astype(dtype)
    x0, y0 = np.clip(x0f, -1, w).astype(np.int64), np.clip(y0f, -1, h).astype(np.int64)
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    return on, vis, (ya * w + xa, ya * w + xb, yb * w + xa, yb * w + xb), tx, ty


def gather_ref(image, view, dtype=np.float64):
    """zdr_texel_gather in ``dtype``, in the header's operation order: (H, W, 4)"""
    dtype = np.dtype(dtype).type
    image = np.asarray(image)
    h, w = image.shape[:2]
    on, vis, (i00, i01, i10, i11), tx, ty = taps(view, (w, h), dtype)
    px = image.reshape(-1, 4)
    out = np.zeros((on.size, 4), dtype)
    k = np.nonzero(on)[0]
    c00, c01, c10, c11 = (px[i[k]].astype(dtype) for i in (i00, i01, i10, i11))
    with np.errstate(invalid="ignore", over="ignore"):
        top = (c00 + (c01 - c00) * tx[k, None]).astype(dtype)
        bot = (c10 + (c11 - c10) * tx[k, None]).astype(dtype)
        out[k] = (vis[k, None] * (top + (bot - top) * ty[k, None])).astype(dtype)
    return out.reshape(np.asarray(view).shape[:-1] + (4,))


def gather_adjoint_ref(d_color, view, res, dtype=np.float64):
    """zdr_texel_gather_backward into a zero image, in ``dtype``: (height, width, 4), the additions in texel order"""
    dtype = np.dtype(dtype).type
    w, h = int(res[0]), int(res[1])
    on, vis, idx, tx, ty = taps(view, res, dtype)
    g = np.asarray(d_color).reshape(-1, 4).astype(dtype)
    ux, uy = dtype(1.0) - tx, dtype(1.0) - ty
    out = np.zeros((h * w, 4), dtype)
    k = np.nonzero(on)[0]
    for i, wt in zip(idx, (ux * uy, tx * uy, ux * ty, tx * ty)):
        np.add.at(out, i[k], ((wt[k] * vis[k]).astype(dtype)[:, None] * g[k]).astype(dtype))
    return out.reshape(h, w, 4)
