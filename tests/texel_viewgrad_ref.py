"""References of the camera gradients (include/zdr.h, "Camera gradients": zdr_texel_gather_dview, zdr_texel_view_backward).

``dview_ref``: the cotangent of the view buffer from a gather's colour cotangent, in NumPy for any float dtype, the header's operations
step by step; float64 is the truth the GPU tests compare with, float32 measures what float32 alone costs
(tests/texel_viewgrad_cases.py turns that into the bars).  The taps are ``texel_project_ref.taps``, the level split is
``texel_mip_ref.level_split``: the forward's own.

``camera_grad_ref``: the view formulas of tests/texel_project_ref.py written once more as torch on the CPU, differentiated by autograd.
``visible`` is not computed: it is held fixed, and float 0 of the cotangent is ignored.  The frame's VALUES are the float32 ones the
kernels project with (``texel_project_ref.camera_frame``: data that both dtypes share, like the points), its DERIVATIVE in the camera
is that of the exact formulas.  Helpers, not tests; tests/test_texel_viewgrad_ref_host.py pins them with checks of their own."""
import numpy as np
import torch

import texel_mip_ref as MR
import texel_project_ref as PR

LN2_32 = np.float32(0.693147180559945309)


def _sample_grad(level, X, Y, l, dtype):
    """the bilinear sample of ``level`` (h, w, 4) at (X 2^-l, Y 2^-l) and its derivative in X, Y: (c, gx, gy), each (N, 4) in ``dtype``"""
    h, w = level.shape[:2]
    sub = np.zeros((X.size, 8), np.float64)
    sub[:, 0] = 1.0
    sub[:, 2], sub[:, 3] = np.ldexp(X.astype(np.float64), -l), np.ldexp(Y.astype(np.float64), -l)
    _, _, (i00, i01, i10, i11), tx, ty = PR.taps(sub, (w, h), dtype)
    px = level.reshape(-1, 4)
    c00, c01, c10, c11 = (px[i].astype(dtype) for i in (i00, i01, i10, i11))
    tx, ty, inv = tx[:, None], ty[:, None], dtype(2.0 ** -l)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (c00 + ((c01 - c00).astype(dtype) * tx).astype(dtype)).astype(dtype)
        bot = (c10 + ((c11 - c10).astype(dtype) * tx).astype(dtype)).astype(dtype)
        c = (top + ((bot - top).astype(dtype) * ty).astype(dtype)).astype(dtype)
        a, b = (c01 - c00).astype(dtype), (c11 - c10).astype(dtype)
        gx = ((a + ((b - a).astype(dtype) * ty).astype(dtype)).astype(dtype) * inv).astype(dtype)
        gy = ((bot - top).astype(dtype) * inv).astype(dtype)
    return c, gx, gy


def _dot4(d, g, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        s = ((d[:, 0] * g[:, 0]).astype(dtype) + (d[:, 1] * g[:, 1]).astype(dtype)).astype(dtype)
        s = (s + (d[:, 2] * g[:, 2]).astype(dtype)).astype(dtype)
        return (s + (d[:, 3] * g[:, 3]).astype(dtype)).astype(dtype)


def _split(view, filter, footprint, L, dtype):
    """(on, s, l0, f) of every texel of a flattened view: the forward's level split; the bilinear filter samples level 0 alone"""
    v = np.asarray(view).reshape(-1, 8)
    on = (v[:, 0] != 0) & ~np.isnan(v[:, 0])
    if filter == "bilinear":
        return on, np.ones(on.size, dtype), np.zeros(on.size, np.int64), np.zeros(on.size, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v[:, 6].astype(dtype) * dtype(np.float32(footprint))).astype(dtype)
    l0, f = MR.level_split(v[:, 6], footprint, L, dtype)
    return on, s, l0, f


def dview_ref(image, view, d_color, filter="bilinear", footprint=1.0, levels=0, dtype=np.float64):
    """zdr_texel_gather_dview in ``dtype``: (H, W, 8), floats 2, 3 and (mip) 6"""
    dtype = np.dtype(dtype).type
    image = np.asarray(image)
    pyr = MR.pyramid_ref(image, levels, dtype) if filter == "mip" else [image.astype(dtype)]
    L = len(pyr) - 1
    v = np.asarray(view).reshape(-1, 8)
    on, s, l0, f = _split(view, filter, footprint, L, dtype)
    d = np.asarray(d_color).reshape(-1, 4).astype(dtype)
    n = on.size
    lo = [np.zeros((n, 4), dtype) for _ in range(3)]
    hi = [np.zeros((n, 4), dtype) for _ in range(3)]
    for l in range(L + 1):
        for dst, k in ((lo, np.nonzero(on & (l0 == l))[0]), (hi, np.nonzero(on & (l0 + 1 == l) & (f != 0))[0])):
            if k.size:
                for q, r in zip(dst, _sample_grad(pyr[l], v[k, 2], v[k, 3], l, dtype)):
                    q[k] = r
    out = np.zeros((n, 8), dtype)
    vis = np.where(on, v[:, 0], 0).astype(dtype)
    blend = (f != 0)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        gx = np.where(blend, (lo[1] + ((hi[1] - lo[1]).astype(dtype) * f[:, None]).astype(dtype)).astype(dtype), lo[1])
        gy = np.where(blend, (lo[2] + ((hi[2] - lo[2]).astype(dtype) * f[:, None]).astype(dtype)).astype(dtype), lo[2])
        out[:, 2] = np.where(on, (vis * _dot4(d, gx, dtype)).astype(dtype), 0)
        out[:, 3] = np.where(on, (vis * _dot4(d, gy, dtype)).astype(dtype), 0)
        moves = on & (f != 0) & (f < 1)
        k = (dtype(np.float32(footprint)) / (np.where(moves, s, 1).astype(dtype) * dtype(LN2_32)).astype(dtype)).astype(dtype)
        ds = (vis * (_dot4(d, (hi[0] - lo[0]).astype(dtype), dtype) * k).astype(dtype)).astype(dtype)
        out[:, 6] = np.where(moves, ds, 0)
    return out.reshape(np.asarray(view).shape[:-1] + (8,))


def dview_uncertain(view, res, filter="bilinear", footprint=1.0, levels=0):
    """(H, W) bool: visible texels whose float64 fx or fy in a sampled level lies within ``PR.JIGGLE`` of an integer, or whose s lies
    within 1e-4 relative of a power of two (mip) — there float32 may take another piece of the forward than float64"""
    v = np.asarray(view).reshape(-1, 8).astype(np.float64)
    L = len(MR.layout(res, levels)) - 1 if filter == "mip" else 0
    on, s, l0, f = _split(view, filter, footprint, L, np.float64)
    unc = np.zeros(on.size, bool)
    for up in (0, 1):
        l = l0 + up
        for c in (2, 3):
            fx = np.ldexp(np.where(on, v[:, c], 0.0), -l) - 0.5
            unc |= (np.abs(fx - np.rint(fx)) < PR.JIGGLE) & (on if up == 0 else on & (f != 0))
    if filter == "mip":
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.log2(np.where(on & (s > 0) & np.isfinite(s), s, 1.0))
        unc |= on & (s > 0.5) & (np.abs(e - np.rint(e)) < 1e-4 / np.log(2.0)) & (np.rint(e) <= L) & (np.rint(e) >= 0)
    return unc.reshape(np.asarray(view).shape[:-1])


# ------------------------------------------------------------------------------------------------------------------- the camera
def camera_vector(camera):
    fov, origin, target, up = PR.camera_tuple(camera)
    return np.asarray([fov, *origin, *target, *up], np.float32)


def _frame(cam, res, frame32):
    """o, fwd, right, upp, tan as functions of the camera tensor; with ``frame32`` their values are replaced by the float32 frame's"""
    o, tg, up = cam[1:4], cam[4:7], cam[7:10]
    d = tg - o
    fwd = d / torch.sqrt((d * d).sum())
    c = torch.linalg.cross(fwd, up)
    right = c / torch.sqrt((c * c).sum())
    upp = torch.linalg.cross(right, fwd)
    tan = torch.tan(0.5 * cam[0])
    out = [o, fwd, right, upp, tan]
    if frame32 is not None:
        vals = [frame32[0], frame32[1], frame32[2], frame32[3], frame32[4]]
        out = [x + (torch.as_tensor(np.asarray(v, np.float64), dtype=x.dtype) - x).detach() for x, v in zip(out, vals)]
    return out


def view_channels(points, cam, res, frame32=None):
    """floats 1 .. 6 of the view buffer for the shaded texels of ``points`` as torch functions of the camera tensor ``cam`` (10 values):
    ((N, 6) tensor, (ys, xs)).  ``frame32``: ``PR.camera_frame``'s tuple, whose values then replace the frame's"""
    points = np.asarray(points)
    ys, xs = np.nonzero(PR.shaded(points))
    dt = cam.dtype
    n = torch.as_tensor(points[ys, xs, 4:7].astype(np.float64), dtype=dt)
    p = torch.as_tensor(points[ys, xs, 8:11].astype(np.float64), dtype=dt)
    ts = torch.as_tensor(points[ys, xs, 7].astype(np.float64), dtype=dt)
    o, fwd, right, upp, tan = _frame(cam, res, frame32)
    half_w, half_h, aspect = 0.5 * res[0], 0.5 * res[1], float(np.float32(res[1]) / np.float32(res[0]))
    v = p - o
    z, dist = (v * fwd).sum(-1), torch.sqrt((v * v).sum(-1))
    wi = -v / dist[:, None]
    cosine = (n * wi).sum(-1)
    front = (z > 0).detach()
    zs = torch.where(front, z, torch.ones_like(z))
    zero = torch.zeros_like(z)
    X = torch.where(front, ((v * right).sum(-1) / zs / tan + 1.0) * half_w, zero)
    Y = torch.where(front, (-(v * upp).sum(-1) / zs / (tan * aspect) + 1.0) * half_h, zero)
    scale = torch.where(front, ts * half_w / (tan * zs), zero)
    return torch.stack([cosine, X, Y, z, dist, scale], -1), (ys, xs)


def camera_grad_ref(points, camera, res, d_view, dtype=torch.float64, terms=False, exact_frame=False):
    """zdr_texel_view_backward by autograd: d_camera (10,) float64 array of sum over shaded texels and floats 1 .. 6 of d_view x view.
    With ``terms`` also (10,) the sum over the texels of |that texel's contribution|: what the sums cancel from.  ``exact_frame``:
    the frame's values are not replaced by the float32 ones (what a finite difference of the formulas sees)"""
    frame32 = None if exact_frame else PR.camera_frame(camera, res)
    cam = torch.tensor(camera_vector(camera).astype(np.float64), dtype=dtype, requires_grad=True)
    ch, (ys, xs) = view_channels(points, cam, res, frame32)
    g = torch.as_tensor(np.asarray(d_view)[ys, xs, 1:7].astype(np.float64), dtype=dtype)
    if ys.size == 0:
        zeros = np.zeros(10)
        return (zeros, zeros) if terms else zeros
    (ch * g).sum().backward()
    grad = cam.grad.detach().double().numpy().copy()
    if not terms:
        return grad

    def per_texel(c):
        return (view_channels(points, c, res, frame32)[0] * g).sum(-1)
    J = torch.func.jacfwd(per_texel)(cam.detach())           # (N, 10)
    return grad, J.abs().sum(0).double().numpy()
