"""Reference of the UV tangents (include/zdr.h: zdr_scene_texel_tangents, zdr_texel_footprint_tangents) in NumPy, for any float dtype:
float64 is the truth the GPU tests compare with, float32 — the header's operation order step by step — measures what float32 alone
costs (tests/texel_tangent_cases.py turns that into the bars).

Built on tests/texel_ref.py (the winners, the world corners in input order, the pixel-space corners and the degenerate test) and
tests/texel_aniso_ref.py (the camera Jacobian and the closed-form ellipse), neither of which is modified.  ``truth_uv_ref`` is the
quality yardstick: the mean of the image over the texel's TRUE patch, the parallelogram its tangents span, supersampled and projected
point by point.  A helper, not a test; tests/test_texel_tangent_ref_host.py pins it."""
import numpy as np

import texel_aniso_ref as AR
import texel_project_ref as PR
import texel_ref as R


def triangle_tangents(P, q, dtype):
    """(Tx, Ty) of one triangle: world corners P (3, 3) in input order, pixel-space corners q (3, 2), in the header's operation order"""
    e1, e2 = (P[1] - P[0]).astype(dtype), (P[2] - P[0]).astype(dtype)
    a1, a2, b1, b2 = q[1][0] - q[0][0], q[2][0] - q[0][0], q[1][1] - q[0][1], q[2][1] - q[0][1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        det = dtype(dtype(a1 * b2) - dtype(a2 * b1))
        tx = ((e1 * b2).astype(dtype) - (e2 * b1).astype(dtype)).astype(dtype) / det
        ty = ((e2 * a1).astype(dtype) - (e1 * a2).astype(dtype)).astype(dtype) / det
    return tx.astype(dtype), ty.astype(dtype)


def tangents_ref(arrays, slots, material, tex_hw, dtype=np.float64, aovs=None):
    """zdr_scene_texel_tangents in ``dtype`` on the winners of ``texel_ref.texel_aovs_ref`` (``aovs``: that call's result for the same
    arguments, computed here when not given).  Returns a dict: ``data`` (H, W, 8) in ``dtype`` and ``aovs``, the dict of texel_aovs_ref."""
    dtype = np.dtype(dtype).type
    H, W = int(tex_hw[0]), int(tex_hw[1])
    if aovs is None:
        aovs = R.texel_aovs_ref(arrays, slots, material, tex_hw, dtype)
    P = R.world_triangles(arrays, dtype)[0]
    Q = R.pixel_space(R.world_triangles(arrays, dtype)[2], H, W, dtype)
    winner = np.where(aovs["cov_g"] != R.EMPTY, aovs["cov_g"], aovs["reach_g"])
    data = np.zeros((H, W, 8), dtype)
    for g in np.unique(winner[winner != R.EMPTY]):
        if R.Setup(Q[g], dtype).degenerate:                     # zdr_scene_texel_aovs's own rule: texel_size is 0 there
            continue
        tx, ty = triangle_tangents(P[g], Q[g], dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.array([tx[1] * ty[2] - tx[2] * ty[1], tx[2] * ty[0] - tx[0] * ty[2], tx[0] * ty[1] - tx[1] * ty[0]], dtype)
            area = np.sqrt(dtype(dtype(c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]))
        row = np.concatenate([tx, [area], ty, [0]]).astype(dtype)
        if not np.isfinite(row).all():
            continue
        ys, xs = np.nonzero(winner == g)
        n = aovs["data"][ys, xs, 4:7].astype(dtype)
        with np.errstate(invalid="ignore"):
            s = ((c[0] * n[:, 0] + c[1] * n[:, 1]).astype(dtype) + c[2] * n[:, 2]).astype(dtype)
        data[ys, xs] = row[None]
        data[ys, xs, 7] = np.where(s > 0, 1.0, np.where(s < 0, -1.0, 0.0))
    return {"data": data, "aovs": aovs}


def zero_rows(tangents):
    return (np.asarray(tangents) == 0).all(-1)


def footprint_tangents_ref(points, tangents, camera, res, dtype=np.float64):
    """zdr_texel_footprint_tangents in ``dtype`` for the sample points ``points`` (H, W, 16) and their tangent rows (H, W, 8): (H, W, 4)"""
    dtype = np.dtype(dtype).type
    points, tangents = np.asarray(points), np.asarray(tangents)
    H, W = points.shape[:2]
    out = np.zeros((H, W, 4), dtype)
    ys, xs = np.nonzero(PR.shaded(points) & ~zero_rows(tangents))
    if ys.size == 0:
        return out
    p = points[ys, xs, 8:11].astype(dtype)
    tx, ty = tangents[ys, xs, 0:3].astype(dtype), tangents[ys, xs, 4:7].astype(dtype)
    z, gX, gY = AR.jacobian(p, PR.camera_frame(camera, res), res, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        m = [PR._dot(g, t).astype(dtype) for g in (gX, gY) for t in (tx, ty)]
    e = AR.ellipse(*m, dtype)
    keep = (z > 0) & np.isfinite(e).all(-1)
    out[ys[keep], xs[keep]] = e[keep]
    return out


def truth_uv_ref(image, points, tangents, camera, res, sub=8):
    """The quality yardstick, float64: per texel the mean of the image — nearest pixel, the image continued by its border — over the
    texel's true patch, the parallelogram p + a Tx + b Ty with a, b in [-1/2, 1/2], ``sub`` x ``sub`` points projected one by one:
    (H, W, 4), zeros where the texel is not shaded"""
    points, tangents, image = np.asarray(points), np.asarray(tangents, np.float64), np.asarray(image, np.float64)
    H, W = points.shape[:2]
    h, w = image.shape[:2]
    out = np.zeros((H, W, 4))
    ys, xs = np.nonzero(PR.shaded(points))
    p = points[ys, xs, 8:11].astype(np.float64)
    tx, ty = tangents[ys, xs, 0:3], tangents[ys, xs, 4:7]
    frame = PR.camera_frame(camera, res)
    offs = (np.arange(sub) + 0.5) / sub - 0.5
    acc = np.zeros((ys.size, 4))
    for a in offs:
        for b in offs:
            q = p + a * tx + b * ty
            _, _, _, X, Y = PR.project(q, frame, res, np.float64)
            xi, yi = np.clip(np.floor(np.nan_to_num(X)), 0, w - 1).astype(np.int64), np.clip(np.floor(np.nan_to_num(Y)), 0, h - 1).astype(np.int64)
            acc += image[yi, xi]
    out[ys, xs] = acc / (sub * sub)
    return out
