"""The references of the camera gradients (tests/texel_viewgrad_ref.py) proven with checks of their own, without a GPU: against central
differences of the forward references, against closed forms, and against the recorded margins (tests/texel_viewgrad_cases.py)."""
import numpy as np
import pytest
import torch

import texel_mip_ref as MR
import texel_project_cases as PC
import texel_project_ref as PR
import texel_viewgrad_cases as VC
import texel_viewgrad_ref as VR
from zdr_amd import Camera


def _forward(img, view, filter, footprint):
    return PR.gather_ref(img, view) if filter == "bilinear" else MR.gather_mip_ref(img, view, footprint)


@pytest.mark.parametrize("name", VC.CASES)
def test_dview_ref_is_the_central_difference_of_the_forward_references(name):
    view = VC.view32(name).astype(np.float64)
    g = VC.d_color(name).astype(np.float64)
    seen = 0
    for filter, footprint in VC.FILTERS:
        certain = ~VC.uncertain(name, view, filter, footprint) & (view[..., 0] != 0)
        for kind in VC.IMAGES:
            img = VC.image(kind, VC.res_of(name)).astype(np.float64)
            ref = VR.dview_ref(img, view, g, filter, footprint)
            for ch, h in ((2, 1e-5), (3, 1e-5), (6, 1e-6)):
                step = h * (np.abs(view[..., 6]) if ch == 6 else 1.0)
                up, dn = view.copy(), view.copy()
                up[..., ch] += step; dn[..., ch] -= step
                diff = (_forward(img, up, filter, footprint) - _forward(img, dn, filter, footprint)) / np.where(step == 0, 1.0, 2.0 * step)[..., None]
                fd = (g * diff).sum(-1)
                if ch == 6 and filter == "bilinear":
                    assert not ref[..., 6].any()
                    continue
                tol = 1e-6 * max(1.0, float(np.abs(ref[..., ch][certain]).max(initial=0.0)))
                assert np.abs(fd - ref[..., ch])[certain].max(initial=0.0) <= tol, (filter, footprint, kind, ch)
                seen += int(certain.sum())
    assert seen > 0


@pytest.mark.parametrize("name", VC.CASES)
def test_bilinear_dview_of_a_ramp_is_its_slope(name):
    res = VC.res_of(name)
    view = VC.view32(name).astype(np.float64)
    g = VC.d_color(name).astype(np.float64)
    ref = VR.dview_ref(VC.image("ramp", res).astype(np.float64), view, g, "bilinear")
    X, Y = view[..., 2], view[..., 3]
    inner = (view[..., 0] != 0) & (X > 1.0) & (X < res[0] - 1.0) & (Y > 1.0) & (Y < res[1] - 1.0)      # all four taps distinct
    weight = (g * np.arange(1, 5)).sum(-1) * view[..., 0]
    assert np.allclose(ref[..., 2][inner], (weight * VC.RAMP[0])[inner], rtol=0, atol=1e-12)
    assert np.allclose(ref[..., 3][inner], (weight * VC.RAMP[1])[inner], rtol=0, atol=1e-12)
    if res == (1, 1):
        assert not ref.any()                                   # every tap is the one pixel


@pytest.mark.parametrize("name", VC.CASES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_mip_reference_equals_the_bilinear_one_where_the_footprint_is_small(name, dtype):
    view = VC.view32(name).copy()
    view[..., 6] = np.minimum(view[..., 6], 0.25)               # scale * footprint <= 1
    img, g = VC.image("noise", VC.res_of(name)), VC.d_color(name)
    a = VR.dview_ref(img, view, g, "bilinear", dtype=dtype)
    b = VR.dview_ref(img, view, g, "mip", 4.0, dtype=dtype)
    assert a.tobytes() == b.tobytes()


def _frame64(cam, res):
    o, tg, up = cam[1:4], cam[4:7], cam[7:10]
    fwd = (tg - o) / np.linalg.norm(tg - o)
    right = np.cross(fwd, up); right /= np.linalg.norm(right)
    return o, fwd, right, np.cross(right, fwd), np.tan(0.5 * cam[0]), np.float64(np.float32(res[1]) / np.float32(res[0]))


def _channels64(points, cam, res):
    """floats 1 .. 6 of the view buffer of the shaded texels from ``PR.project`` in float64 with the exact frame of ``cam``"""
    ys, xs = np.nonzero(PR.shaded(points))
    n, p, ts = (points[ys, xs, a:b].astype(np.float64) for a, b in ((4, 7), (8, 11), (7, 8)))
    frame = _frame64(cam, res)
    z, dist, wi, X, Y = PR.project(p, frame, res, np.float64)
    scale = np.where(z > 0, ts[:, 0] * (0.5 * res[0]) / (frame[4] * np.where(z > 0, z, 1.0)), 0.0)
    return np.stack([PR._dot(n, wi), X, Y, z, dist, scale], -1), (ys, xs)


@pytest.mark.parametrize("name", VC.CASES)
def test_the_camera_gradient_is_the_central_difference_of_the_view_reference(name):
    pts = PC.points(name).copy()
    res, camera = VC.res_of(name), VC.camera_of(name)
    cam = VR.camera_vector(camera).astype(np.float64)
    ch, (ys, xs) = _channels64(pts, cam, res)
    near = np.abs(ch[:, 3]) < 0.05                              # a texel near the camera's plane changes sides under the step
    pts[ys[near], xs[near], 12] = 0.0
    g = VC.d_view(pts.shape)
    grad, terms = VR.camera_grad_ref(pts, camera, res, g, terms=True, exact_frame=True)
    ch, (ys, xs) = _channels64(pts, cam, res)
    assert np.allclose(ch, VR.view_channels(pts, torch.tensor(cam), res)[0].numpy(), rtol=1e-12, atol=1e-12)
    gg = g[ys, xs, 1:7].astype(np.float64)
    h = 1e-6
    noise = 8 * 2.0 ** -52 * float(np.abs(ch * gg).sum()) / h    # what the difference of two float64 sums of this size is good for
    for k in range(10):
        up, dn = cam.copy(), cam.copy()
        up[k] += h; dn[k] -= h
        fd = ((_channels64(pts, up, res)[0] - _channels64(pts, dn, res)[0]) * gg).sum() / (2 * h)
        assert abs(fd - grad[k]) <= 1e-6 * terms[k] + noise, (k, fd, grad[k], terms[k], noise)


@pytest.mark.parametrize("name", VC.CASES)
def test_the_float32_references_stay_within_the_recorded_margins_and_the_cap(name):
    view, reached = VC.view32(name), PC.reached(name)
    for filter, footprint in VC.FILTERS:
        unc = VC.uncertain(name, view, filter, footprint) & reached
        assert unc.sum() < VC.MAX_UNCERTAIN_REF * reached.sum(), (filter, footprint, int(unc.sum()))
        recorded = VC.MARGINS[f"{name}/{filter}/{footprint:g}"]
        for kind in VC.IMAGES:
            img, g = VC.image(kind, VC.res_of(name)), VC.d_color(name)
            bars = VC.dview_bars(VR.dview_ref(img, view, g, filter, footprint, 0, np.float32), VR.dview_ref(img, view, g, filter, footprint), ~unc)
            for (bar, err, top), m in zip(bars, recorded):       # (twice: log2 in float32 is the host library's)
                assert err <= max(2.0 * m, VC.FLOOR_ULPS * VC.EPS32 * top), (filter, footprint, kind, err, m)


def test_camera_tensor_round_trip():
    cam = Camera(0.6911, (0.1, 2.5, 6.25), (-0.2, 2.6, -2.5), (0.0, 1.0, 0.0))
    t = cam.to_tensor()
    assert t.dtype == torch.float32 and tuple(t.shape) == (10,) and t.device.type == "cpu" and not t.requires_grad
    assert t.tolist() == [float(np.float32(x)) for x in (cam.fov, *cam.origin, *cam.target, *cam.up)]
    back = Camera.from_tensor(t)
    assert back.to_tensor().tolist() == t.tolist()
    assert np.float32(back.fov) == np.float32(cam.fov) and tuple(np.float32(back.up)) == tuple(np.float32(list(cam.up)))
    with pytest.raises(ValueError):
        Camera.from_tensor(torch.zeros(9))
