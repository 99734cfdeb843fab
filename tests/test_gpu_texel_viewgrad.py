"""-m gpu: the camera gradients (include/zdr.h, "Camera gradients": zdr_texel_gather_dview, zdr_texel_view_backward; zdr_amd:
texel_gather_dview, Scene.texel_view_backward, camera tensors) against the float64 references of tests/texel_viewgrad_ref.py on the
cases of tests/texel_viewgrad_cases.py, and the properties the header states.

The kernels get the case's float32 sample points and their OWN view buffer; the references are evaluated on that very buffer (the
convention of ``texel_project_cases.linear_bar``).  d_view: a texel fails when a channel is off the float64 reference by more than
4 x the float32 reference's largest error (floor 4 float32 ulps of the channel's largest value); failing and uncertain texels together
may be 1 % of the reached ones.  The 10 camera sums: 4 x the float32 autograd's error, floor 4 ulps of the sum of |terms|.  Every figure
is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_texel_project as TP
import texel_cases as TC
import texel_mip_ref as MR
import texel_project_cases as PC
import texel_project_ref as PR
import texel_viewgrad_cases as VC
import texel_viewgrad_ref as VR
from zdr_amd import (Camera, Scene, image_pyramid_backward, image_pyramid_forward, texel_gather, texel_gather_dview, texel_gather_forward,
                     texel_gather_mip_backward, texel_gather_mip_forward)
from zdr_amd import _native as N
from zdr_amd import project as P

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -3            # ZDR_E_* of include/zdr.h
bits = TP.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def kernel_view(name):
    scene = TP.case_scene(name, "bvh")
    return scene, scene.texel_view_forward(TP.case_points(name), VC.res_of(name), camera=TP.camera(PC.CASES[name][1]))


def dview(img, view, g, filter, footprint, **kw):
    return texel_gather_dview(img, view, g, filter=filter, footprint=footprint, **kw)


# ------------------------------------------------------------------------------------------- d_view
@pytest.mark.parametrize("name", VC.CASES)
def test_dview_parity_with_the_float64_reference(name):
    _, view = kernel_view(name)
    v, reached = view.cpu().numpy(), PC.reached(name)
    g = dev(VC.d_color(name))
    for filter, footprint in VC.FILTERS:
        for kind in VC.IMAGES:
            got = dview(dev(VC.image(kind, VC.res_of(name))), view, g, filter, footprint).cpu().numpy()
            bad, unc, bars = VC.dview_check(name, kind, filter, footprint, v, got)
            off = int(((bad | unc) & reached).sum())
            print(f"[dview parity] {name} {filter} {footprint:g} {kind}: failing {int((bad & reached).sum())}, uncertain {int((unc & reached).sum())} of "
                  f"{int(reached.sum())}; bars " + " ".join(f"{b[0]:.3e}" for b in bars) + f"; largest " + " ".join(f"{b[2]:.3e}" for b in bars))
            assert off <= VC.MAX_UNCERTAIN * reached.sum(), (filter, footprint, kind)
            assert not got[~reached].any()
            if VC.res_of(name) != (1, 1) and filter == "bilinear":
                assert np.abs(got[..., 2:4]).sum() > 0


def test_invisible_texels_give_eight_zeros_and_read_nothing():
    name = "cbox_64x64_standard"
    res = VC.res_of(name)
    _, view = kernel_view(name)
    view = view.clone()
    view[..., 0] *= (view[..., 2] < 11.0)                         # nothing visible taps the pixels x >= 12 any more
    hidden = view[..., 0] == 0
    assert 0 < int(hidden.sum()) < hidden.numel()
    img, g = dev(VC.image("noise", res)), dev(VC.d_color(name))
    for filter, footprint in VC.FILTERS:
        clean = dview(img, view, g, filter, footprint)
        assert torch.isfinite(clean).all() and not clean[hidden].any() and float(clean[~hidden][..., 2:4].abs().sum()) > 0
        dirty_view, dirty_g = view.clone(), g.clone()
        dirty_view[..., 2][hidden] = float("nan"); dirty_view[..., 3][hidden] = float("inf"); dirty_view[..., 6][hidden] = float("nan")
        dirty_g[hidden] = float("nan")
        dirty_img = img.clone()
        if filter == "bilinear":                                  # (a NaN pixel would spread through the coarser levels of a pyramid)
            dirty_img[:, 13:] = float("nan")
        got = dview(dirty_img, dirty_view, dirty_g, filter, footprint, out=torch.full_like(clean, float("nan")))
        assert torch.equal(bits(got), bits(clean)), (filter, footprint)
    nan_vis = view.clone()
    nan_vis[..., 0][hidden] = float("nan")                        # a NaN visible is invisible
    assert torch.equal(bits(dview(img, nan_vis, g, "mip", 4.0)), bits(dview(img, view, g, "mip", 4.0)))


@pytest.mark.parametrize("name", ["cbox_16x16_standard", "cbox_64x64_inside"])
def test_mip_dview_is_the_bilinear_one_bit_for_bit_where_the_footprint_is_small(name):
    _, view = kernel_view(name)
    view = view.clone()
    view[..., 6] = torch.rand_like(view[..., 6]) * 0.249          # scale * footprint < 1 with footprint 4
    view[0, :3, 6] = torch.tensor([0.0, 0.25, float("nan")], device="cuda")
    img, g = dev(VC.image("noise", VC.res_of(name))), dev(VC.d_color(name))
    a, b = dview(img, view, g, "bilinear", 1.0), dview(img, view, g, "mip", 4.0)
    assert torch.equal(bits(a), bits(b)) and float(a.abs().sum()) > 0


def test_a_1x1_image_gives_no_gradient():
    name = "cbox_64x64_inside_1x1"
    _, view = kernel_view(name)
    assert int((view[..., 0] != 0).sum()) > 0
    img, g = dev(VC.image("noise", (1, 1))), dev(VC.d_color(name))
    for filter, footprint in VC.FILTERS:
        assert not dview(img, view, g, filter, footprint, out=torch.full_like(view, 3.0)).any()


def test_two_dview_runs_give_the_same_bits_whatever_the_output_held():
    name = "cbox_64x64_standard"
    _, view = kernel_view(name)
    img, g = dev(VC.image("smooth", VC.res_of(name))), dev(VC.d_color(name))
    for filter, footprint in VC.FILTERS:
        a = dview(img, view, g, filter, footprint, out=torch.zeros_like(view))
        b = dview(img, view, g, filter, footprint, out=torch.full_like(view, float("nan")))
        assert torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------- the camera sums
def camera_parity(tag, scene, pts, camera, res, g):
    got = scene.texel_view_backward(dev(pts), dev(g), res, camera=camera).cpu().numpy().astype(np.float64)
    g64, bars, err32, terms = VC.camera_bars(pts, camera, res, g)
    err = np.abs(got - g64)
    print(f"[camera parity] {tag}: kernel error / bar " + " ".join(f"{e:.2e}/{b:.2e}" for e, b in zip(err, bars)))
    print(f"[camera parity] {tag}: float32 reference error " + " ".join(f"{e:.2e}" for e in err32) + "; sum |terms| " + " ".join(f"{t:.2e}" for t in terms))
    assert np.isfinite(got).all() and (err <= bars).all(), (tag, err, bars)
    return got


@pytest.mark.parametrize("name", VC.CASES)
def test_texel_view_backward_parity_with_the_float64_autograd(name):
    scene = TP.case_scene(name, "bvh")
    pts = PC.points(name)
    got = camera_parity(name, scene, pts, TP.camera(PC.CASES[name][1]), VC.res_of(name), VC.d_view(pts.shape))
    assert np.abs(got).sum() > 0


# 384 x 352 = 135,168 texels = 528 partial rows: more rows than stage 2 has lanes (256), 33 rows to each of its 16 sub-sums;
# 37 x 29 = 1,073 texels = 4 full workgroups and a fifth with 49 texels: a last wave with idle lanes and three waves without any;
# 520 x 512 = 266,240 texels: more than 1,024 workgroups' worth (262,144), so the grid is capped and a lane adds more than one texel
@pytest.mark.parametrize("shape", [(384, 352), (37, 29), (520, 512)])
def test_the_reduction_across_its_loop_boundaries(shape):
    scene = TP.case_scene("cbox_16x16_standard", "bvh")
    pts = VC.planar_points(*shape)
    g = VC.d_view(pts.shape, seed=1)
    n = shape[0] * shape[1]
    assert N.lib().zdr_texel_view_backward_workspace_bytes(*shape) == 128 * min((n + 255) // 256, 1024)
    camera_parity(f"planar {shape[0]} x {shape[1]}", scene, pts, TP.camera("standard"), (96, 64), g)


def planted(name):
    """a case's points with NaN positions and normals planted, its d_view, and the mask of texels that are not shaded"""
    pts = PC.points(name).copy()
    rng = np.random.default_rng(5)
    ys, xs = np.nonzero(PR.shaded(pts))
    pick = rng.choice(ys.size, 12, replace=False)
    pts[ys[pick[:6]], xs[pick[:6]], 8] = np.nan
    pts[ys[pick[6:]], xs[pick[6:]], 5] = np.nan
    return pts, VC.d_view(pts.shape, seed=2), ~PR.shaded(pts)


def test_unshaded_texels_and_floats_0_and_7_contribute_nothing():
    name = "cbox_64x64_standard"
    scene, cam, res = TP.case_scene(name, "bvh"), TP.camera("standard"), VC.res_of(name)
    pts, g, off = planted(name)
    assert off.sum() > 12
    clean = scene.texel_view_backward(dev(pts), dev(g), res, camera=cam)
    assert torch.isfinite(clean).all() and float(clean.abs().sum()) > 0
    dirty = g.copy()
    dirty[off] = np.nan                                           # the rows of texels that are not shaded are not read
    dirty[..., 0] = np.nan; dirty[..., 7] = np.inf                # floats 0 and 7 are ignored
    assert torch.equal(bits(scene.texel_view_backward(dev(pts), dev(dirty), res, camera=cam)), bits(clean))
    camera_parity(name + " planted", scene, pts, cam, res, g)


def test_texels_behind_the_camera_contribute_through_cosine_depth_and_distance_only():
    name = "cbox_64x64_inside"
    scene, cam, res = TP.case_scene(name, "bvh"), TP.camera("inside"), VC.res_of(name)
    pts, g = PC.points(name), VC.d_view(PC.points(name).shape, seed=3)
    behind = PR.shaded(pts) & ~PC.reference(name)["front"] & ~PC.reference(name)["uncertain"]
    assert behind.sum() > 100
    clean = scene.texel_view_backward(dev(pts), dev(g), res, camera=cam)
    dirty = g.copy()
    for c in (2, 3, 6):
        dirty[..., c][behind] = np.nan                            # X, Y and scale are the constant 0 there
    assert torch.isfinite(clean).all() and torch.equal(bits(scene.texel_view_backward(dev(pts), dev(dirty), res, camera=cam)), bits(clean))
    less = g.copy()
    for c in (1, 4, 5):
        less[..., c][behind] = 0.0
    assert not torch.equal(bits(scene.texel_view_backward(dev(pts), dev(less), res, camera=cam)), bits(clean))
    only = np.zeros_like(g)
    for c in (1, 4, 5):
        only[..., c][behind] = g[..., c][behind]
    camera_parity(name + " behind only", scene, pts, cam, res, only)


def test_two_backward_runs_give_the_same_bits_whatever_the_workspace_held():
    name = "cbox_64x64_standard"
    scene, cam, res = TP.case_scene(name, "bvh"), TP.camera("standard"), VC.res_of(name)
    for pts in (PC.points(name), VC.planar_points(384, 352)):
        g = dev(VC.d_view(pts.shape, seed=4))
        need = N.lib().zdr_texel_view_backward_workspace_bytes(pts.shape[0], pts.shape[1])
        a = scene.texel_view_backward(dev(pts), g, res, camera=cam, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"),
                                      out=torch.zeros(10, device="cuda"))
        b = scene.texel_view_backward(dev(pts), g, res, camera=cam, workspace=torch.full((need + 64,), 0xAB, dtype=torch.uint8, device="cuda"),
                                      out=torch.full((10,), float("nan"), device="cuda"))
        assert torch.equal(bits(a), bits(b)) and float(a.abs().sum()) > 0


# ------------------------------------------------------------------------------------------- end to end
def reference_camera_grads(pts, cameras, photos, views, footprint, loss, np_dtype, t_dtype):
    """the gradient of ``loss(colors, cosines, visibles)`` in each camera: the loss itself by autograd on the CPU in ``t_dtype`` from the
    reference's colours on the kernel's view buffers, then ``dview_ref`` and ``camera_grad_ref``.  -> [(gradient, sum of |terms|)]"""
    colors = [torch.tensor(MR.gather_mip_ref(p, v, footprint, dtype=np_dtype).astype(np.float64), dtype=t_dtype, requires_grad=True) for p, v in zip(photos, views)]
    cosines = [torch.tensor(v[..., 1].astype(np.float64), dtype=t_dtype, requires_grad=True) for v in views]
    loss(colors, cosines, [torch.tensor(v[..., 0].astype(np.float64), dtype=t_dtype) for v in views]).backward()
    out = []
    for cam, p, v, c, cs in zip(cameras, photos, views, colors, cosines):
        res = (p.shape[1], p.shape[0])
        d = VR.dview_ref(p, v, c.grad.double().numpy(), "mip", footprint, dtype=np_dtype).astype(np.float64)
        d[..., 1] = cs.grad.double().numpy()
        out.append(VR.camera_grad_ref(pts, cam, res, d, t_dtype, terms=True))
    return out


def check_camera_grads(tag, pts, cameras, photos, views, footprint, loss, grads):
    r64 = reference_camera_grads(pts, cameras, photos, views, footprint, loss, np.float64, torch.float64)
    r32 = reference_camera_grads(pts, cameras, photos, views, footprint, loss, np.float32, torch.float32)
    for i, (got, (g64, terms), (g32, _)) in enumerate(zip(grads, r64, r32)):
        bars = np.maximum(4.0 * np.abs(g32 - g64), VC.FLOOR_ULPS * VC.EPS32 * terms)
        err = np.abs(got.double().numpy() - g64)
        print(f"[camera end to end] {tag} view {i}: gradient " + " ".join(f"{x:.3e}" for x in g64))
        print(f"[camera end to end] {tag} view {i}: kernel error / bar " + " ".join(f"{e:.2e}/{b:.2e}" for e, b in zip(err, bars)))
        assert (err <= bars).all() and np.abs(g64).sum() > 0, (tag, i, err, bars)


def cbox_scene():
    scene = Scene(TC.cbox_arrays(), integrator="direct")
    scene.camera = TP.camera("standard")
    return scene


def test_a_camera_tensor_receives_the_gradient_of_a_texture_space_loss():
    scene = cbox_scene()
    gen = torch.Generator().manual_seed(7)
    material = torch.rand(64, 64, 4, generator=gen).cuda()
    texels = scene.texel_aovs(material)
    photo = torch.rand(32, 48, 4, generator=gen).cuda()
    theta = torch.rand(64, 64, 4, generator=gen).cuda()
    cam = TP.camera("standard").to_tensor().requires_grad_()
    view = scene.texel_view(material, res=(48, 32), camera=cam, texels=texels)
    assert view.data.requires_grad
    fixed = scene.texel_view(material, res=(48, 32), camera=TP.camera("standard"), texels=texels)
    assert torch.equal(bits(view.data.detach()), bits(fixed.data))          # the forward bits are those of the Camera
    color = view.gather(photo, filter="mip", footprint=4)
    assert torch.equal(bits(color.detach()), bits(fixed.gather(photo, filter="mip", footprint=4)))
    (view.weight()[..., None] * (color - theta).square()).sum().backward()
    assert cam.grad is not None and cam.grad.device.type == "cpu" and tuple(cam.grad.shape) == (10,)

    def loss(colors, cosines, visibles):
        return ((visibles[0] * cosines[0].abs())[..., None] * (colors[0] - theta.cpu().to(colors[0].dtype)).square()).sum()
    check_camera_grads("one view", texels.data.cpu().numpy(), [PC.CAMERAS["standard"]], [photo.cpu().numpy()], [fixed.data.cpu().numpy()], 4.0, loss, [cam.grad])


def test_texel_project_passes_gradient_to_two_camera_tensors():
    scene = cbox_scene()
    gen = torch.Generator().manual_seed(8)
    material = torch.rand(64, 64, 4, generator=gen).cuda()
    texels = scene.texel_aovs(material)
    photos = [torch.rand(32, 48, 4, generator=gen).cuda(), torch.rand(24, 40, 4, generator=gen).cuda()]
    theta = torch.rand(64, 64, 4, generator=gen).cuda()
    names = ("standard", "inside")
    cams = [TP.camera(n).to_tensor().requires_grad_() for n in names]
    proj = scene.texel_project(list(zip(cams, photos)), material, texels=texels, filter="mip", footprint=2.0)
    still = scene.texel_project([(TP.camera(n), p) for n, p in zip(names, photos)], material, texels=texels, filter="mip", footprint=2.0)
    assert torch.equal(bits(proj.color.detach()), bits(still.color)) and not still.color.requires_grad
    (proj.color - theta).square().sum().backward()

    def loss(colors, cosines, visibles):
        ws = [v * c.abs() for v, c in zip(visibles, cosines)]
        num, weight = ws[0][..., None] * colors[0] + ws[1][..., None] * colors[1], ws[0] + ws[1]
        seen = weight > 0
        color = torch.where(seen[..., None], num / torch.where(seen, weight, torch.ones_like(weight))[..., None], torch.zeros_like(num))
        return (color - theta.cpu().to(color.dtype)).square().sum()
    views = [scene.texel_view(material, res=(p.shape[1], p.shape[0]), camera=TP.camera(n), texels=texels).data.cpu().numpy() for n, p in zip(names, photos)]
    check_camera_grads("two views", texels.data.cpu().numpy(), [PC.CAMERAS[n] for n in names], [p.cpu().numpy() for p in photos], views, 2.0, loss,
                       [c.grad for c in cams])


def test_a_camera_object_stays_on_the_paths_it_took():
    scene = cbox_scene()
    gen = torch.Generator().manual_seed(9)
    material = torch.rand(64, 64, 4, generator=gen).cuda()
    texels = scene.texel_aovs(material)
    photo = torch.rand(32, 48, 4, generator=gen).cuda().requires_grad_()
    y = torch.randn(64, 64, 4, generator=gen).cuda()
    for camera in (TP.camera("standard"), TP.camera("standard").to_tensor()):        # a tensor without grad is read and nothing more
        view = scene.texel_view(material, res=(48, 32), camera=camera, texels=texels)
        assert view.data.requires_grad is False and view.data.grad_fn is None
        assert torch.equal(bits(view.data), bits(scene.texel_view_forward(texels.data, (48, 32), camera=TP.camera("standard"))))
        out = view.gather(photo, filter="mip", footprint=4)
        assert type(out.grad_fn).__name__ == "TexelGatherMipOperatorBackward"
        assert torch.equal(bits(out.detach()), bits(texel_gather_mip_forward(photo.detach(), image_pyramid_forward(photo.detach()), view.data, 4.0)))
        assert type(view.gather(photo).grad_fn).__name__ == "TexelGatherOperatorBackward"
        assert torch.equal(bits(view.gather(photo).detach()), bits(texel_gather_forward(photo.detach(), view.data)))
        grad, = torch.autograd.grad(out, photo, y)
        d_image, d_pyramid = texel_gather_mip_backward(y, view.data, (48, 32), 4.0)
        want = image_pyramid_backward(d_pyramid, (48, 32), d_image=d_image)
        assert float((grad - want).abs().max()) <= 1e-5 * float(want.abs().max())    # (float atomics: the order of addition varies)


# ------------------------------------------------------------------------------------------- errors
def test_wrong_arguments_raise():
    scene = cbox_scene()
    material = torch.rand(16, 16, 4, device="cuda")
    texels = scene.texel_aovs(material)
    photo = torch.rand(16, 24, 4, device="cuda")
    cam = TP.camera("standard").to_tensor().requires_grad_()
    with pytest.raises(ValueError):
        scene.texel_view(material, res=(24, 16), camera=cam.detach().cuda(), texels=texels)      # a device tensor
    with pytest.raises(ValueError):
        scene.texel_view_forward(texels.data, (24, 16), camera=torch.zeros(9))
    with pytest.raises(ValueError):
        scene.texel_view_forward(texels.data, (24, 16), camera=cam.detach().double())
    view = scene.texel_view(material, res=(24, 16), camera=cam, texels=texels, footprint=True)
    with pytest.raises(ValueError):
        view.gather(photo, plan=True)
    with pytest.raises(ValueError):
        view.gather(photo, filter="aniso")
    with pytest.raises(ValueError):
        scene.texel_project([(cam, photo)], material, texels=texels, filter="aniso")
    with pytest.raises(ValueError):
        scene.texel_project([(cam, photo)], material, texels=texels, plan=True)
    data, g = view.data.detach(), torch.rand(16, 16, 4, device="cuda")
    with pytest.raises(ValueError):
        texel_gather_dview(photo, data, g, filter="aniso")
    with pytest.raises(ValueError):
        texel_gather_dview(photo, data, g[:8].contiguous())
    with pytest.raises(ValueError):
        texel_gather_dview(photo, data, g, filter="mip", footprint=0.0)
    with pytest.raises(ValueError):
        texel_gather_dview(photo, data, g, out=torch.zeros(16, 16, 4, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_view_backward(texels.data, torch.zeros(16, 16, 4, device="cuda"), (24, 16))
    with pytest.raises(ValueError):
        scene.texel_view_backward(texels.data, torch.zeros(16, 16, 8, device="cuda"), (24, 16), out=torch.zeros(9, device="cuda"))
    with pytest.raises(ValueError):
        scene.texel_view_backward(texels.data, torch.zeros(16, 16, 8, device="cuda"), (24, 16), workspace=torch.zeros(64, dtype=torch.uint8, device="cuda"))
    # the C entry points themselves
    L = N.lib()
    pyr = image_pyramid_forward(photo)
    out = torch.zeros(16, 16, 8, device="cuda")

    def dparams(**kw):
        p = N.TexelGatherDviewParams()
        p.struct_size = C.sizeof(N.TexelGatherDviewParams)
        p.tex_h, p.tex_w, p.width, p.height, p.filter, p.levels, p.footprint = 16, 16, 24, 16, 1, 0, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def dcall(p, view=data.data_ptr(), image=photo.data_ptr(), pyramid=pyr.data_ptr(), d_color=g.data_ptr(), d_view=out.data_ptr()):
        return L.zdr_texel_gather_dview(C.byref(p), view, image, pyramid, d_color, d_view, scene._stream())
    assert dcall(dparams()) == 0 and dcall(dparams(filter=0), pyramid=None) == 0
    for bad in (dparams(struct_size=4), dparams(tex_h=0), dparams(width=-1), dparams(levels=-1), dparams(filter=3), dparams(filter=-1),
                dparams(footprint=0.0), dparams(footprint=float("nan")), dparams(footprint=float("inf"))):
        assert dcall(bad) == E_INVALID
    assert dcall(dparams(filter=2)) == E_UNSUPPORTED and dcall(dparams(tex_h=1 << 14, tex_w=(1 << 12) + 1)) == E_UNSUPPORTED
    assert dcall(dparams(), view=None) == E_INVALID and dcall(dparams(), pyramid=None) == E_INVALID and dcall(dparams(), d_view=None) == E_INVALID
    assert dcall(dparams(), d_color=g.data_ptr() + 4) == E_INVALID                    # misaligned
    assert dcall(dparams(), d_view=data.data_ptr()) == E_INVALID                      # the output on an input
    assert dcall(dparams(), d_view=g.data_ptr()) == E_INVALID
    need = L.zdr_texel_view_backward_workspace_bytes(16, 16)
    assert need == 128 and L.zdr_texel_view_backward_workspace_bytes(0, 16) == 0 and L.zdr_texel_view_backward_workspace_bytes(1 << 14, (1 << 12) + 1) == 0
    from zdr_amd.render import _camera_pod
    ws, d_cam, d_view = torch.zeros(need, dtype=torch.uint8, device="cuda"), torch.zeros(16, device="cuda"), torch.zeros(16, 16, 8, device="cuda")

    def vparams(**kw):
        p = N.TexelViewParams()
        p.struct_size = C.sizeof(N.TexelViewParams)
        p.tex_h, p.tex_w, p.width, p.height, p.camera = 16, 16, 24, 16, _camera_pod(TP.camera("standard"))
        for k, v in kw.items():
            if k == "fov":
                p.camera.fov = v
            else:
                setattr(p, k, v)
        return p

    def vcall(p, pts=texels.data.data_ptr(), dv=d_view.data_ptr(), dc=d_cam.data_ptr(), w=ws.data_ptr()):
        return L.zdr_texel_view_backward(C.byref(p), pts, dv, dc, w, scene._stream())
    assert vcall(vparams()) == 0
    for bad in (vparams(struct_size=8), vparams(tex_w=0), vparams(height=0), vparams(fov=0.0), vparams(fov=3.2), vparams(fov=float("nan"))):
        assert vcall(bad) == E_INVALID
    assert vcall(vparams(tex_h=1 << 14, tex_w=(1 << 12) + 1)) == E_UNSUPPORTED
    assert vcall(vparams(), pts=None) == E_INVALID and vcall(vparams(), dv=None) == E_INVALID and vcall(vparams(), dc=None) == E_INVALID
    assert vcall(vparams(), w=None) == E_INVALID and vcall(vparams(), dc=d_cam.data_ptr() + 4) == E_INVALID
    assert vcall(vparams(), dc=ws.data_ptr()) == E_INVALID and vcall(vparams(), w=d_view.data_ptr()) == E_INVALID
    torch.cuda.synchronize()
    scene.check()
