"""-m gpu: the anisotropic gather (texel_footprint_forward, texel_gather(..., filter="aniso"); include/zdr.h, zdr_texel_footprint,
zdr_texel_gather_aniso, zdr_texel_gather_aniso_backward) against the reference of tests/texel_aniso_ref.py.

The footprint buffer is held against the float64 reference under the bars of tests/texel_aniso_cases.py.  The gather's exact families
are compared bit for bit with the mip gather and the bilinear gather; with several probes it and the full adjoint are held against the
float64 reference on the kernel's OWN view and footprint buffers under the project's rule (4 x the float32 reference's own error
against float64, floor 4 float32 ulps of the largest value), the texels within 1e-4 of a switch of the probe count or of a clamp left
out (``texel_aniso_ref.exempt``; at most 1 % of the visible texels may be exempt or failing).  The adjoint's cotangent is drawn from
[0, 1), for the reason given in tests/test_gpu_texel_mip.py.  Every figure is printed before it is asserted."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_gpu_texel_project as TP
import texel_aniso_cases as AC
import texel_aniso_ref as AR
import texel_cases as TC
import texel_mip_ref as MR
import texel_project_ref as PR
from test_texel_aniso_ref_host import synthetic_footprint
from test_texel_mip_ref_host import synthetic
from zdr_amd import (Scene, TexelFootprint, TexelView, image_pyramid_backward, image_pyramid_forward, texel_footprint_forward, texel_gather,
                     texel_gather_aniso_backward, texel_gather_aniso_forward, texel_gather_forward, texel_gather_mip_forward)
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -3            # ZDR_E_* of include/zdr.h
SIZES = [(96, 64), (33, 17), (7, 5), (1, 1)]           # (width, height)
bits = TP.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@functools.lru_cache(None)
def buffers(name, res=AC.RES):
    """the kernels' own view and footprint buffers of a case, (H, W, 8) and (H, W, 4) on the GPU"""
    cam = TP.camera(AC.CASES[name][1])
    pts = TP.case_points(name)
    view = TP.case_scene(name, "bvh").texel_view_forward(pts, res, camera=cam)
    fp = texel_footprint_forward(pts, res, cam)
    torch.cuda.synchronize()
    return view, fp


# ------------------------------------------------------------------------------------------- the footprint buffer
@pytest.mark.parametrize("name", list(AC.CASES))
def test_footprint_parity_with_the_float64_reference(name):
    _, fp = buffers(name)
    got = fp.cpu().numpy()
    vis, ref = AC.visible(name), AC.view_reference(name)
    err = AC.footprint_errors(name, got)[vis].max(0)
    fail = AC.footprint_failing(name, got)
    print(f"[texel footprint parity] {name}: visible {int(vis.sum())}, failing {int(fail.sum())}")
    for q, e, bar, margin in zip(AC.QUANTITIES, err, AC.footprint_bars(name), AC.MARGINS[name]):
        print(f"    {q}: kernel vs float64 largest {e:.3e}; float32 reference {margin:.3e}; bar {bar:.3e}")
    shaded = PR.shaded(AC.points(name))
    assert (got[~shaded] == 0).all()                                              # four zeros where the texel is not shaded ...
    behind = shaded & ~ref["front"] & ~ref["uncertain"]
    assert (got[behind] == 0).all() and (name != "cbox_64x64_inside" or int(behind.sum()) > 100)     # ... or lies behind the camera
    assert np.isfinite(got).all() and float(np.abs(got[vis]).sum()) > 0
    assert int(fail.sum()) <= AC.MAX_EXEMPT * vis.sum(), (name, int(fail.sum()))
    pts, cam = TP.case_points(name), TP.camera(AC.CASES[name][1])
    again = texel_footprint_forward(pts, AC.RES, cam, out=torch.full_like(fp, float("nan")))        # the same bits from run to run, whatever out held
    assert torch.equal(bits(again), bits(fp))
    assert isinstance(TexelView(buffers(name)[0], AC.RES, fp).footprint, TexelFootprint)
    f = TexelView(buffers(name)[0], AC.RES, fp).footprint
    assert f.major_axis.shape == fp.shape[:2] + (2,) and torch.equal(f.minor, fp[..., 2]) and torch.equal(f.major, fp[..., 3])


def test_a_nan_in_a_position_or_a_reach_of_zero_gives_four_zeros_and_leaves_the_others_alone():
    name = "cbox_16x16_standard"
    pts = TP.case_points(name).clone()
    cam = TP.camera("standard")
    clean = texel_footprint_forward(pts, AC.RES, cam)
    ys, xs = np.nonzero(AC.visible(name))
    pts[ys[0], xs[0], 9] = float("nan"); pts[ys[1], xs[1], 5] = float("nan"); pts[ys[2], xs[2], 12] = 0.0
    got = texel_footprint_forward(pts, AC.RES, cam)
    hit = torch.zeros(clean.shape[:2], dtype=torch.bool, device="cuda")
    for i in range(3):
        hit[ys[i], xs[i]] = True
    assert (got[hit] == 0).all() and (clean[hit][:, 3] > 0).all() and torch.equal(bits(got[~hit]), bits(clean[~hit]))


# ------------------------------------------------------------------------------------------- the gather on synthetic buffers
@pytest.mark.parametrize("res", SIZES)
def test_the_exact_families_bit_for_bit(res):
    rng = np.random.default_rng(41)
    w, h = res
    image = dev(rng.normal(size=(h, w, 4)))
    pyr = image_pyramid_forward(image)
    view = synthetic(rng, 400, res)
    # 1. major_axis = (scale, 0), minor = major = scale: the mip gather's bits at footprints 1, 3 and 0.5
    iso = np.zeros((400, 1, 4), np.float32)
    iso[:, 0, 0] = iso[:, 0, 2] = iso[:, 0, 3] = view[:, 0, 6]
    for footprint in (1.0, 3.0, 0.5):
        got = texel_gather_aniso_forward(image, pyr, dev(view), dev(iso), footprint)
        assert torch.equal(bits(got), bits(texel_gather_mip_forward(image, pyr, dev(view), footprint))), (res, footprint)
    # 2. max_aniso = 1 with major = scale: the mip gather's bits, whatever the axis and the minor axis
    fp = synthetic_footprint(rng, 400)
    fp[:, 0, 3] = view[:, 0, 6]; fp[:, 0, 2] = view[:, 0, 6] * rng.uniform(0.05, 1.0, 400).astype(np.float32)
    got = texel_gather_aniso_forward(image, pyr, dev(view), dev(fp), 1.0, 1)
    assert torch.equal(bits(got), bits(texel_gather_mip_forward(image, pyr, dev(view), 1.0))), res
    # 3. wherever major x footprint <= 1 the bits are the bilinear gather's
    fp = synthetic_footprint(rng, 400, major=(0.01, 1.0))
    fp[0, 0, 2:] = 1.0                                                            # (exactly 1: not A > 1)
    assert torch.equal(bits(texel_gather_aniso_forward(image, pyr, dev(view), dev(fp))), bits(texel_gather_forward(image, dev(view)))), res
    fp = synthetic_footprint(rng, 400, major=(0.5, 8.0))
    small = torch.from_numpy(fp[:, 0, 3] * np.float32(0.25) <= 1).cuda()
    got = texel_gather_aniso_forward(image, pyr, dev(view), dev(fp), 0.25)
    assert int(small.sum()) > 50 and torch.equal(bits(got[small]), bits(texel_gather_forward(image, dev(view))[small])), res
    # 4. what lies behind an invisible texel never reaches the result: X, Y, the footprint row, the image and the pyramid
    fp = synthetic_footprint(rng, 400)
    clean = texel_gather_aniso_forward(image, pyr, dev(view), dev(fp))
    off = view[:, 0, 0] == 0
    dirty, dirty_fp = view.copy(), fp.copy()
    dirty[off, 0, 2] = np.nan; dirty[off, 0, 3] = 1e30; dirty_fp[off] = np.nan
    got = texel_gather_aniso_forward(image, pyr, dev(dirty), dev(dirty_fp), out=torch.full((400, 1, 4), float("nan"), device="cuda"))
    assert torch.equal(bits(got), bits(clean)) and (got[torch.from_numpy(off).cuda()] == 0).all() and not torch.isnan(got).any()
    dirty[:, 0, 0] = 0
    assert (texel_gather_aniso_forward(torch.full_like(image, float("nan")), torch.full_like(pyr, float("nan")), dev(dirty), dev(dirty_fp)) == 0).all()
    # 5. a constant image comes out as visible x the constant within 2 ulps (N (1 / N) rounds); visible is 0 or 1 here
    const = torch.full((h, w, 4), 0.3, device="cuda")
    got = texel_gather_aniso_forward(const, image_pyramid_forward(const), dev(view), dev(fp)).cpu().numpy().astype(np.float64)
    err = float(np.abs(got - view[..., 0:1].astype(np.float64) * np.float64(np.float32(0.3))).max())
    print(f"[texel aniso constant] {res}: largest error {err / float(np.spacing(np.float32(0.3))):.2f} ulps")
    assert err <= 2 * float(np.spacing(np.float32(0.3)))


# ------------------------------------------------------------------------------------------- parity with several probes
def parity(tag, image, g, view, fp, res, footprint, max_aniso, levels=0, visible_only=True):
    """gather and full adjoint of the kernels on the GPU buffers ``view``, ``fp`` against the references on the same buffers"""
    v, f = view.cpu().numpy(), fp.cpu().numpy()
    flat_vis = (v[..., 0] != 0) & ~np.isnan(v[..., 0])
    ex = AR.exempt(f, footprint, max_aniso) & flat_vis
    keep = ~ex
    counts = np.bincount(AR.probes(f[flat_vis], footprint, max_aniso)[0], minlength=max_aniso + 1)[1:].tolist()
    r64, r32 = AR.gather_aniso_ref(image, v, f, footprint, max_aniso, levels), AR.gather_aniso_ref(image, v, f, footprint, max_aniso, levels, np.float32)
    bar = AC.gather_bar(r32, r64, keep)
    gpu_image = dev(image)
    got = texel_gather_aniso_forward(gpu_image, image_pyramid_forward(gpu_image, levels), view, fp, footprint, max_aniso, levels).cpu().numpy()
    err = np.abs(got - r64).max(-1)
    fail = ~(err <= bar) & keep
    print(f"[texel aniso parity] {tag} {res} footprint {footprint} max_aniso {max_aniso}: visible {int(flat_vis.sum())}, N = 1 .. {max_aniso}: {counts}, "
          f"exempt {int(ex.sum())}, failing {int(fail.sum())}; kernel vs float64 {float(err[keep].max()):.3e}; float32 reference "
          f"{float(np.abs(r32 - r64)[keep].max()):.3e}; bar {bar:.3e}")
    assert float(np.abs(got).sum()) > 0 and int((fail | ex).sum()) <= AC.MAX_EXEMPT * flat_vis.sum()
    g = np.where(ex[..., None], np.float32(0.0), g).astype(np.float32)            # an exempt texel sends nothing back
    a64 = AR.gather_aniso_adjoint_ref(g, v, f, res, footprint, max_aniso, levels)
    a32 = AR.gather_aniso_adjoint_ref(g, v, f, res, footprint, max_aniso, levels, np.float32)
    bar = AC.gather_bar(a32, a64)
    d_image, d_pyramid = texel_gather_aniso_backward(dev(g), view, fp, res, footprint, max_aniso, levels)
    d = image_pyramid_backward(d_pyramid, res, levels, d_image=d_image).cpu().numpy()
    err = float(np.abs(d - a64).max())
    print(f"[texel aniso adjoint parity] {tag} {res} footprint {footprint} max_aniso {max_aniso}: kernel vs float64 transpose {err:.3e}; float32 "
          f"reference {float(np.abs(a32 - a64).max()):.3e}; bar {bar:.3e}; largest |d_image| {np.abs(a64).max():.3e}")
    assert err <= bar and float(np.abs(d).sum()) > 0
    return counts


@pytest.mark.parametrize("footprint", [1.0, 0.5])
@pytest.mark.parametrize("max_aniso", [8, 2])
@pytest.mark.parametrize("res", [(96, 64), (33, 17)])
@pytest.mark.parametrize("name", list(AC.CASES))
def test_gather_and_full_adjoint_parity_on_the_kernels_own_buffers(name, res, max_aniso, footprint):
    view, fp = buffers(name, res)
    rng = np.random.default_rng(43)
    image = rng.uniform(0, 1, (res[1], res[0], 4)).astype(np.float32)
    g = rng.uniform(0, 1, tuple(view.shape[:2]) + (4,)).astype(np.float32)
    counts = parity(name, image, g, view, fp, res, footprint, max_aniso)
    if res == AC.RES and footprint == 1.0:
        assert sum(counts[1:]) > 0                                                # several probes are in play ...
        if max_aniso == 2 or name in ("cbox_16x16_standard", "multi_24_standard"):
            assert counts[-1] > 0                                                 # ... and the clamp to max_aniso


@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("max_aniso", [8, 16])
def test_gather_and_full_adjoint_parity_across_the_border_and_through_every_level(max_aniso, levels):
    """positions all over a 33 x 17 image and axes of up to 60 pixels in any direction: probes leave the image on every side (their taps
    are clamped to it), and minor axes from 0.2 to 60 pixels read every level; with ``levels=2`` everything from 4 pixels on reads the
    last level the pyramid has"""
    res = (33, 17)
    rng = np.random.default_rng(44)
    v = synthetic(rng, 600, res)
    fp = synthetic_footprint(rng, 600, major=(0.5, 60.0), ratio=(1.0, 24.0))
    image, g = rng.uniform(0, 1, (res[1], res[0], 4)).astype(np.float32), rng.uniform(0, 1, (600, 1, 4)).astype(np.float32)
    on = v[:, 0, 0] == 1
    N_, s = AR.probes(fp[on], 1.0, max_aniso)
    l0, _ = MR.level_split(s, 1.0, len(MR.layout(res, levels)) - 1)
    assert len(set(l0.tolist())) == (3 if levels else 6) and N_.max() == max_aniso
    t = (2.0 * (N_ - 1) + 1 - N_) / (2 * N_)                                     # the last probe of every texel
    X = v[on, 0, 2] + t * fp[on, 0, 0]
    assert (X < -1).any() or (X > res[0] + 1).any()
    parity("synthetic", image, g, dev(v), dev(fp), res, 1.0, max_aniso, levels)


# ------------------------------------------------------------------------------------------- quality
@pytest.mark.parametrize("name", ["cbox_16x16_standard", "cbox_64x64_standard"])
def test_the_quality_condition_on_the_kernels_own_output(name):
    view, fp = buffers(name)
    for label, image in AC.images().items():
        image = image.astype(np.float32)
        truth = AR.truth_ref(image, AC.points(name), AC.camera(name), AC.RES)
        gpu_image = dev(image)
        pyr = image_pyramid_forward(gpu_image)
        aniso = AC.rmse(name, texel_gather_aniso_forward(gpu_image, pyr, view, fp).cpu().numpy(), truth)
        others = {"bilinear": AC.rmse(name, texel_gather_forward(gpu_image, view).cpu().numpy(), truth),
                  "mip 1": AC.rmse(name, texel_gather_mip_forward(gpu_image, pyr, view, 1.0).cpu().numpy(), truth),
                  "mip 0.5": AC.rmse(name, texel_gather_mip_forward(gpu_image, pyr, view, 0.5).cpu().numpy(), truth)}
        print(f"[texel aniso quality] {name} {label}: aniso {aniso:.4f}  " + "  ".join(f"{k} {v:.4f}" for k, v in others.items())
              + f"  (aniso / best other {aniso / min(others.values()):.2f})")
        for k, v in others.items():
            assert aniso < v, (name, label, k, aniso, v)


# ------------------------------------------------------------------------------------------- autograd
def test_the_gradient_passes_through_the_aniso_gather_and_is_zero_where_no_probe_reaches():
    name = "cbox_64x64_standard"
    res = AC.RES
    view, fp = buffers(name)
    view = view.clone()
    view[..., 0] *= (view[..., 2] < 40.0)                          # nothing visible lies right of x = 40 ...
    gen = torch.Generator().manual_seed(5)
    image = torch.rand(res[1], res[0], 4, generator=gen).cuda().requires_grad_()
    y = torch.rand(64, 64, 4, generator=gen).cuda()
    tv = TexelView(view, res, fp)
    out = texel_gather(image, tv, filter="aniso")
    assert out.requires_grad and torch.equal(bits(out.detach()), bits(texel_gather_aniso_forward(image, image_pyramid_forward(image), view, fp)))
    out.backward(y)
    v, f = view.cpu().numpy(), fp.cpu().numpy()
    a64 = AR.gather_aniso_adjoint_ref(y.cpu().numpy(), v, f, res)
    bar = AC.gather_bar(AR.gather_aniso_adjoint_ref(y.cpu().numpy(), v, f, res, dtype=np.float32), a64)
    err = float(np.abs(image.grad.cpu().numpy() - a64).max())
    untouched = torch.from_numpy((a64 == 0).all(-1)).cuda()         # ... so, the cotangent and every weight being >= 0, exactly the pixels no tap reaches
    print(f"[texel aniso autograd] image.grad vs float64 transpose {err:.3e}; bar {bar:.3e}; pixels no probe's taps reach {int(untouched.sum())}")
    assert err <= bar and int(untouched.sum()) > 500 and (image.grad[untouched] == 0).all() and float(image.grad.abs().sum()) > 0
    vg, fg = view.clone().requires_grad_(), fp.clone().requires_grad_()
    grads = torch.autograd.grad(texel_gather(image, TexelView(vg, res, fg), filter="aniso").sum(), [image, vg, fg], allow_unused=True)
    assert grads[1] is None and grads[2] is None                   # the view and the footprint buffer receive none


def test_the_defaults_keep_their_bits_and_texel_project_composes_the_aniso_gather():
    scene = Scene(TC.cbox_arrays(), integrator="direct")
    scene.camera = TP.camera("standard")
    material = torch.rand(16, 16, 4, device="cuda")
    texels = scene.texel_aovs(material)
    gen = torch.Generator().manual_seed(6)
    photo = torch.rand(64, 96, 4, generator=gen).cuda().requires_grad_()
    plain_view = scene.texel_view(material, res=(96, 64), texels=texels)
    assert plain_view.footprint_data is None and plain_view.footprint is None     # the default: nothing is computed
    view = scene.texel_view(material, res=(96, 64), texels=texels, footprint=True)
    assert torch.equal(bits(view.data), bits(plain_view.data))
    assert torch.equal(bits(view.footprint_data), bits(texel_footprint_forward(texels.data, (96, 64), scene.camera)))
    assert float(((view.footprint.major > 1.125 * view.footprint.minor) & (view.visible == 1)).sum()) > 20
    assert torch.equal(view.footprint.major_axis, view.footprint_data[..., 0:2])
    pyr = image_pyramid_forward(photo)
    plain = texel_gather_forward(photo, view)
    for v in (view, plain_view):                                                  # every default and filter="mip" return the bits they returned
        assert torch.equal(bits(texel_gather(photo, v).detach()), bits(plain)) and torch.equal(bits(v.gather(photo).detach()), bits(plain))
        for footprint in (0.5, 1.0):
            mip = texel_gather_mip_forward(photo, pyr, v, footprint)
            assert torch.equal(bits(texel_gather(photo, v, filter="mip", footprint=footprint).detach()), bits(mip))
            assert torch.equal(bits(v.gather(photo, filter="mip", footprint=footprint).detach()), bits(mip))
    w = view.weight()
    seen = w > 0

    def compose(c):
        return torch.where(seen[..., None], w[..., None] * c / torch.where(seen, w, torch.ones_like(w))[..., None], torch.zeros(16, 16, 4, device="cuda"))
    cams = [(TP.camera("standard"), photo)]
    assert torch.equal(bits(scene.texel_project(cams, material, texels=texels).color.detach()), bits(compose(plain)))
    assert torch.equal(bits(scene.texel_project(cams, material, texels=texels, filter="mip").color.detach()), bits(compose(texel_gather_mip_forward(photo, pyr, view, 1.0))))
    for footprint, max_aniso in ((1.0, 8), (0.5, 8), (1.0, 2)):
        aniso = texel_gather_aniso_forward(photo, pyr, view, view.footprint_data, footprint, max_aniso)
        assert not torch.equal(aniso, plain)
        assert torch.equal(bits(view.gather(photo, filter="aniso", footprint=footprint, max_aniso=max_aniso).detach()), bits(aniso))
        got = scene.texel_project(cams, material, texels=texels, filter="aniso", footprint=footprint, max_aniso=max_aniso)
        assert torch.equal(bits(got.color.detach()), bits(compose(aniso))) and torch.equal(got.weight, w)
    got.color.sum().backward()
    assert float((photo.grad != 0).float().mean()) > float((torch.autograd.grad(scene.texel_project(cams, material, texels=texels).color.sum(), photo)[0] != 0).float().mean())
    scene.check()


def test_the_example_runs_with_the_aniso_filter():
    spec = importlib.util.spec_from_file_location("optimize_texture_aniso", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "optimize_texture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    losses = ex.run(iters=2, res=32, spp=4, tex=32, init_from_target=True, project_filter="aniso", verbose=False)
    print(f"[texel aniso example] first-iteration loss from the anisotropically filtered target {losses[0]:.5f} (reported, not asserted)")
    assert len(losses) == 2 and np.isfinite(losses).all()


# ------------------------------------------------------------------------------------------- errors
def test_wrong_arguments_raise():
    L = N.lib()
    rng = np.random.default_rng(2)
    view = dev(synthetic(rng, 256, (24, 16)).reshape(16, 16, 8))
    fp = dev(synthetic_footprint(rng, 256).reshape(16, 16, 4))
    image = torch.rand(16, 24, 4, device="cuda")
    pyr = image_pyramid_forward(image)
    g = torch.rand(16, 16, 4, device="cuda")
    cam = TP.camera("standard")
    pts = TP.case_points("cbox_16x16_standard")
    with pytest.raises(ValueError):
        texel_gather(image, view, filter="aniso")                                  # a bare view buffer carries no footprint buffer
    with pytest.raises(ValueError):
        texel_gather(image, TexelView(view, (24, 16)), filter="aniso")
    with pytest.raises(ValueError):
        TexelView(view, (24, 16)).gather(image, filter="aniso")
    tv = TexelView(view, (24, 16), fp)
    for max_aniso in (0, 17, -1, 2.5):
        with pytest.raises(ValueError):
            texel_gather(image, tv, filter="aniso", max_aniso=max_aniso)
        with pytest.raises(ValueError):
            texel_gather_aniso_forward(image, pyr, view, fp, 1.0, max_aniso)
        with pytest.raises(ValueError):
            texel_gather_aniso_backward(g, view, fp, (24, 16), 1.0, max_aniso)
    for footprint in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            texel_gather(image, tv, filter="aniso", footprint=footprint)
        with pytest.raises(ValueError):
            texel_gather_aniso_forward(image, pyr, view, fp, footprint)
        with pytest.raises(ValueError):
            texel_gather_aniso_backward(g, view, fp, (24, 16), footprint)
    for bad in (fp[:8].contiguous(), fp[..., :3].contiguous(), fp.cpu(), fp.double()):          # mismatched sizes
        with pytest.raises(ValueError):
            texel_gather_aniso_forward(image, pyr, view, bad)
        with pytest.raises(ValueError):
            texel_gather(image, TexelView(view, (24, 16), bad), filter="aniso")
    with pytest.raises(ValueError):
        texel_gather_aniso_forward(image, pyr[:-1].contiguous(), view, fp)
    with pytest.raises(ValueError):
        texel_gather_aniso_forward(image, pyr, view, fp, out=torch.zeros(16, 16, 3, device="cuda"))
    with pytest.raises(ValueError):
        texel_gather_aniso_backward(torch.rand(8, 8, 4, device="cuda"), view, fp, (24, 16))
    with pytest.raises(ValueError):
        texel_gather_aniso_backward(g, view, fp, (24, 16), d_pyramid=torch.zeros(3, 4, device="cuda"))
    with pytest.raises(ValueError):
        tv.gather(torch.rand(24, 16, 4, device="cuda"), filter="aniso")           # an image of another size than the view's
    for bad in (pts[..., :8].contiguous(), pts.cpu(), pts.double()):
        with pytest.raises(ValueError):
            texel_footprint_forward(bad, (24, 16), cam)
    with pytest.raises(ValueError):
        texel_footprint_forward(pts, (0, 16), cam)
    with pytest.raises(ValueError):
        texel_footprint_forward(pts, (24, 16), cam, out=torch.zeros(16, 16, 8, device="cuda"))
    # the C entry points themselves
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    from zdr_amd.render import _camera_pod

    def fparams(**kw):
        p = N.TexelFootprintParams()
        p.struct_size = C.sizeof(N.TexelFootprintParams)
        p.tex_h, p.tex_w, p.width, p.height = 16, 16, 24, 16
        p.camera = _camera_pod(cam)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    out = torch.zeros(16, 16, 4, device="cuda")
    foot = lambda p, t=pts.data_ptr(), o=out.data_ptr(): L.zdr_texel_footprint(p if p is None else C.byref(p), t, o, stream)   # noqa: E731
    assert foot(fparams()) == 0
    wide = fparams()
    wide.camera.fov = 4.0
    for bad in (None, fparams(struct_size=8), fparams(tex_h=0), fparams(tex_w=-2), fparams(width=0), fparams(height=-1), wide):
        assert foot(bad) == E_INVALID
    assert foot(fparams(tex_h=8193, tex_w=8192)) == E_UNSUPPORTED and foot(fparams(width=16385, height=16384)) == E_UNSUPPORTED
    assert foot(fparams(), t=None) == E_INVALID and foot(fparams(), o=None) == E_INVALID and foot(fparams(), t=pts.data_ptr() + 4) == E_INVALID
    assert foot(fparams(), o=pts.data_ptr()) == E_INVALID and foot(fparams(), o=pts.data_ptr() + 64) == E_INVALID          # out overlaps the input

    def gparams(**kw):
        p = N.TexelGatherAnisoParams()
        p.struct_size = C.sizeof(N.TexelGatherAnisoParams)
        p.tex_h, p.tex_w, p.width, p.height, p.levels, p.footprint, p.max_aniso = 16, 16, 24, 16, 0, 1.0, 8
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    color, d_image, d_pyr = torch.zeros(16, 16, 4, device="cuda"), torch.zeros(16, 24, 4, device="cuda"), torch.zeros_like(pyr)
    fwd = lambda p, v=view.data_ptr(), f=fp.data_ptr(), i=image.data_ptr(), q=pyr.data_ptr(), c=color.data_ptr(): L.zdr_texel_gather_aniso(   # noqa: E731
        p if p is None else C.byref(p), v, f, i, q, c, stream)
    bwd = lambda p, v=view.data_ptr(), f=fp.data_ptr(), i=g.data_ptr(), q=d_pyr.data_ptr(), c=d_image.data_ptr(): L.zdr_texel_gather_aniso_backward(   # noqa: E731
        p if p is None else C.byref(p), v, f, i, c, q, stream)
    assert fwd(gparams()) == 0 and bwd(gparams()) == 0 and fwd(gparams(max_aniso=1)) == 0 and fwd(gparams(max_aniso=16)) == 0
    for call in (fwd, bwd):
        for bad in (None, gparams(struct_size=28), gparams(tex_h=0), gparams(tex_w=-2), gparams(width=0), gparams(height=-1), gparams(levels=-1), gparams(footprint=0.0),
                    gparams(footprint=-1.0), gparams(footprint=float("nan")), gparams(footprint=float("inf")), gparams(max_aniso=0), gparams(max_aniso=17),
                    gparams(max_aniso=-3)):
            assert call(bad) == E_INVALID
        assert call(gparams(tex_h=8193, tex_w=8192)) == E_UNSUPPORTED and call(gparams(width=16385, height=16384)) == E_UNSUPPORTED
        for arg in "vfiqc":
            assert call(gparams(), **{arg: None}) == E_INVALID
        assert call(gparams(), v=view.data_ptr() + 4) == E_INVALID and call(gparams(), f=fp.data_ptr() + 8) == E_INVALID
    for other in (view, fp, image, pyr):                                                                             # the output overlaps an input
        assert fwd(gparams(), c=other.data_ptr()) == E_INVALID and fwd(gparams(), c=other.data_ptr() + 64) == E_INVALID
    for other in (view, fp, g):
        assert bwd(gparams(), c=other.data_ptr()) == E_INVALID and bwd(gparams(), q=other.data_ptr() + 64) == E_INVALID
    assert bwd(gparams(), c=d_pyr.data_ptr()) == E_INVALID and bwd(gparams(), q=d_image.data_ptr() + 64) == E_INVALID   # ... or the other output
    torch.cuda.synchronize()
