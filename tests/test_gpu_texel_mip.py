"""-m gpu: the prefiltered gather (zdr_amd/mip.py, texel_gather(..., filter="mip"); include/zdr.h, zdr_image_pyramid,
zdr_image_pyramid_backward, zdr_texel_gather_mip, zdr_texel_gather_mip_backward) against the reference of tests/texel_mip_ref.py.

The pyramid and its adjoint have a defined order, no contraction and no atomic: they must equal the float32 reference bit for bit, at
sizes on both sides of the fused tail's 32 x 32 and through the paired level launches.  The gather's exact families are compared bit
for bit with the bilinear gather of the level they name; with fractional levels it and the full adjoint are held against the float64
reference under the project's rule (``texel_project_cases.linear_bar``: 4 x the float32 reference's own error against float64, floor
4 float32 ulps of the largest value — the factor covers the atomics' addition order and, forward, log2f's last bit; about 4e-7 on
unit-range images).  Every figure is printed before it is asserted."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import test_gpu_texel_project as TP
import texel_cases as TC
import texel_mip_ref as MR
import texel_project_cases as PC
from test_texel_mip_ref_host import synthetic
from zdr_amd import (ImagePyramid, Scene, image_pyramid, image_pyramid_backward, image_pyramid_forward, pyramid_layout, texel_gather,
                     texel_gather_forward, texel_gather_mip_backward, texel_gather_mip_forward)
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -3            # ZDR_E_* of include/zdr.h
SIZES = [(1, 1), (2, 1), (1, 9), (7, 5), (24, 16), (33, 17)]          # (width, height)
# 32 x 20 is the fused tail alone and 33 x 20 one level launch before it (the hand-over, in one axis only); 67 x 35 takes a launch of two
# levels to reach the tail, 131 x 70 one of two and one of one
PYRAMID_SIZES = SIZES + [(32, 20), (33, 20), (67, 35), (131, 70)]
bits = TP.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def levels_of(image, levels=0):
    """the GPU's own levels of an image, as a list of (h, w, 4) tensors"""
    return ImagePyramid(image, image_pyramid_forward(image, levels), levels).levels


# ------------------------------------------------------------------------------------------- the pyramid
@pytest.mark.parametrize("res", PYRAMID_SIZES)
def test_pyramid_and_adjoint_equal_the_float32_reference_bit_for_bit(res):
    rng = np.random.default_rng(11)
    w, h = res
    image = rng.normal(size=(h, w, 4)).astype(np.float32)
    base = rng.normal(size=(h, w, 4)).astype(np.float32)
    for levels in (0, 1, 2, 3):
        lay = pyramid_layout(res, levels)
        assert [(a, b) for a, b, _ in lay] == [(a, b) for a, b, _ in MR.layout(res, levels)]
        want = MR.pack(MR.pyramid_ref(image, levels, np.float32))
        got = image_pyramid_forward(dev(image), levels)
        assert got.shape == want.shape
        if len(lay) > 1:
            assert torch.equal(bits(got), bits(dev(want))), (res, levels)
            again = image_pyramid_forward(dev(image), levels, out=torch.full_like(got, float("nan")))       # a dirty output
            assert torch.equal(bits(again), bits(got))
        G = rng.normal(size=want.shape).astype(np.float32)
        up = MR.pyramid_adjoint_ref(G, res, levels, np.float32)
        d = image_pyramid_backward(dev(G), res, levels)
        assert torch.equal(bits(d), bits(dev(np.zeros_like(up) + up))), (res, levels)
        into = image_pyramid_backward(dev(G), res, levels, d_image=dev(base))                                   # it adds into what d_image holds
        assert torch.equal(bits(into), bits(dev(base + up))), (res, levels)
        if len(lay) > 1:
            assert float(d.abs().sum()) > 0


def test_a_constant_image_has_constant_levels_of_the_same_bits():
    image = torch.full((17, 33, 4), 0.3, device="cuda")
    for v in levels_of(image):
        assert torch.equal(bits(v), bits(torch.full_like(v, 0.3)))


# ------------------------------------------------------------------------------------------- the gather on synthetic views
@pytest.mark.parametrize("res", SIZES)
def test_the_four_properties_bit_for_bit(res):
    rng = np.random.default_rng(12)
    w, h = res
    image = dev(rng.normal(size=(h, w, 4)))
    pyr = image_pyramid_forward(image)
    levels = levels_of(image)
    L = len(levels) - 1
    # 1. wherever s <= 1 the result is the bilinear gather's
    view = synthetic(rng, 400, res, scale=(0.01, 1.0))
    view[:3, 0, 6] = (0.0, 1.0, np.nan); view[:3, 0, 0] = 1                    # a scale of 0 or NaN: level 0, a finite result
    assert torch.isfinite(texel_gather_mip_forward(image, pyr, dev(view))).all()
    assert torch.equal(bits(texel_gather_mip_forward(image, pyr, dev(view))), bits(texel_gather_forward(image, dev(view))))
    # 2. scale = 2^k, footprint 1: the bilinear gather of level k with X, Y scaled by 2^-k;  infinity and anything >= 2^L: level L
    for lvl, scale in [(k, 2.0 ** k) for k in range(L + 1)] + [(L, np.inf), (L, 2.0 ** L * 1.7)]:
        view = synthetic(rng, 400, res)
        view[:, 0, 6] = scale
        scaled = view.copy()
        scaled[:, 0, 2:4] = view[:, 0, 2:4] * np.float32(2.0 ** -lvl)
        got = texel_gather_mip_forward(image, pyr, dev(view))
        assert torch.isfinite(got).all()
        assert torch.equal(bits(got), bits(texel_gather_forward(levels[lvl].contiguous(), dev(scaled)))), (res, lvl, scale)
    # 3. a constant image comes out as visible x that constant, for any scale
    view = synthetic(rng, 400, res)
    view[:, 0, 0] *= rng.uniform(0.2, 1.0, 400).astype(np.float32)
    const = torch.full((h, w, 4), 0.3, device="cuda")
    got = texel_gather_mip_forward(const, image_pyramid_forward(const), dev(view))
    assert torch.equal(bits(got), bits((dev(view)[..., 0:1] * torch.tensor(0.3, device="cuda")).expand(400, 1, 4)))
    # 4. what lies behind an invisible texel never reaches the result: X, Y, scale, the image and the pyramid
    view = synthetic(rng, 400, res)
    clean = texel_gather_mip_forward(image, pyr, dev(view))
    off = view[:, 0, 0] == 0
    view[off, 0, 2] = np.nan; view[off, 0, 3] = 1e30; view[off, 0, 6] = np.nan
    got = texel_gather_mip_forward(image, pyr, dev(view), out=torch.full((400, 1, 4), float("nan"), device="cuda"))
    assert torch.equal(bits(got), bits(clean)) and (got[torch.from_numpy(off).cuda()] == 0).all() and not torch.isnan(got).any()
    view[:, 0, 0] = 0
    assert (texel_gather_mip_forward(torch.full_like(image, float("nan")), torch.full_like(pyr, float("nan")), dev(view)) == 0).all()


def test_a_checkerboard_gathers_to_exactly_one_half():
    rng = np.random.default_rng(8)
    ys, xs = np.mgrid[0:64, 0:64]
    board = dev(np.repeat(((xs + ys) % 2).astype(np.float32)[..., None], 4, -1))
    view = synthetic(rng, 400, (64, 64))
    view[:, 0, 6] = rng.uniform(2.0, 40.0, 400)
    on = torch.from_numpy(view[:, 0, 0] == 1).cuda()
    got = texel_gather_mip_forward(board, image_pyramid_forward(board), dev(view))
    assert (got[on] == 0.5).all() and (got[~on] == 0).all()
    plain = texel_gather_forward(board, dev(view))[on]
    print(f"[texel mip checkerboard] bilinear standard deviation {float(plain.std()):.3f}")
    assert float(plain.std()) > 0.1


# ------------------------------------------------------------------------------------------- parity with fractional levels
@pytest.mark.parametrize("res", [(24, 16), (33, 17)])
@pytest.mark.parametrize("footprint", [1.0, 3.0, 0.5])
@pytest.mark.parametrize("name", ["cbox_64x64_standard", "cbox_64x64_inside_1x1"])
def test_gather_and_full_adjoint_parity_on_the_kernels_own_view_buffer(name, footprint, res):
    """The cotangent is drawn from [0, 1), like the image, not from a normal distribution.  On ``cbox_64x64_inside_1x1`` the 175 visible
    texels all land in [0, 1) x [0, 1), so 490 of the 700 atomics add into pixel (0, 0), and the bar — the project's rule — is 4 x the
    error of ONE order of that sum, the float32 reference's.  With a signed cotangent the partial sums are a random walk that cancels,
    and the error of one order says little about another's: adding the same 700 float32 products in 2,000 random orders on the host
    (no kernel involved) exceeded 4 x the texel order's error in 8.2 % of the orders at 24 x 16 and in 3.2 % at 33 x 17, and on an
    MI355X the kernel came out at 2.8e-6 to 3.5e-6 in twelve runs and at 1.25e-5, above the bar of 1.09e-5, in two others.  With a
    cotangent of one sign every partial sum grows towards the result and every order rounds at the same magnitudes: none of 2,000 random
    orders exceeded the bar (on the float64 reference's view of the case: largest 9.2e-5 against bars of 2.3e-4 and 1.4e-4, at a largest
    |d_image| of 76 and 82; on the kernel's own view the bars are 1.7e-4 and the kernel came out at 1.4e-5 to 4.3e-5).  The views, the
    footprints, the image sizes and the rule of the bar are unchanged; a wrong tap, weight or level is off by 1e-2 either way."""
    view = TP.run_case(name, "bvh")
    v = view.cpu().numpy()
    rng = np.random.default_rng(17)
    image, g = rng.uniform(0, 1, (res[1], res[0], 4)).astype(np.float32), rng.uniform(0, 1, (64, 64, 4)).astype(np.float32)
    l0, f = MR.level_split(v[..., 6][v[..., 0] == 1], footprint, len(MR.layout(res)) - 1, np.float32)
    r64, r32 = MR.gather_mip_ref(image, v, footprint), MR.gather_mip_ref(image, v, footprint, 0, np.float32)
    bar = MR.linear_bar(r32, r64)
    gpu_image = dev(image)
    got = texel_gather_mip_forward(gpu_image, image_pyramid_forward(gpu_image), view, footprint).cpu().numpy()
    err = float(np.abs(got - r64).max())
    print(f"[texel mip parity] {name} {res} footprint {footprint}: visible {int(v[..., 0].sum())}, levels {sorted(set(l0.tolist()))}, fractional {int((f != 0).sum())}; "
          f"kernel vs float64 {err:.3e}; float32 reference {float(np.abs(r32 - r64).max()):.3e}; bar {bar:.3e}")
    assert float(np.abs(got).sum()) > 0 and err <= bar
    a64, a32 = MR.gather_mip_adjoint_ref(g, v, res, footprint), MR.gather_mip_adjoint_ref(g, v, res, footprint, 0, np.float32)
    bar = MR.linear_bar(a32, a64)
    d_image, d_pyramid = texel_gather_mip_backward(dev(g), view, res, footprint)
    d = image_pyramid_backward(d_pyramid, res, d_image=d_image).cpu().numpy()
    err = float(np.abs(d - a64).max())
    print(f"[texel mip adjoint parity] {name} {res} footprint {footprint}: kernel vs float64 transpose {err:.3e}; float32 reference "
          f"{float(np.abs(a32 - a64).max()):.3e}; bar {bar:.3e}; largest |d_image| {np.abs(a64).max():.3e}")
    assert err <= bar


@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("res", [(33, 17), (67, 35)])
def test_gather_and_full_adjoint_parity_through_every_level_on_a_synthetic_view(res, levels):
    """the views above reach level 1 at most; scales drawn log-uniformly from [0.25, 40) reach every level of these images, and with
    ``levels=2`` everything from scale 4 on reads the last level the pyramid has"""
    rng = np.random.default_rng(19)
    v = synthetic(rng, 500, res)
    image, g = rng.uniform(0, 1, (res[1], res[0], 4)).astype(np.float32), rng.normal(size=(500, 1, 4)).astype(np.float32)
    l0, _ = MR.level_split(v[:, 0, 6], 1.0, len(MR.layout(res, levels)) - 1, np.float32)
    assert len(set(l0.tolist())) == (3 if levels else 6)
    r64 = MR.gather_mip_ref(image, v, 1.0, levels)
    bar = MR.linear_bar(MR.gather_mip_ref(image, v, 1.0, levels, np.float32), r64)
    gpu_image = dev(image)
    err = float(np.abs(texel_gather_mip_forward(gpu_image, image_pyramid_forward(gpu_image, levels), dev(v), 1.0, levels).cpu().numpy() - r64).max())
    print(f"[texel mip parity] synthetic {res} levels {levels}: levels read {sorted(set(l0.tolist()))}; kernel vs float64 {err:.3e}; bar {bar:.3e}")
    assert err <= bar
    a64 = MR.gather_mip_adjoint_ref(g, v, res, 1.0, levels)
    bar = MR.linear_bar(MR.gather_mip_adjoint_ref(g, v, res, 1.0, levels, np.float32), a64)
    d_image, d_pyramid = texel_gather_mip_backward(dev(g), dev(v), res, 1.0, levels)
    err = float(np.abs(image_pyramid_backward(d_pyramid, res, levels, d_image=d_image).cpu().numpy() - a64).max())
    print(f"[texel mip adjoint parity] synthetic {res} levels {levels}: kernel vs float64 transpose {err:.3e}; bar {bar:.3e}; largest |d_image| {np.abs(a64).max():.3e}")
    assert err <= bar


# ------------------------------------------------------------------------------------------- autograd
def test_the_gradient_passes_through_the_mip_gather_and_is_zero_where_no_footprint_reaches():
    name = "cbox_64x64_standard"
    res = PC.CASES[name][2]
    view = TP.run_case(name, "bvh")
    view[..., 0] *= (view[..., 2] < 11.0)                         # nothing visible taps the pixels x >= 12 of level 0 ...
    gen = torch.Generator().manual_seed(2)
    # ... nor, with scales in [0.3, 0.95) and footprint 2 (s < 2: level 0 and, where s > 1, level 1), a pixel of level 1 above them: X < 11
    # taps the columns 4 and 5 of level 1 at most, the pixels 8 .. 11 of the image
    view[..., 6] = (0.3 + 0.65 * torch.rand(64, 64, generator=gen)).cuda()
    assert float(((view[..., 6] * 2.0 > 1.0) & (view[..., 0] == 1)).sum()) > 100      # fractional levels are in play
    image = torch.rand(res[1], res[0], 4, generator=gen).cuda().requires_grad_()
    y = torch.randn(64, 64, 4, generator=gen).cuda()
    out = texel_gather(image, view, filter="mip", footprint=2.0)
    assert out.requires_grad
    out.backward(y)
    dx = torch.randn(res[1], res[0], 4, generator=gen).cuda()
    lhs = float((texel_gather_mip_forward(dx, image_pyramid_forward(dx), view, 2.0).double() * y.double()).sum())
    rhs = float((dx.double() * image.grad.double()).sum())
    print(f"[texel mip dot product] <K dx, y> = {lhs:.9e}, <dx, K^T y> = {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))
    assert (image.grad[:, 12:] == 0).all() and float(image.grad[:, :11].abs().sum()) > 0
    vg = view.clone().requires_grad_()
    assert torch.autograd.grad(texel_gather(image, vg, filter="mip").sum(), [image, vg], allow_unused=True)[1] is None      # the view receives none


def test_image_pyramid_is_differentiable_and_its_levels_are_views():
    gen = torch.Generator().manual_seed(3)
    image = torch.rand(17, 33, 4, generator=gen).cuda().requires_grad_()
    pyr = image_pyramid(image)
    assert isinstance(pyr, ImagePyramid) and pyr.levels[0] is image and len(pyr.levels) == 7 and pyr.res == (33, 17)
    assert [tuple(v.shape) for v in pyr.levels[1:3]] == [(9, 17, 4), (5, 9, 4)] and pyr.data.shape == (sum(w * h for w, h, _ in pyramid_layout((33, 17))[1:]), 4)
    assert pyr.levels[2].data_ptr() == pyr.data.data_ptr() + 16 * 9 * 17 and pyr.data.requires_grad
    ys = [torch.randn(v.shape, generator=gen).cuda() for v in pyr.levels[1:]]
    sum((v * y).sum() for v, y in zip(pyr.levels[1:], ys)).backward()
    want = MR.pyramid_adjoint_ref([None] + [y.cpu().numpy() for y in ys], (33, 17), 0, np.float32)
    assert torch.equal(bits(image.grad), bits(dev(np.zeros_like(want) + want)))
    cut = image_pyramid(image.detach(), levels=2)
    assert len(cut.levels) == 3 and torch.equal(bits(cut.levels[2]), bits(pyr.levels[2].detach()))


def test_the_defaults_give_the_bilinear_bits_and_texel_project_composes_the_mip_gather():
    scene = Scene(TC.cbox_arrays(), integrator="direct")
    scene.camera = TP.camera("standard")
    material = torch.rand(16, 16, 4, device="cuda")
    texels = scene.texel_aovs(material)
    gen = torch.Generator().manual_seed(4)
    photo = torch.rand(64, 96, 4, generator=gen).cuda().requires_grad_()
    view = scene.texel_view(material, res=(96, 64), texels=texels)
    assert float(((view.scale > 2) & (view.visible == 1)).sum()) > 20         # texels that cover many pixels: the prefilter matters
    plain = texel_gather_forward(photo, view)
    assert torch.equal(bits(texel_gather(photo, view).detach()), bits(plain)) and torch.equal(bits(view.gather(photo).detach()), bits(plain))
    assert torch.equal(bits(texel_gather(photo, view, filter="bilinear", footprint=7.0).detach()), bits(plain))
    w = view.weight()
    seen = w > 0

    def compose(c):
        return torch.where(seen[..., None], w[..., None] * c / torch.where(seen, w, torch.ones_like(w))[..., None], torch.zeros(16, 16, 4, device="cuda"))
    one = scene.texel_project([(TP.camera("standard"), photo)], material, texels=texels)
    assert torch.equal(bits(one.color.detach()), bits(compose(plain)))
    for footprint in (0.5, 1.0):
        mip = texel_gather_mip_forward(photo, image_pyramid_forward(photo), view, footprint)
        assert not torch.equal(mip, plain)
        assert torch.equal(bits(view.gather(photo, filter="mip", footprint=footprint).detach()), bits(mip))
        got = scene.texel_project([(TP.camera("standard"), photo)], material, texels=texels, filter="mip", footprint=footprint)
        assert torch.equal(bits(got.color.detach()), bits(compose(mip))) and torch.equal(got.weight, w)
    got.color.sum().backward()
    assert float((photo.grad != 0).float().mean()) > 2 * float((torch.autograd.grad(one.color.sum(), photo)[0] != 0).float().mean())   # the gradient reaches the footprint
    scene.check()


def test_the_example_runs_with_the_mip_filter():
    spec = importlib.util.spec_from_file_location("optimize_texture_mip", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "optimize_texture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    losses = ex.run(iters=2, res=32, spp=4, tex=32, init_from_target=True, project_filter="mip", verbose=False)
    print(f"[texel mip example] first-iteration loss from the prefiltered target {losses[0]:.5f} (reported, not asserted)")
    assert len(losses) == 2 and np.isfinite(losses).all()


# ------------------------------------------------------------------------------------------- errors
def test_wrong_arguments_raise():
    L = N.lib()
    view = dev(synthetic(np.random.default_rng(1), 256, (24, 16)).reshape(16, 16, 8))
    image = torch.rand(16, 24, 4, device="cuda")
    pyr = image_pyramid_forward(image)
    npix = pyr.shape[0]
    for bad in (image[..., :3].contiguous(), image.cpu(), image.double()):
        with pytest.raises(ValueError):
            image_pyramid_forward(bad)
        with pytest.raises(ValueError):
            image_pyramid(bad)
    with pytest.raises(ValueError):
        image_pyramid_forward(image, levels=-1)
    with pytest.raises(ValueError):
        image_pyramid_forward(image, out=torch.zeros(npix + 1, 4, device="cuda"))
    with pytest.raises(ValueError):
        image_pyramid_backward(pyr, (24, 0))
    with pytest.raises(ValueError):
        image_pyramid_backward(pyr, (24, 16), levels=2)                                    # a buffer of another pyramid
    with pytest.raises(ValueError):
        image_pyramid_backward(pyr, (24, 16), d_image=torch.zeros(24, 16, 4, device="cuda"))
    with pytest.raises(ValueError):
        pyramid_layout((0, 4))
    for footprint in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            texel_gather_mip_forward(image, pyr, view, footprint)
        with pytest.raises(ValueError):
            texel_gather_mip_backward(torch.rand(16, 16, 4, device="cuda"), view, (24, 16), footprint)
        with pytest.raises(ValueError):
            texel_gather(image, view, filter="mip", footprint=footprint)
    with pytest.raises(ValueError):
        texel_gather(image, view, filter="trilinear")
    with pytest.raises(ValueError):
        texel_gather_mip_forward(image, pyr[:-1].contiguous(), view)
    with pytest.raises(ValueError):
        texel_gather_mip_forward(image, pyr, view[..., :4].contiguous())
    with pytest.raises(ValueError):
        texel_gather_mip_forward(image, pyr, view, out=torch.zeros(16, 16, 3, device="cuda"))
    with pytest.raises(ValueError):
        texel_gather_mip_backward(torch.rand(8, 8, 4, device="cuda"), view, (24, 16))
    with pytest.raises(ValueError):
        texel_gather_mip_backward(torch.rand(16, 16, 4, device="cuda"), view, (24, 16), d_pyramid=torch.zeros(3, 4, device="cuda"))
    # the C entry points themselves
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pparams(**kw):
        p = N.ImagePyramidParams()
        p.struct_size = C.sizeof(N.ImagePyramidParams)
        p.width, p.height, p.levels = 24, 16, 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    assert L.zdr_image_pyramid_bytes(C.byref(pparams())) == 16 * npix and L.zdr_image_pyramid_bytes(C.byref(pparams(width=1, height=1))) == 16
    assert L.zdr_image_pyramid_bytes(C.byref(pparams(levels=1))) == 16 * 12 * 8
    d_image, d_pyr = torch.zeros(16, 24, 4, device="cuda"), torch.zeros_like(pyr)
    assert L.zdr_image_pyramid(C.byref(pparams()), image.data_ptr(), pyr.data_ptr(), stream) == 0
    assert L.zdr_image_pyramid_backward(C.byref(pparams()), d_pyr.data_ptr(), d_image.data_ptr(), stream) == 0
    for bad in (pparams(struct_size=8), pparams(width=0), pparams(height=-1), pparams(levels=-1)):
        assert L.zdr_image_pyramid_bytes(C.byref(bad)) == 0
        assert L.zdr_image_pyramid(C.byref(bad), image.data_ptr(), pyr.data_ptr(), stream) == E_INVALID
        assert L.zdr_image_pyramid_backward(C.byref(bad), d_pyr.data_ptr(), d_image.data_ptr(), stream) == E_INVALID
    big = pparams(width=16385, height=16384)
    assert L.zdr_image_pyramid_bytes(C.byref(big)) == 0 and L.zdr_image_pyramid(C.byref(big), image.data_ptr(), pyr.data_ptr(), stream) == E_UNSUPPORTED
    assert L.zdr_image_pyramid_backward(C.byref(big), d_pyr.data_ptr(), d_image.data_ptr(), stream) == E_UNSUPPORTED
    for fn, a, b in ((L.zdr_image_pyramid, image, pyr), (L.zdr_image_pyramid_backward, d_pyr, d_image)):
        assert fn(None, a.data_ptr(), b.data_ptr(), stream) == E_INVALID
        assert fn(C.byref(pparams()), None, b.data_ptr(), stream) == E_INVALID and fn(C.byref(pparams()), a.data_ptr(), None, stream) == E_INVALID
        assert fn(C.byref(pparams()), a.data_ptr() + 4, b.data_ptr(), stream) == E_INVALID and fn(C.byref(pparams()), a.data_ptr(), b.data_ptr() + 8, stream) == E_INVALID
        assert fn(C.byref(pparams()), a.data_ptr(), a.data_ptr(), stream) == E_INVALID                               # the pyramid aliases the image
        assert fn(C.byref(pparams()), a.data_ptr(), a.data_ptr() + 64, stream) == E_INVALID

    def gparams(**kw):
        p = N.TexelGatherMipParams()
        p.struct_size = C.sizeof(N.TexelGatherMipParams)
        p.tex_h, p.tex_w, p.width, p.height, p.levels, p.footprint = 16, 16, 24, 16, 0, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    color = torch.zeros(16, 16, 4, device="cuda")
    fwd = lambda p, v=view.data_ptr(), i=image.data_ptr(), q=pyr.data_ptr(), c=color.data_ptr(): L.zdr_texel_gather_mip(p if p is None else C.byref(p), v, i, q, c, stream)   # noqa: E731
    bwd = lambda p, v=view.data_ptr(), g=color.data_ptr(), i=d_image.data_ptr(), q=d_pyr.data_ptr(): L.zdr_texel_gather_mip_backward(p if p is None else C.byref(p), v, g, i, q, stream)   # noqa: E731
    assert fwd(gparams()) == 0 and bwd(gparams()) == 0
    for call in (fwd, bwd):
        for bad in (None, gparams(struct_size=20), gparams(tex_h=0), gparams(tex_w=-2), gparams(width=0), gparams(height=-1), gparams(levels=-1), gparams(footprint=0.0),
                    gparams(footprint=-1.0), gparams(footprint=float("nan")), gparams(footprint=float("inf"))):
            assert call(bad) == E_INVALID
        assert call(gparams(tex_h=8193, tex_w=8192)) == E_UNSUPPORTED and call(gparams(width=16385, height=16384)) == E_UNSUPPORTED
        assert call(gparams(), v=None) == E_INVALID and call(gparams(), v=view.data_ptr() + 4) == E_INVALID
        assert call(gparams(), i=None) == E_INVALID and call(gparams(), i=image.data_ptr() + 8) == E_INVALID
        assert call(gparams(), q=None) == E_INVALID and call(gparams(), q=pyr.data_ptr() + 4) == E_INVALID
    assert fwd(gparams(), c=None) == E_INVALID and fwd(gparams(), c=color.data_ptr() + 4) == E_INVALID
    assert bwd(gparams(), g=None) == E_INVALID and bwd(gparams(), g=color.data_ptr() + 4) == E_INVALID
    for other in (view, image, pyr):                                                                                 # the output overlaps an input
        assert fwd(gparams(), c=other.data_ptr()) == E_INVALID and fwd(gparams(), c=other.data_ptr() + 64) == E_INVALID
    for other in (view, color):
        assert bwd(gparams(), i=other.data_ptr()) == E_INVALID and bwd(gparams(), q=other.data_ptr() + 64) == E_INVALID
    assert bwd(gparams(), i=d_pyr.data_ptr()) == E_INVALID and bwd(gparams(), q=d_image.data_ptr() + 64) == E_INVALID   # ... or the other output
    torch.cuda.synchronize()
