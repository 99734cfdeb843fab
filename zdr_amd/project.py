"""Projective texturing, the gather half (include/zdr.h, zdr_texel_gather): a camera's image read into texture space through the view
buffer of ``Scene.texel_view`` — for every texel the camera sees, the bilinear value of the image at the texel's pixel position — and
the adjoint of that map, which scatters a texture-space gradient back onto the image.

    view = scene.texel_view(theta, res=(w, h))               # geometry: one ray per texel, no gradient
    color = texel_gather(photo, view)                        # (H, W, 4), differentiable in photo
    loss = (view.weight()[..., None] * (color - theta)).square().sum()     # a loss in texture space

With the view held fixed the map is linear in the image.  The VIEW BUFFER receives no gradient.  The bilinear gather point-samples: a
texel that covers many pixels (``view.scale`` >> 1) aliases.  ``texel_gather(photo, view, filter="mip")`` is the remedy (README,
"Prefiltered gather"): a mip pyramid of the image (zdr_amd/mip.py) and a trilinear gather whose level comes from ``view.scale``, with
the exact transposes of both, so that the gradient reaches every pixel under a texel's footprint.  That filter is isotropic;
``texel_gather(photo, view, filter="aniso")`` (README, "Anisotropic gather") takes the level from the short axis of each texel's
on-screen ellipse (``texel_footprint_forward``, ``scene.texel_view(..., footprint=True)``) and averages probes along the long one.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N

VIEW_CHANNELS = 8


def _view_data(view):
    data = getattr(view, "data", view)                        # a TexelView or the (H, W, 8) tensor itself
    if not isinstance(data, torch.Tensor) or data.dim() != 3 or data.shape[2] != VIEW_CHANNELS or data.dtype != torch.float32 or data.shape[0] < 1 or data.shape[1] < 1:
        raise ValueError(f"view must be a TexelView or a float32 (H, W, {VIEW_CHANNELS}) tensor")
    if not data.is_cuda:
        raise ValueError(f"the view buffer must be on a GPU, not on {data.device}")
    return data.detach().contiguous()


def _check_image(x, what, device):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 4 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 (height, width, 4) tensor, not {tuple(getattr(x, 'shape', ()))} {getattr(x, 'dtype', type(x))}")
    if x.device != device:
        raise ValueError(f"{what} must be on the view buffer's device {device}, not on {x.device}")


def _out(out, shape, device, what):
    if out is None:
        return None
    if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 {shape} tensor on {device}")
    return out


def _call(fn, view, src, dst, res):
    p = N.TexelGatherParams()
    p.struct_size = C.sizeof(N.TexelGatherParams)
    p.tex_h, p.tex_w, p.width, p.height = int(view.shape[0]), int(view.shape[1]), int(res[0]), int(res[1])
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        N.check(fn(C.byref(p), view.data_ptr(), src.data_ptr(), dst.data_ptr(), stream))
    return dst


def texel_gather_forward(image, view, *, out=None):
    """zdr_texel_gather: ``color[t] = visible[t] * bilinear(image, X[t] - 0.5, Y[t] - 0.5)``, (H, W, 4).  ``image`` is (height, width, 4)
    float32, ``view`` a ``TexelView`` or its (H, W, 8) tensor; ``out`` is allocated when not given.  Only enqueues, on torch's current
    stream."""
    view = _view_data(view)
    _check_image(image, "image", view.device)
    shape = (int(view.shape[0]), int(view.shape[1]), 4)
    out = _out(out, shape, view.device, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=view.device)
    return _call(N.lib().zdr_texel_gather, view, image.detach().contiguous(), out, (image.shape[1], image.shape[0]))


def texel_gather_backward(d_color, view, res, *, d_image=None):
    """zdr_texel_gather_backward: the adjoint of ``texel_gather_forward`` for an image of ``res = (width, height)``, ADDED INTO
    ``d_image`` ((height, width, 4); a zero tensor when not given) with float atomics.  The view receives no gradient."""
    view = _view_data(view)
    w, h = int(res[0]), int(res[1])
    if w < 1 or h < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    _check_image(d_color, "d_color", view.device)
    if tuple(d_color.shape[:2]) != tuple(view.shape[:2]):
        raise ValueError(f"d_color must have the view's size {tuple(view.shape[:2])}, not {tuple(d_color.shape[:2])}")
    d_image = _out(d_image, (h, w, 4), view.device, "d_image")
    if d_image is None:
        d_image = torch.zeros((h, w, 4), dtype=torch.float32, device=view.device)
    return _call(N.lib().zdr_texel_gather_backward, view, d_color.detach().contiguous(), d_image, (w, h))


def _mip_params(view, res, levels, footprint) -> N.TexelGatherMipParams:
    footprint = float(footprint)
    if not (0.0 < footprint < float("inf")):
        raise ValueError(f"footprint must be finite and > 0, not {footprint}")
    p = N.TexelGatherMipParams()
    p.struct_size = C.sizeof(N.TexelGatherMipParams)
    p.tex_h, p.tex_w, p.width, p.height = int(view.shape[0]), int(view.shape[1]), int(res[0]), int(res[1])
    p.levels, p.footprint = levels, footprint
    return p


def texel_gather_mip_forward(image, pyramid, view, footprint=1.0, levels=0, *, out=None):
    """zdr_texel_gather_mip: the trilinear gather of ``image`` and its packed levels >= 1 ``pyramid`` (``image_pyramid_forward`` of the
    same ``levels``), (H, W, 4): the level of a texel is log2(max(view.scale * footprint, 1)), split into a level and a fraction.
    ``out`` is allocated when not given.  Only enqueues, on torch's current stream."""
    from . import mip as M
    view = _view_data(view)
    _check_image(image, "image", view.device)
    levels, res = M._levels_arg(levels), (int(image.shape[1]), int(image.shape[0]))
    M._check_packed(pyramid, "pyramid", res, levels, view.device)
    p = _mip_params(view, res, levels, footprint)
    shape = (int(view.shape[0]), int(view.shape[1]), 4)
    out = _out(out, shape, view.device, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=view.device)
    image = image.detach().contiguous()
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        N.check(N.lib().zdr_texel_gather_mip(C.byref(p), view.data_ptr(), image.data_ptr(), pyramid.data_ptr(), out.data_ptr(), stream))
    return out


def texel_gather_mip_backward(d_color, view, res, footprint=1.0, levels=0, *, d_image=None, d_pyramid=None):
    """zdr_texel_gather_mip_backward: the adjoint of ``texel_gather_mip_forward`` for an image of ``res = (width, height)``, ADDED INTO
    ``d_image`` ((height, width, 4)) and ``d_pyramid`` (the packed levels >= 1), zero tensors when not given, with float atomics.
    Returns ``(d_image, d_pyramid)``; ``image_pyramid_backward(d_pyramid, res, levels, d_image=d_image)`` completes the image's
    gradient.  The view receives no gradient."""
    from . import mip as M
    view = _view_data(view)
    w, h = int(res[0]), int(res[1])
    if w < 1 or h < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    levels = M._levels_arg(levels)
    _check_image(d_color, "d_color", view.device)
    if tuple(d_color.shape[:2]) != tuple(view.shape[:2]):
        raise ValueError(f"d_color must have the view's size {tuple(view.shape[:2])}, not {tuple(d_color.shape[:2])}")
    p = _mip_params(view, (w, h), levels, footprint)
    d_image = _out(d_image, (h, w, 4), view.device, "d_image")
    if d_image is None:
        d_image = torch.zeros((h, w, 4), dtype=torch.float32, device=view.device)
    if d_pyramid is None:
        d_pyramid = torch.zeros((M.pyramid_pixels((w, h), levels), 4), dtype=torch.float32, device=view.device)
    M._check_packed(d_pyramid, "d_pyramid", (w, h), levels, view.device)
    d_color = d_color.detach().contiguous()
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        N.check(N.lib().zdr_texel_gather_mip_backward(C.byref(p), view.data_ptr(), d_color.data_ptr(), d_image.data_ptr(), d_pyramid.data_ptr(), stream))
    return d_image, d_pyramid


class TexelGatherOperator(torch.autograd.Function):
    """The linear map color = K image.  Gradient with respect to the image only; keeps nothing but the detached view buffer."""
    @staticmethod
    def forward(ctx, image, view):
        ctx.save_for_backward(view)
        ctx.res = (int(image.shape[1]), int(image.shape[0]))
        return texel_gather_forward(image, view)

    @staticmethod
    def backward(ctx, grad_output):
        view, = ctx.saved_tensors
        return texel_gather_backward(grad_output, view, ctx.res), None


class TexelGatherMipOperator(torch.autograd.Function):
    """The linear map color = K image with K = (mip gather) o (image, pyramid): four calls, two each way.  Gradient with respect to the
    image only; keeps nothing but the detached view buffer."""
    @staticmethod
    def forward(ctx, image, view, footprint):
        from .mip import image_pyramid_forward
        ctx.save_for_backward(view)
        ctx.res, ctx.footprint = (int(image.shape[1]), int(image.shape[0])), footprint
        return texel_gather_mip_forward(image, image_pyramid_forward(image), view, footprint)

    @staticmethod
    def backward(ctx, grad_output):
        from .mip import image_pyramid_backward
        view, = ctx.saved_tensors
        d_image, d_pyramid = texel_gather_mip_backward(grad_output, view, ctx.res, ctx.footprint)
        return image_pyramid_backward(d_pyramid, ctx.res, d_image=d_image), None, None


FOOTPRINT_CHANNELS = 4
MAX_ANISO = 16


def _footprint_data(data, view):
    if not isinstance(data, torch.Tensor) or tuple(data.shape) != (int(view.shape[0]), int(view.shape[1]), FOOTPRINT_CHANNELS) or data.dtype != torch.float32:
        raise ValueError(f"footprint_data must be a float32 {(int(view.shape[0]), int(view.shape[1]), FOOTPRINT_CHANNELS)} tensor, the footprint buffer of the view's texels")
    if data.device != view.device:
        raise ValueError(f"the footprint buffer must be on the view buffer's device {view.device}, not on {data.device}")
    return data.detach().contiguous()


def texel_footprint_forward(texel_data, res, camera, *, out=None, tangents=None):
    """zdr_texel_footprint: the (H, W, 4) footprint buffer — the major axis of each texel's on-screen ellipse as a vector in pixels
    (floats 0, 1), the lengths of the minor and of the major axis (floats 2, 3) — of ``camera`` with an image of ``res`` = (width, height),
    for the surface points of ``texel_data``, an (H, W, 16) tensor in the layout of ``Scene.texel_aovs_forward`` of which the normal,
    the texel size, the position and ``reach`` are read.  Four zeros where the texel is not shaded or lies behind the camera.  ``out``
    is allocated when not given.  Without ``tangents`` a texel is a square patch of side ``texel_size`` (zdr_texel_footprint); with
    ``tangents``, the (H, W, 8) buffer of ``Scene.texel_tangents_forward`` for the same texels, it is the parallelogram they span
    (zdr_texel_footprint_tangents), and a texel whose tangent row is zero gets four zeros.  No scene, no workspace; only enqueues, on
    torch's current stream."""
    from .render import _camera_pod
    if not isinstance(texel_data, torch.Tensor) or texel_data.dim() != 3 or texel_data.shape[2] != N.AOV_CHANNELS or texel_data.dtype != torch.float32 \
            or texel_data.shape[0] < 1 or texel_data.shape[1] < 1:
        raise ValueError(f"texel_data must be a float32 (H, W, {N.AOV_CHANNELS}) tensor")
    if not texel_data.is_cuda:
        raise ValueError(f"texel_data must be on a GPU, not on {texel_data.device}")
    width, height = int(res[0]), int(res[1])
    if width < 1 or height < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    texel_data = texel_data.detach().contiguous()
    if tangents is not None:
        want = (int(texel_data.shape[0]), int(texel_data.shape[1]), 8)
        if not isinstance(tangents, torch.Tensor) or tuple(tangents.shape) != want or tangents.dtype != torch.float32:
            raise ValueError(f"tangents must be a float32 {want} tensor, the tangent buffer of texel_data's texels")
        if tangents.device != texel_data.device:
            raise ValueError(f"tangents must be on texel_data's device {texel_data.device}, not on {tangents.device}")
        tangents = tangents.detach().contiguous()
    shape = (int(texel_data.shape[0]), int(texel_data.shape[1]), FOOTPRINT_CHANNELS)
    out = _out(out, shape, texel_data.device, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=texel_data.device)
    p = N.TexelFootprintParams()
    p.struct_size = C.sizeof(N.TexelFootprintParams)
    p.tex_h, p.tex_w, p.width, p.height = shape[0], shape[1], width, height
    p.camera = _camera_pod(camera)
    with torch.cuda.device(texel_data.device):
        stream = C.c_void_p(torch.cuda.current_stream(texel_data.device).cuda_stream)
        if tangents is None:
            N.check(N.lib().zdr_texel_footprint(C.byref(p), texel_data.data_ptr(), out.data_ptr(), stream))
        else:
            N.check(N.lib().zdr_texel_footprint_tangents(C.byref(p), texel_data.data_ptr(), tangents.data_ptr(), out.data_ptr(), stream))
    return out


def _aniso_params(view, res, levels, footprint, max_aniso) -> N.TexelGatherAnisoParams:
    footprint = float(footprint)
    if not (0.0 < footprint < float("inf")):
        raise ValueError(f"footprint must be finite and > 0, not {footprint}")
    if isinstance(max_aniso, bool) or int(max_aniso) != max_aniso or not (1 <= int(max_aniso) <= MAX_ANISO):
        raise ValueError(f"max_aniso must be an integer in 1 .. {MAX_ANISO}, not {max_aniso!r}")
    p = N.TexelGatherAnisoParams()
    p.struct_size = C.sizeof(N.TexelGatherAnisoParams)
    p.tex_h, p.tex_w, p.width, p.height = int(view.shape[0]), int(view.shape[1]), int(res[0]), int(res[1])
    p.levels, p.footprint, p.max_aniso = levels, footprint, int(max_aniso)
    return p


def texel_gather_aniso_forward(image, pyramid, view, footprint_data, footprint=1.0, max_aniso=8, levels=0, *, out=None):
    """zdr_texel_gather_aniso: the anisotropic gather of ``image`` and its packed levels >= 1 ``pyramid`` (``image_pyramid_forward`` of
    the same ``levels``), (H, W, 4): up to ``max_aniso`` trilinear probes along the major axis of each texel's ellipse in
    ``footprint_data`` (``texel_footprint_forward``), at the level of the minor axis.  ``out`` is allocated when not given.  Only
    enqueues, on torch's current stream."""
    from . import mip as M
    view = _view_data(view)
    footprint_data = _footprint_data(footprint_data, view)
    _check_image(image, "image", view.device)
    levels, res = M._levels_arg(levels), (int(image.shape[1]), int(image.shape[0]))
    M._check_packed(pyramid, "pyramid", res, levels, view.device)
    p = _aniso_params(view, res, levels, footprint, max_aniso)
    shape = (int(view.shape[0]), int(view.shape[1]), 4)
    out = _out(out, shape, view.device, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=view.device)
    image = image.detach().contiguous()
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        N.check(N.lib().zdr_texel_gather_aniso(C.byref(p), view.data_ptr(), footprint_data.data_ptr(), image.data_ptr(), pyramid.data_ptr(), out.data_ptr(), stream))
    return out


def texel_gather_aniso_backward(d_color, view, footprint_data, res, footprint=1.0, max_aniso=8, levels=0, *, d_image=None, d_pyramid=None):
    """zdr_texel_gather_aniso_backward: the adjoint of ``texel_gather_aniso_forward`` for an image of ``res = (width, height)``, ADDED
    INTO ``d_image`` ((height, width, 4)) and ``d_pyramid`` (the packed levels >= 1), zero tensors when not given, with float atomics.
    Returns ``(d_image, d_pyramid)``; ``image_pyramid_backward(d_pyramid, res, levels, d_image=d_image)`` completes the image's
    gradient.  The view and the footprint buffer receive no gradient."""
    from . import mip as M
    view = _view_data(view)
    footprint_data = _footprint_data(footprint_data, view)
    w, h = int(res[0]), int(res[1])
    if w < 1 or h < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    levels = M._levels_arg(levels)
    _check_image(d_color, "d_color", view.device)
    if tuple(d_color.shape[:2]) != tuple(view.shape[:2]):
        raise ValueError(f"d_color must have the view's size {tuple(view.shape[:2])}, not {tuple(d_color.shape[:2])}")
    p = _aniso_params(view, (w, h), levels, footprint, max_aniso)
    d_image = _out(d_image, (h, w, 4), view.device, "d_image")
    if d_image is None:
        d_image = torch.zeros((h, w, 4), dtype=torch.float32, device=view.device)
    if d_pyramid is None:
        d_pyramid = torch.zeros((M.pyramid_pixels((w, h), levels), 4), dtype=torch.float32, device=view.device)
    M._check_packed(d_pyramid, "d_pyramid", (w, h), levels, view.device)
    d_color = d_color.detach().contiguous()
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        N.check(N.lib().zdr_texel_gather_aniso_backward(C.byref(p), view.data_ptr(), footprint_data.data_ptr(), d_color.data_ptr(), d_image.data_ptr(),
                                                        d_pyramid.data_ptr(), stream))
    return d_image, d_pyramid


class TexelGatherAnisoOperator(torch.autograd.Function):
    """The linear map color = K image with K = (anisotropic gather) o (image, pyramid): four calls, two each way.  Gradient with respect
    to the image only; keeps nothing but the detached view and footprint buffers."""
    @staticmethod
    def forward(ctx, image, view, footprint_data, footprint, max_aniso):
        from .mip import image_pyramid_forward
        ctx.save_for_backward(view, footprint_data)
        ctx.res, ctx.footprint, ctx.max_aniso = (int(image.shape[1]), int(image.shape[0])), footprint, max_aniso
        return texel_gather_aniso_forward(image, image_pyramid_forward(image), view, footprint_data, footprint, max_aniso)

    @staticmethod
    def backward(ctx, grad_output):
        from .mip import image_pyramid_backward
        view, footprint_data = ctx.saved_tensors
        d_image, d_pyramid = texel_gather_aniso_backward(grad_output, view, footprint_data, ctx.res, ctx.footprint, ctx.max_aniso)
        return image_pyramid_backward(d_pyramid, ctx.res, d_image=d_image), None, None, None, None


FILTERS = ("bilinear", "mip", "aniso")
DVIEW_FILTERS = {"bilinear": 0, "mip": 1}


def texel_gather_dview(image, view, d_color, *, filter="bilinear", pyramid=None, footprint=1.0, levels=0, out=None):
    """zdr_texel_gather_dview: the cotangent of the view buffer, (H, W, 8), from the cotangent ``d_color`` (H, W, 4) of
    ``texel_gather_forward(image, view)`` (``filter="bilinear"``) or of ``texel_gather_mip_forward(image, pyramid, view, footprint,
    levels)`` (``filter="mip"``; ``pyramid`` is built here when not given).  Floats 2, 3 (d_X, d_Y) and, for "mip", 6 (d_scale) carry
    values, the rest are 0; eight zeros where the texel is not visible: visibility is held fixed.  ``filter="aniso"`` raises
    ``ValueError``.  Every row of ``out`` is overwritten; it is allocated when not given.  No atomic, the same bits from run to run.
    Only enqueues, on torch's current stream."""
    from . import mip as M
    if filter not in DVIEW_FILTERS:
        raise ValueError(f'filter must be "bilinear" or "mip", not {filter!r}: the anisotropic gather has no derivative in the view buffer')
    view = _view_data(view)
    _check_image(image, "image", view.device)
    _check_image(d_color, "d_color", view.device)
    if tuple(d_color.shape[:2]) != tuple(view.shape[:2]):
        raise ValueError(f"d_color must have the view's size {tuple(view.shape[:2])}, not {tuple(d_color.shape[:2])}")
    res = (int(image.shape[1]), int(image.shape[0]))
    image, d_color = image.detach().contiguous(), d_color.detach().contiguous()
    p = N.TexelGatherDviewParams()
    p.struct_size = C.sizeof(N.TexelGatherDviewParams)
    p.tex_h, p.tex_w, p.width, p.height = int(view.shape[0]), int(view.shape[1]), res[0], res[1]
    p.filter, p.levels, p.footprint = DVIEW_FILTERS[filter], 0, 1.0
    pyramid_ptr = None
    if filter == "mip":
        m = _mip_params(view, res, M._levels_arg(levels), footprint)     # (raises on a bad footprint)
        p.levels, p.footprint = m.levels, m.footprint
        if pyramid is None:
            pyramid = M.image_pyramid_forward(image, p.levels)
        M._check_packed(pyramid, "pyramid", res, p.levels, view.device)
        pyramid_ptr = pyramid.data_ptr()
    shape = (int(view.shape[0]), int(view.shape[1]), VIEW_CHANNELS)
    out = _out(out, shape, view.device, "out")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=view.device)
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        N.check(N.lib().zdr_texel_gather_dview(C.byref(p), view.data_ptr(), image.data_ptr(), pyramid_ptr, d_color.data_ptr(), out.data_ptr(), stream))
    return out


class TexelGatherViewOperator(torch.autograd.Function):
    """color = gather(image, view) over BOTH arguments, for a view buffer that carries gradient (a differentiable camera; README,
    "Camera gradients").  The forward is the gathers' own; the backward is their image adjoint plus ``texel_gather_dview``.  Visibility
    is held fixed."""
    @staticmethod
    def forward(ctx, image, view, filter, footprint):
        from .mip import image_pyramid_forward
        view = view.detach().contiguous()
        pyramid = image_pyramid_forward(image) if filter == "mip" else None
        ctx.filter, ctx.footprint = filter, footprint
        ctx.save_for_backward(image, view, *(() if pyramid is None else (pyramid,)))
        if filter == "mip":
            return texel_gather_mip_forward(image, pyramid, view, footprint)
        return texel_gather_forward(image, view)

    @staticmethod
    def backward(ctx, grad_output):
        from .mip import image_pyramid_backward
        image, view = ctx.saved_tensors[:2]
        res = (int(image.shape[1]), int(image.shape[0]))
        d_image = d_view = None
        if ctx.needs_input_grad[0]:
            if ctx.filter == "mip":
                d_image, d_pyramid = texel_gather_mip_backward(grad_output, view, res, ctx.footprint)
                d_image = image_pyramid_backward(d_pyramid, res, d_image=d_image)
            else:
                d_image = texel_gather_backward(grad_output, view, res)
        if ctx.needs_input_grad[1]:
            pyramid = ctx.saved_tensors[2] if ctx.filter == "mip" else None
            d_view = texel_gather_dview(image, view, grad_output, filter=ctx.filter, pyramid=pyramid, footprint=ctx.footprint)
        return d_image, d_view, None, None


def texel_gather(image, view, *, filter="bilinear", footprint=1.0, max_aniso=8, plan=None):
    """The image gathered into texture space: (H, W, 4), 0 on the texels the camera does not see.  Differentiable in ``image`` only.

    ``filter="bilinear"`` (the default): four taps of the image at the texel's pixel position; ``image.grad`` is the scatter of the
    texture-space gradient onto the four pixels each visible texel reads, exactly 0 on pixels that no visible texel taps.  It
    point-samples: where ``view.scale`` >> 1 it aliases.
    ``filter="mip"``: the prefiltered gather (README, "Prefiltered gather").  A mip pyramid of the image is built and every texel reads
    the two levels around log2(max(view.scale * footprint, 1)), blended by the fraction; where that is 0 (``scale * footprint <= 1``)
    the result is the bilinear one bit for bit.  ``footprint`` (finite, > 0) scales the footprint: 0.5 sharpens by one level.
    ``image.grad`` reaches every pixel under a texel's footprint, through the exact transposes of the gather and of the pyramid.  The
    filter is isotropic: grazing texels are over-blurred across their short axis.
    ``filter="aniso"``: the anisotropic gather (README, "Anisotropic gather").  ``view`` must be a ``TexelView`` made with
    ``footprint=True``: the level comes from the MINOR axis of each texel's on-screen ellipse, and up to ``max_aniso`` (1 .. 16)
    trilinear probes are spread along the major axis and averaged.  ``footprint`` scales both axes.  Where the major axis times
    ``footprint`` is at most 1 the result is the bilinear one bit for bit.  ``image.grad`` as for "mip".
    ``plan``: None (the default) scatters ``image.grad`` with float atomics, whose order of addition varies from run to run.  True, or
    a ``GatherPlan`` made for this view, image size and filter (``view.gather_plan``; any other raises ``ValueError``), leaves the
    forward as it is, bit for bit, and computes ``image.grad`` through the plan (README, "Gather plan"; zdr_amd/plan.py): no atomic,
    the same bits from run to run.  True builds the plan on first use — one synchronisation — and keeps it on the ``TexelView``.
    A view whose ``data`` carries gradient from a camera tensor (``scene.texel_view(..., camera=tensor)``; README, "Camera
    gradients") also receives gradient, with visibility held fixed: "bilinear" and "mip" only, and without ``plan`` — either
    raises ``ValueError``.  A leaf tensor passed as the view receives none, as before; ``texel_gather_dview`` computes its cotangent."""
    if filter not in FILTERS:
        raise ValueError(f"filter must be one of {FILTERS}, not {filter!r}")
    footprint_data = getattr(view, "footprint_data", None)
    view_object = view
    live = view if isinstance(view, torch.Tensor) else getattr(view, "data", None)     # (a tensor's own .data is detached: it would hide the gradient)
    view = _view_data(view)
    _check_image(image, "image", view.device)
    # A view that a differentiable camera made — its data is the result of an autograd node — gets gradient.  A leaf tensor that merely
    # has requires_grad set stays on the path it always took and receives none: texel_gather_dview serves it directly.
    if isinstance(live, torch.Tensor) and live.requires_grad and live.grad_fn is not None and torch.is_grad_enabled():
        if plan is not None:
            raise ValueError("a gather plan is tied to a fixed view: plan= cannot be used with a view that carries gradient")
        if filter == "aniso":
            raise ValueError('filter="aniso" has no derivative in the view buffer: use "mip" or "bilinear" with a differentiable camera')
        if filter == "mip":
            _mip_params(view, (int(image.shape[1]), int(image.shape[0])), 0, footprint)     # (raises on a bad footprint)
        return TexelGatherViewOperator.apply(image, live, filter, float(footprint))
    if plan is not None:
        from . import plan as GP
        if filter == "aniso":
            if footprint_data is None:
                raise ValueError('filter="aniso" needs a view that carries a footprint buffer: scene.texel_view(..., footprint=True)')
            footprint_data = _footprint_data(footprint_data, view)
        key = GP.plan_key((int(image.shape[1]), int(image.shape[0])), filter, footprint, max_aniso, 0)
        GP._params(view, key)                                        # (raises on a bad footprint or max_aniso)
        plan = GP.resolve_plan(plan, view_object, view, key)
        return GP.TexelGatherPlanOperator.apply(image, plan, view, footprint_data if filter == "aniso" else None)
    if filter == "aniso":
        if footprint_data is None:
            raise ValueError('filter="aniso" needs a view that carries a footprint buffer: scene.texel_view(..., footprint=True)')
        footprint_data = _footprint_data(footprint_data, view)
        _aniso_params(view, (int(image.shape[1]), int(image.shape[0])), 0, footprint, max_aniso)     # (raises on a bad footprint or max_aniso)
        return TexelGatherAnisoOperator.apply(image, view, footprint_data, float(footprint), int(max_aniso))
    if filter == "mip":
        _mip_params(view, (int(image.shape[1]), int(image.shape[0])), 0, footprint)     # (raises on a bad footprint)
        return TexelGatherMipOperator.apply(image, view, float(footprint))
    return TexelGatherOperator.apply(image, view)
