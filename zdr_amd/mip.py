"""The mip pyramid of an image (include/zdr.h, zdr_image_pyramid) and its exact transpose: what the prefiltered gather of
zdr_amd/project.py (``texel_gather(..., filter="mip")``) reads its coarser levels from.

    pyr = image_pyramid(photo)                               # differentiable in photo
    pyr.levels[0] is photo;  pyr.levels[2]                    # (ceil(h / 4), ceil(w / 4), 4), a view of pyr.data

Level l + 1 is the 2 x 2 box filter of level l, ``((a00 + a01) + (a10 + a11)) * 0.25`` per channel, the image continued by its border
pixels; the levels >= 1 sit packed one after another in ``data``.  Both passes are HIP kernels without atomics: the same bits from run
to run.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N


def _levels_arg(levels) -> int:
    levels = 0 if levels is None else int(levels)
    if levels < 0:
        raise ValueError(f"levels must be 0 (down to 1 x 1) or a positive count, not {levels}")
    return levels


def pyramid_layout(res, levels=0):
    """The levels of the pyramid of an image of ``res = (width, height)``: a list of (width, height, offset), level 0 first; ``offset``
    counts pixels (float4) from the start of the packed buffer and is None for level 0, which is the image itself.  ``levels``: stop
    after that many halvings (0: down to 1 x 1)."""
    w, h, levels = int(res[0]), int(res[1]), _levels_arg(levels)
    if w < 1 or h < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    out, off = [(w, h, None)], 0
    while (w > 1 or h > 1) and (levels == 0 or len(out) - 1 < levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h, off))
        off += w * h
    return out


def pyramid_pixels(res, levels=0) -> int:
    """Pixels (float4) of the packed buffer: zdr_image_pyramid_bytes / 16, 1 for an image without a level >= 1."""
    return max(sum(w * h for w, h, _ in pyramid_layout(res, levels)[1:]), 1)


def _params(res, levels) -> N.ImagePyramidParams:
    p = N.ImagePyramidParams()
    p.struct_size = C.sizeof(N.ImagePyramidParams)
    p.width, p.height, p.levels = int(res[0]), int(res[1]), levels
    return p


def _check_image(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[2] != 4 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 (height, width, 4) tensor, not {tuple(getattr(x, 'shape', ()))} {getattr(x, 'dtype', type(x))}")
    if not x.is_cuda:
        raise ValueError(f"{what} must be on a GPU, not on {x.device}")


def _check_packed(x, what, res, levels, device):
    n = pyramid_pixels(res, levels)
    if not isinstance(x, torch.Tensor) or tuple(x.shape) != (n, 4) or x.dtype != torch.float32 or x.device != device or not x.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 ({n}, 4) tensor on {device}: the packed levels >= 1 of a {res[0]} x {res[1]} image")
    return x


def image_pyramid_forward(image, levels=0, *, out=None):
    """zdr_image_pyramid: the packed levels >= 1 of ``image`` ((height, width, 4) float32), a (pixels, 4) tensor (``pyramid_layout`` says
    where each level lies); ``out`` is allocated when not given.  Only enqueues, on torch's current stream."""
    _check_image(image, "image")
    levels, res = _levels_arg(levels), (int(image.shape[1]), int(image.shape[0]))
    if out is None:
        out = torch.empty((pyramid_pixels(res, levels), 4), dtype=torch.float32, device=image.device)
    _check_packed(out, "out", res, levels, image.device)
    image = image.detach().contiguous()
    with torch.cuda.device(image.device):
        stream = C.c_void_p(torch.cuda.current_stream(image.device).cuda_stream)
        N.check(N.lib().zdr_image_pyramid(C.byref(_params(res, levels)), image.data_ptr(), out.data_ptr(), stream))
    return out


def image_pyramid_backward(d_pyramid, res, levels=0, *, d_image=None):
    """zdr_image_pyramid_backward: the transpose of ``image_pyramid_forward`` for an image of ``res = (width, height)``, ADDED INTO
    ``d_image`` ((height, width, 4); a zero tensor when not given).  ``d_pyramid`` — the cotangents of the levels >= 1, packed — is
    used as a workspace: its contents afterwards are unspecified."""
    levels, res = _levels_arg(levels), (int(res[0]), int(res[1]))
    if res[0] < 1 or res[1] < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    if not isinstance(d_pyramid, torch.Tensor) or not d_pyramid.is_cuda:
        raise ValueError("d_pyramid must be a tensor on a GPU")
    _check_packed(d_pyramid, "d_pyramid", res, levels, d_pyramid.device)
    if d_image is None:
        d_image = torch.zeros((res[1], res[0], 4), dtype=torch.float32, device=d_pyramid.device)
    elif tuple(d_image.shape) != (res[1], res[0], 4) or d_image.dtype != torch.float32 or d_image.device != d_pyramid.device or not d_image.is_contiguous():
        raise ValueError(f"d_image must be a contiguous float32 {(res[1], res[0], 4)} tensor on {d_pyramid.device}")
    with torch.cuda.device(d_pyramid.device):
        stream = C.c_void_p(torch.cuda.current_stream(d_pyramid.device).cuda_stream)
        N.check(N.lib().zdr_image_pyramid_backward(C.byref(_params(res, levels)), d_pyramid.data_ptr(), d_image.data_ptr(), stream))
    return d_image


class ImagePyramid:
    """An image and its coarser levels, from ``image_pyramid``: ``levels[l]`` is (h_l, w_l, 4), level 0 the image itself and the others
    views of ``data``, the packed (pixels, 4) buffer of the levels >= 1; ``res`` = (width, height) of level 0."""

    def __init__(self, image, data, levels=0):
        self.image, self.data = image, data
        self.res = (int(image.shape[1]), int(image.shape[0]))
        self.levels = [image] + [data[off:off + w * h].view(h, w, 4) for w, h, off in pyramid_layout(self.res, levels)[1:]]


class ImagePyramidOperator(torch.autograd.Function):
    """The linear map image -> packed levels >= 1.  Keeps nothing."""
    @staticmethod
    def forward(ctx, image, levels):
        ctx.res, ctx.levels = (int(image.shape[1]), int(image.shape[0])), levels
        return image_pyramid_forward(image, levels)

    @staticmethod
    def backward(ctx, grad_output):
        return image_pyramid_backward(grad_output.contiguous().clone(), ctx.res, ctx.levels), None      # (a copy: the call uses it as a workspace)


def image_pyramid(image, levels=0) -> ImagePyramid:
    """The mip pyramid of ``image`` ((height, width, 4) float32 on the GPU), differentiable in ``image``: an ``ImagePyramid``.
    ``levels``: stop after that many halvings (0: down to 1 x 1)."""
    _check_image(image, "image")
    levels = _levels_arg(levels)
    return ImagePyramid(image, ImagePyramidOperator.apply(image, levels), levels)
