"""Feature-guided à-trous denoiser (include/zdr.h, zdr_denoise): an edge-stopping wavelet filter of a rendered image, guided by the
first-hit normal, depth, albedo and instance of ``Scene.render_aovs``, meant to sit between a noisy render and a loss.

    image = scene.render(material, res=(W, H), spp=16, seed=s)
    aovs = scene.render_aovs(material, res=(W, H), spp=16, seed=s)        # the same camera samples: the buffers line up
    clean = denoise(image, aovs)                                            # (H, W, 4), differentiable
    (clean[..., :3] - target).abs().mean().backward()

The filter is linear in the image while the guides are held fixed; its adjoint is a HIP kernel as well, exact and deterministic.
The edge-stopping WEIGHTS are not differentiated: the feature buffers receive no gradient from them.  With ``demodulate`` the image
is divided by the first-hit albedo before the filter and multiplied by it afterwards, in torch, so that texture detail is not
blurred; that albedo does carry gradient back to the materials through ``render_aovs``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N


def _data(aovs):
    return aovs.data if hasattr(aovs, "CHANNELS") else aovs


def _params(shape, levels, sigma_normal, sigma_depth, sigma_albedo) -> N.DenoiseParams:
    p = N.DenoiseParams()
    p.struct_size = C.sizeof(N.DenoiseParams)
    p.height, p.width, p.levels = int(shape[0]), int(shape[1]), int(levels)
    p.sigma_normal, p.sigma_depth, p.sigma_albedo = float(sigma_normal), float(sigma_depth), float(sigma_albedo)
    return p


def workspace_bytes(res, levels) -> int:
    """Bytes of workspace a call at ``res = (width, height)`` with ``levels`` levels needs (zdr_denoise_workspace_bytes)."""
    n = N.lib().zdr_denoise_workspace_bytes(C.byref(_params((res[1], res[0]), levels, 0.0, 0.0, 0.0)))
    if n == 0:
        raise N.ZdrError(f"libzdr_hip error: {N.lib().zdr_last_error().decode()}")
    return int(n)


def _check(x, aovs):
    if x.dim() != 3 or x.shape[2] != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError(f"the image must be a float32 (H, W, 4) tensor on the GPU, not {tuple(x.shape)} {x.dtype} on {x.device}")
    H, W = int(x.shape[0]), int(x.shape[1])
    if tuple(aovs.shape) != (H, W, N.AOV_CHANNELS) or aovs.dtype != torch.float32 or aovs.device != x.device:
        raise ValueError(f"aovs must be a float32 ({H}, {W}, {N.AOV_CHANNELS}) tensor on {x.device}")
    return H, W


def _call(fn, x, aovs, levels, sigmas, out, workspace):
    """One of the two C calls on torch's current stream: x -> out, both (H, W, 4) float32 and contiguous on the device of ``aovs``."""
    H, W = _check(x, aovs)
    x, aovs = x.contiguous(), aovs.contiguous()
    need = workspace_bytes((W, H), levels)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {tuple(x.shape)} tensor on {x.device}")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif workspace.device != x.device or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on {x.device}")
    p = _params((H, W), levels, *sigmas)
    with torch.cuda.device(x.device):
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        N.check(fn(C.byref(p), aovs.data_ptr(), x.data_ptr(), out.data_ptr(), workspace.data_ptr(), stream))
    return out


def denoise_forward(image, aovs, *, levels, sigma_normal, sigma_depth, sigma_albedo, out=None, workspace=None):
    """zdr_denoise: the filtered image.  ``aovs`` is the (H, W, 16) tensor; ``out`` and ``workspace`` (any tensor of at least
    ``workspace_bytes`` bytes) are allocated when not given.  Only enqueues, on torch's current stream."""
    return _call(N.lib().zdr_denoise, image, _data(aovs), levels, (sigma_normal, sigma_depth, sigma_albedo), out, workspace)


def denoise_backward(d_out, aovs, *, levels, sigma_normal, sigma_depth, sigma_albedo, d_image=None, workspace=None):
    """zdr_denoise_backward: the adjoint of ``denoise_forward`` with respect to the image, ``d_image`` overwritten.  Needs no forward
    call before it and nothing of it in ``workspace``."""
    return _call(N.lib().zdr_denoise_backward, d_out, _data(aovs), levels, (sigma_normal, sigma_depth, sigma_albedo), d_image, workspace)


class DenoiseOperator(torch.autograd.Function):
    """The linear core out = K image.  Gradient with respect to the image only; keeps nothing but the detached feature buffers."""
    @staticmethod
    def forward(ctx, image, aovs, levels, sigma_normal, sigma_depth, sigma_albedo):
        ctx.save_for_backward(aovs)
        ctx.args = dict(levels=levels, sigma_normal=sigma_normal, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo)
        return denoise_forward(image, aovs, **ctx.args)

    @staticmethod
    def backward(ctx, grad_output):
        aovs, = ctx.saved_tensors
        return denoise_backward(grad_output, aovs, **ctx.args), None, None, None, None, None


def demodulation_albedo(data, albedo_floor):
    """m of ``denoise(demodulate=True)``, (H, W, 3): max(albedo / coverage, ``albedo_floor``) where coverage > 0 and the hit has a
    material (slot >= 0), 1 elsewhere.  ``data`` is the (H, W, 16) feature tensor; differentiable in its albedo and coverage."""
    cov = data[..., 11:12]
    has = (cov > 0) & (data[..., 15:16] >= 0)
    return torch.where(has, (data[..., 0:3] / torch.where(has, cov, torch.ones_like(cov))).clamp_min(albedo_floor), torch.ones_like(data[..., 0:3]))


def denoise(image, aovs, *, levels=4, sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=None, demodulate=True, albedo_floor=1e-2):
    """Filters ``image`` ((H, W, 4) float32 on the GPU) with ``levels`` à-trous levels (1..6; steps 1, 2, 4, ...) whose weights stop at
    edges of the guides in ``aovs`` — an ``Aovs`` of ``Scene.render_aovs`` or its (H, W, 16) tensor, rendered with the same ``res``,
    ``spp`` and ``seed`` as the image.  Returns (H, W, 4); a constant alpha stays what it was.

    ``sigma_normal``, ``sigma_depth`` (relative to the depth) and ``sigma_albedo`` are the widths of the three edge-stopping terms of
    include/zdr.h; a width <= 0 switches its term off, and pixels of different instances never mix.  ``sigma_albedo=None`` means 0.2
    with ``demodulate``, 0.1 without: narrow without, where it is all that keeps texture detail; wide with, where the demodulation
    keeps the detail and the term is left to stop at unlike materials and at the rim of an emitter.  (It cannot be off there: a
    pixel on the rim of a light flush with the ceiling has the ceiling's normal, depth and — if its first sample hit the ceiling —
    instance, and only its albedo, which the light's samples pull towards 0, tells it from its neighbours.  With the term off the
    filter smeared such pixels and tripled the Cornell box's RMSE; profiles/denoise_quality.txt.)

    ``demodulate``: rgb is divided by m = max(albedo / coverage, ``albedo_floor``) before the filter and multiplied by it afterwards
    (m = 1 where nothing was hit or the hit has no material); alpha is filtered as it is.  This happens in torch around the kernel.

    Gradients: exact with respect to ``image`` (the adjoint kernel), and through m with respect to whatever ``aovs`` depends on (the
    materials, when it came from ``render_aovs``).  The edge-stopping weights are treated as constants: no gradient flows through
    them."""
    data = _data(aovs)
    _check(image, data)
    if sigma_albedo is None:
        sigma_albedo = 0.2 if demodulate else 0.1
    core = lambda x: DenoiseOperator.apply(x, data.detach(), int(levels), float(sigma_normal), float(sigma_depth), float(sigma_albedo))  # noqa: E731
    if not demodulate:
        return core(image)
    m = demodulation_albedo(data, albedo_floor)
    out = core(torch.cat([image[..., :3] / m, image[..., 3:]], -1))
    return torch.cat([out[..., :3] * m, out[..., 3:]], -1)
