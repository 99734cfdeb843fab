"""Push-pull hole filling (include/zdr.h, zdr_push_pull): the texels of an (H, W, 4) texture whose weight is 0 are filled from the ones
whose weight is positive, through a weighted pyramid, and the texels of weight 1 come out bit for bit as they went in — a baker's seam
padding, with the masks of ``Scene.texel_aovs`` as the weight.

    f = scene.texel_aovs(theta)                              # coverage, reach: what each texel is
    material = push_pull(theta, f.coverage)                  # (H, W, 4), differentiable in theta
    scene.render(material, res=res, spp=spp, seed=s).sum().backward()

The map is linear in the texture while the weight is held fixed; its adjoint is a HIP kernel as well, exact and deterministic.  So
``push_pull(theta, coverage)`` is a reparameterisation of the material: padding and unreached texels are always the smooth continuation
of their chart, the gradient that spills onto them is carried back to the covered texels that determine them, and ``theta.grad`` is
exactly 0 wherever the weight is 0.  The WEIGHT is not differentiated: it receives no gradient.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N


def _params(shape, levels) -> N.PushPullParams:
    p = N.PushPullParams()
    p.struct_size = C.sizeof(N.PushPullParams)
    p.height, p.width, p.levels = int(shape[0]), int(shape[1]), 0 if levels is None else int(levels)
    return p


def workspace_bytes(res, levels=None) -> int:
    """Bytes of workspace a call at ``res = (width, height)`` needs (zdr_push_pull_workspace_bytes); ``levels=None``: down to 1 x 1."""
    n = N.lib().zdr_push_pull_workspace_bytes(C.byref(_params((res[1], res[0]), levels)))
    if n == 0:
        raise N.ZdrError(f"libzdr_hip error: {N.lib().zdr_last_error().decode()}")
    return int(n)


def _check(x, weight, levels):
    if x.dim() != 3 or x.shape[2] != 4 or x.shape[0] < 1 or x.shape[1] < 1 or x.dtype != torch.float32:
        raise ValueError(f"the texture must be a float32 (H, W, 4) tensor, not {tuple(x.shape)} {x.dtype}")
    H, W = int(x.shape[0]), int(x.shape[1])
    if tuple(weight.shape) != (H, W) or weight.dtype not in (torch.float32, torch.bool):
        raise ValueError(f"weight must be a float32 or bool ({H}, {W}) tensor, not {tuple(weight.shape)} {weight.dtype}")
    if levels is not None and int(levels) < 1:
        raise ValueError(f"levels must be None (down to 1 x 1) or a positive count, not {levels}")
    if not x.is_cuda or weight.device != x.device:
        raise ValueError(f"the texture and the weight must be on one GPU, not on {x.device} and {weight.device}")
    return H, W


def _call(fn, x, weight, levels, out, workspace):
    """One of the two C calls on torch's current stream: x -> out, both (H, W, 4) float32 and contiguous on the device of ``x``."""
    H, W = _check(x, weight, levels)
    x = x.contiguous()
    weight = (weight.float() if weight.dtype == torch.bool else weight).contiguous()      # (a view such as TexelAovs.coverage is copied)
    need = workspace_bytes((W, H), levels)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 {tuple(x.shape)} tensor on {x.device}")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif workspace.device != x.device or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"workspace must be a contiguous tensor of at least {need} bytes on {x.device}")
    p = _params((H, W), levels)
    with torch.cuda.device(x.device):
        stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        N.check(fn(C.byref(p), weight.data_ptr(), x.data_ptr(), out.data_ptr(), workspace.data_ptr(), stream))
    return out


def push_pull_forward(x, weight, *, levels=None, out=None, workspace=None):
    """zdr_push_pull: the filled texture.  ``weight`` is (H, W), float32 or bool; ``out`` and ``workspace`` (any tensor of at least
    ``workspace_bytes`` bytes) are allocated when not given.  Only enqueues, on torch's current stream."""
    return _call(N.lib().zdr_push_pull, x, weight, levels, out, workspace)


def push_pull_backward(d_out, weight, *, levels=None, d_x=None, workspace=None):
    """zdr_push_pull_backward: the adjoint of ``push_pull_forward`` with respect to the texture, ``d_x`` overwritten.  Needs no forward
    call before it and nothing of it in ``workspace``.  The weight receives no gradient."""
    return _call(N.lib().zdr_push_pull_backward, d_out, weight, levels, d_x, workspace)


class PushPullOperator(torch.autograd.Function):
    """The linear map y = K x.  Gradient with respect to the texture only; keeps nothing but the detached weight."""
    @staticmethod
    def forward(ctx, x, weight, levels):
        ctx.save_for_backward(weight)
        ctx.levels = levels
        return push_pull_forward(x, weight, levels=levels)

    @staticmethod
    def backward(ctx, grad_output):
        weight, = ctx.saved_tensors
        return push_pull_backward(grad_output, weight, levels=ctx.levels), None, None


def push_pull(x, weight, *, levels=None):
    """Fills ``x`` ((H, W, 4) float32 on the GPU) where ``weight`` ((H, W), float32 in [0, 1] or bool — ``TexelAovs.coverage`` or
    ``.reach``) is 0 from where it is positive, and returns (H, W, 4).  Definition (include/zdr.h has the operation order):

        a_0 = clamp(w, 0, 1), p_0 = a_0 x;  push: a_{l+1} = min(S, 1), p_{l+1} = P a_{l+1} / S over the 2 x 2 children's sums S, P;
        top: y_L = p_L / a_L;  pull: y_l = p_l + (1 - a_l) U(y_{l+1}), U bilinear with taps 0.75 / 0.25;  y = x where w = 1.

    Every output texel is a convex combination of the texels of positive weight; what sits behind weight 0 — NaN included — is never
    read into the result.  ``levels``: stop the pyramid after that many halvings (None: down to 1 x 1); holes it cannot reach are 0.

    Gradients: exact with respect to ``x`` (the adjoint kernel, no atomics: the same bits from run to run), exactly 0 where the weight
    is 0.  The weight is treated as a constant: no gradient flows to it."""
    _check(x, weight, levels)
    w = weight.detach()
    w = (w.float() if w.dtype == torch.bool else w).contiguous()
    return PushPullOperator.apply(x, w, None if levels is None else int(levels))
