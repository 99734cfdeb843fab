"""The gather plan (include/zdr.h, zdr_gather_plan_*): the adjoint of ``texel_gather`` — bilinear, mip or aniso — without float atomics.

    plan = view.gather_plan(res, filter="mip")               # once per (view, image size, filter): ONE synchronisation, to learn nnz
    d_image = plan.adjoint(d_color)                          # every step: a gather over CSR rows, the same bits from run to run
    color = texel_gather(photo, view, filter="mip", plan=True)     # the same forward; .backward() goes through the (cached) plan

With the view held fixed the gather is a sparse linear map, and a view is fixed for as long as camera and geometry are.  The plan lays
that map's transpose out as rows per destination pixel — level 0 first, then the packed levels >= 1 of the pyramid — each row holding
(texel, weight) entries in the order the scatter kernels enumerate them; ``apply`` sums a row in a defined order (sixteen sub-sums and
a tree, include/zdr.h), adds it into ``d_image`` and writes it to ``d_pyramid``.  The weights are the scatter kernels' own products, so
an entry times ``d_color`` is bit for bit the addend of the atomic adjoint: the two differ in the order of the additions alone.
A plan takes 8 bytes per entry and 4 per row; the build needs about 16 more bytes per entry, and the sort's own buffers, while it runs.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as N
from . import mip as M
from . import project as P

FILTER_IDS = {"bilinear": 0, "mip": 1, "aniso": 2}
MAX_NNZ = 2 ** 31 - 1


def plan_key(res, filter, footprint=1.0, max_aniso=8, levels=0):
    """What a plan is built for, the parameters its filter does not read left out (None): (res, filter, footprint, max_aniso, levels)."""
    if filter not in FILTER_IDS:
        raise ValueError(f"filter must be one of {P.FILTERS}, not {filter!r}")
    res = (int(res[0]), int(res[1]))
    if filter == "bilinear":
        return (res, filter, None, None, None)
    return (res, filter, float(footprint), int(max_aniso) if filter == "aniso" else None, M._levels_arg(levels))


class GatherPlan:
    """The transpose of one gather, from ``gather_plan``: ``row_start`` (rows + 1,) int32 and ``entries`` (nnz, 2) int32 — column 0 the
    texel index, column 1 the bits of the float32 weight (``texels``, ``weights`` read them) — in the CSR layout of include/zdr.h;
    ``nnz``; ``res`` = (width, height) of the image, ``filter``, ``footprint``, ``max_aniso``, ``levels`` (None where the filter does
    not read them), ``tex_hw`` the texture's size, ``rows`` the number of destinations, ``stamp`` the ``view_stamp`` of the buffers it
    was built from."""

    def __init__(self, params, row_start, entries_buffer, nnz, key, tex_hw, stamp=None):
        self._params, self._buffer, self.stamp = params, entries_buffer, stamp
        self.row_start, self.entries, self.nnz = row_start, entries_buffer[:nnz], nnz
        self.key = key
        self.res, self.filter, self.footprint, self.max_aniso, self.levels = key
        self.tex_hw, self.rows = tex_hw, int(row_start.shape[0]) - 1
        self.device = row_start.device

    texels = property(lambda self: self.entries[:, 0])
    weights = property(lambda self: self.entries[:, 1].view(torch.float32))

    @property
    def nbytes(self):
        """bytes of the plan on the device: 8 per entry, 4 per row"""
        return 8 * self.nnz + 4 * (self.rows + 1)

    def apply(self, d_color, d_image=None, d_pyramid=None):
        """zdr_gather_plan_apply: every row summed in the header's order; ADDED INTO ``d_image`` ((height, width, 4); a zero tensor when
        not given; a pixel no texel taps is not touched) and, for mip and aniso, WRITTEN to ``d_pyramid`` (the packed levels >= 1;
        allocated when not given, never read, no need to zero it).  Returns ``d_image``, or ``(d_image, d_pyramid)`` for mip and aniso.
        Only enqueues, on torch's current stream: no allocation when the outputs are given, no synchronisation."""
        w, h = self.res
        P._check_image(d_color, "d_color", self.device)
        if tuple(d_color.shape[:2]) != self.tex_hw:
            raise ValueError(f"d_color must have the plan's texture size {self.tex_hw}, not {tuple(d_color.shape[:2])}")
        d_image = P._out(d_image, (h, w, 4), self.device, "d_image")
        if d_image is None:
            d_image = torch.zeros((h, w, 4), dtype=torch.float32, device=self.device)
        pyr = 0
        if self.filter != "bilinear":
            if d_pyramid is None:
                d_pyramid = torch.empty((M.pyramid_pixels(self.res, self.levels), 4), dtype=torch.float32, device=self.device)
            M._check_packed(d_pyramid, "d_pyramid", self.res, self.levels, self.device)
            pyr = d_pyramid.data_ptr()
        elif d_pyramid is not None:
            raise ValueError("a bilinear plan has no pyramid: d_pyramid must be None")
        d_color = d_color.detach().contiguous()
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            N.check(N.lib().zdr_gather_plan_apply(C.byref(self._params), self.row_start.data_ptr(), self._buffer.data_ptr(), d_color.data_ptr(),
                                                  d_image.data_ptr(), pyr, stream))
        return d_image if self.filter == "bilinear" else (d_image, d_pyramid)

    def adjoint(self, d_color):
        """The full image gradient (height, width, 4) of the gather for the texture-space gradient ``d_color``: ``apply`` into a zero
        image, then ``image_pyramid_backward`` for mip and aniso."""
        if self.filter == "bilinear":
            return self.apply(d_color)
        d_image, d_pyramid = self.apply(d_color)
        return M.image_pyramid_backward(d_pyramid, self.res, self.levels, d_image=d_image)


def view_stamp(view, filter):
    """What identifies the buffers a plan was built from: address and version counter of the view buffer and, for "aniso", of the
    footprint buffer.  An in-place write to either, or another tensor in their place, changes it."""
    data = getattr(view, "data", view)
    stamp = (data.data_ptr(), data._version)
    fp = getattr(view, "footprint_data", None)
    if filter == "aniso" and isinstance(fp, torch.Tensor):
        stamp += (fp.data_ptr(), fp._version)
    return stamp


def _params(view, key) -> N.GatherPlanParams:
    res, filter, footprint, max_aniso, levels = key
    if filter == "mip":
        P._mip_params(view, res, levels, footprint)                  # (raises on a bad footprint)
    elif filter == "aniso":
        P._aniso_params(view, res, levels, footprint, max_aniso)     # (raises on a bad footprint or max_aniso)
    p = N.GatherPlanParams()
    p.struct_size = C.sizeof(N.GatherPlanParams)
    p.tex_h, p.tex_w, p.width, p.height = int(view.shape[0]), int(view.shape[1]), res[0], res[1]
    p.filter, p.levels = FILTER_IDS[filter], levels or 0
    p.footprint, p.max_aniso = (1.0 if footprint is None else footprint), (1 if max_aniso is None else max_aniso)
    return p


def gather_plan(view, res, filter="bilinear", footprint=1.0, max_aniso=8, levels=0) -> GatherPlan:
    """The plan of ``texel_gather(image, view, filter=...)`` for images of ``res`` = (width, height): a ``GatherPlan``.  ``view``: a
    ``TexelView`` or its (H, W, 8) tensor; "aniso" reads the view's footprint buffer and raises ``ValueError`` when it has none.
    The build SYNCHRONISES ONCE, to learn the number of entries before it allocates them; it is a one-off per view, like
    ``Scene.add_envmap``.  ``footprint``, ``max_aniso``, ``levels``: as the filter's own gather takes them."""
    key = plan_key(res, filter, footprint, max_aniso, levels)
    if key[0][0] < 1 or key[0][1] < 1:
        raise ValueError(f"res must be a positive (width, height), not {res}")
    footprint_data = getattr(view, "footprint_data", None)
    stamp = view_stamp(view, filter) if isinstance(getattr(view, "data", view), torch.Tensor) else None
    view = P._view_data(view)
    fp = 0
    if filter == "aniso":
        if footprint_data is None:
            raise ValueError('filter="aniso" needs a view that carries a footprint buffer: scene.texel_view(..., footprint=True)')
        footprint_data = P._footprint_data(footprint_data, view)
        fp = footprint_data.data_ptr()
    p = _params(view, key)
    L = N.lib()
    rows = int(L.zdr_gather_plan_rows(C.byref(p)))
    if rows == 0:
        raise N.ZdrError(f"zdr_gather_plan_rows: {L.zdr_last_error().decode()}")
    with torch.cuda.device(view.device):
        stream = C.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
        ws = torch.empty(int(L.zdr_gather_plan_workspace_bytes(C.byref(p), 0)), dtype=torch.uint8, device=view.device)
        N.check(L.zdr_gather_plan_count(C.byref(p), view.data_ptr(), fp, ws.data_ptr(), stream))
        nnz = int(ws[:8].view(torch.int64).item())                  # the build's one synchronisation
        if nnz > MAX_NNZ:
            raise N.ZdrError(f"the plan would have {nnz} entries: more than 2^31 - 1")
        nbytes = int(L.zdr_gather_plan_workspace_bytes(C.byref(p), nnz))
        if nbytes == 0:
            raise N.ZdrError(f"zdr_gather_plan_workspace_bytes: {L.zdr_last_error().decode()}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=view.device)
        row_start = torch.empty(rows + 1, dtype=torch.int32, device=view.device)
        entries = torch.empty((max(nnz, 2), 2), dtype=torch.int32, device=view.device)     # (never empty: the pointer is not null)
        N.check(L.zdr_gather_plan_build(C.byref(p), view.data_ptr(), fp, nnz, ws.data_ptr(), row_start.data_ptr(), entries.data_ptr(), stream))
    return GatherPlan(p, row_start, entries, nnz, key, (int(view.shape[0]), int(view.shape[1])), stamp)


def resolve_plan(plan, view_object, view, key):
    """The ``GatherPlan`` that ``plan`` — True or a plan — stands for in a gather of ``key`` through ``view``.  True builds it on first
    use and keeps it on the ``TexelView``, and builds it anew when the view's buffers are no longer the ones it was built from (another
    tensor, or an in-place write: ``view_stamp``); a plan made for another key, texture size or view raises ``ValueError``."""
    if plan is True:
        if isinstance(view_object, torch.Tensor) or not hasattr(view_object, "__dict__"):
            raise ValueError("plan=True keeps the plan on the TexelView: pass the TexelView, or a GatherPlan made with gather_plan")
        cache = view_object.__dict__.setdefault("_gather_plans", {})
        if key not in cache or cache[key].stamp != view_stamp(view_object, key[1]):
            cache[key] = gather_plan(view_object, *key[:2], **{k: v for k, v in zip(("footprint", "max_aniso", "levels"), key[2:]) if v is not None})
        return cache[key]
    if not isinstance(plan, GatherPlan):
        raise ValueError(f"plan must be None, True or a GatherPlan, not {plan!r}")
    if plan.key != key:
        raise ValueError(f"the plan was made for (res, filter, footprint, max_aniso, levels) = {plan.key}, this gather is {key}")
    if plan.tex_hw != (int(view.shape[0]), int(view.shape[1])) or plan.device != view.device:
        raise ValueError(f"the plan was made for a {plan.tex_hw} texture on {plan.device}, not for {tuple(view.shape[:2])} on {view.device}")
    if plan.stamp != view_stamp(view_object, key[1]):
        raise ValueError("the plan was made from other view (or footprint) buffers than this gather's, or they were written to since: build it again")
    return plan


class TexelGatherPlanOperator(torch.autograd.Function):
    """color = K image with the forward of ``texel_gather`` — the same calls, the same bits — and K^T through a plan."""
    @staticmethod
    def forward(ctx, image, plan, view, footprint_data):
        ctx.plan = plan
        if plan.filter == "bilinear":
            return P.texel_gather_forward(image, view)
        if plan.filter == "mip":
            return P.texel_gather_mip_forward(image, M.image_pyramid_forward(image), view, plan.footprint)
        return P.texel_gather_aniso_forward(image, M.image_pyramid_forward(image), view, footprint_data, plan.footprint, plan.max_aniso)

    @staticmethod
    def backward(ctx, grad_output):
        return ctx.plan.adjoint(grad_output), None, None, None
