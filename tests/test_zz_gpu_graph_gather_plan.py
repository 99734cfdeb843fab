"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): ``GatherPlan.apply`` (zdr_gather_plan_apply) captured in a HIP
graph with torch.cuda.graph, on a single stream, WITHOUT an eager apply before — the call never allocates and never synchronises — and
replayed twice after ``d_color`` was overwritten in place.  The plan itself is built eagerly beforehand: its build synchronises once
and is not part of a step.  The apply has no atomic and a defined summation order, so every replay must give the eager call's bits.
Anything that raises during the capture — an allocation, a copy, a synchronise hidden in the Python layer — fails the test."""
import pytest
import torch

import test_gpu_texel_project as TP
import texel_aniso_cases as AC
from zdr_amd import TexelView, image_pyramid_backward, pyramid_layout, texel_footprint_forward

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("filter,kw", [("bilinear", {}), ("mip", {"footprint": 2.0}), ("aniso", {"footprint": 1.5, "max_aniso": 8})])
def test_the_apply_can_be_captured_without_a_warm_up_and_replays_the_eager_bits(filter, kw):
    name, res = "cbox_16x16_standard", (67, 35)
    cam, pts = TP.camera(AC.CASES[name][1]), TP.case_points(name)
    view = TexelView(TP.case_scene(name, "bvh").texel_view_forward(pts, res, camera=cam), res, texel_footprint_forward(pts, res, cam))
    plan = view.gather_plan(res, filter, **kw)                       # (the build: eager, one synchronisation; no apply has run)
    H, W = view.data.shape[:2]
    npix = max(sum(w * h for w, h, _ in pyramid_layout(res)[1:]), 1)
    g = torch.zeros(H, W, 4, device="cuda")
    d_image = torch.zeros(res[1], res[0], 4, device="cuda")
    d_pyr = None if filter == "bilinear" else torch.zeros(npix, 4, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.apply(g, d_image, d_pyr)
        if d_pyr is not None:
            image_pyramid_backward(d_pyr, res, d_image=d_image)
    gen = torch.Generator().manual_seed(12)
    for replay in range(2):
        g.copy_(torch.randn(H, W, 4, generator=gen))
        d_image.zero_()
        if d_pyr is not None:
            d_pyr.fill_(float("nan"))                                # (written, never read)
        graph.replay()
        torch.cuda.synchronize()
        got = d_image.clone()
        want = plan.adjoint(g)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and float(got.abs().sum()) > 0, (filter, replay)
    del graph
