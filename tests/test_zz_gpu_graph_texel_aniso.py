"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_texel_footprint, zdr_image_pyramid,
zdr_texel_gather_aniso, zdr_texel_gather_aniso_backward and zdr_image_pyramid_backward captured in one HIP graph with torch.cuda.graph,
on a single stream, and replayed.  The calls never allocate and never synchronise, so they are captured WITHOUT an eager call before; a
replay after the inputs were overwritten in place gives what the eager calls give on them — bit for bit for the footprint buffer and
the gather, within the adjoint's bar (its atomics add in an order that varies from run to run) for d_image.  Anything that raises
during the capture — an allocation, a copy, a synchronise hidden in the Python layer — fails the test."""
import numpy as np
import pytest
import torch

import test_gpu_texel_project as TP
import texel_aniso_cases as AC
import texel_aniso_ref as AR
from zdr_amd import _native as N
from zdr_amd import (image_pyramid_backward, image_pyramid_forward, pyramid_layout, texel_footprint_forward, texel_gather_aniso_backward,
                     texel_gather_aniso_forward)

pytestmark = pytest.mark.gpu


def test_footprint_gather_and_adjoint_can_be_captured_without_a_warm_up_and_replayed():
    name, res, footprint, max_aniso = "cbox_16x16_standard", (67, 35), 1.5, 8   # (a launch of two levels, then the fused tail)
    cam = TP.camera(AC.CASES[name][1])
    want_view = TP.case_scene(name, "bvh").texel_view_forward(TP.case_points(name), res, camera=cam)      # (the view buffer is an input here)
    H, W = want_view.shape[:2]
    npix = sum(w * h for w, h, _ in pyramid_layout(res)[1:])
    pts, view = torch.zeros(H, W, 16, device="cuda"), torch.zeros(H, W, 8, device="cuda")
    image, g = torch.zeros(res[1], res[0], 4, device="cuda"), torch.zeros(H, W, 4, device="cuda")
    fp, pyr, color = torch.zeros(H, W, 4, device="cuda"), torch.zeros(npix, 4, device="cuda"), torch.zeros(H, W, 4, device="cuda")
    d_image, d_pyr = torch.zeros(res[1], res[0], 4, device="cuda"), torch.zeros(npix, 4, device="cuda")
    N.lib()                                                          # the library is loaded; nothing of libzdr_aniso.so has been launched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        texel_footprint_forward(pts, res, cam, out=fp)
        image_pyramid_forward(image, out=pyr)
        texel_gather_aniso_forward(image, pyr, view, fp, footprint, max_aniso, out=color)
        texel_gather_aniso_backward(g, view, fp, res, footprint, max_aniso, d_image=d_image, d_pyramid=d_pyr)
        image_pyramid_backward(d_pyr, res, d_image=d_image)
    gen = torch.Generator().manual_seed(10)
    pts.copy_(TP.case_points(name)); view.copy_(want_view)
    image.copy_(torch.rand(res[1], res[0], 4, generator=gen)); g.copy_(torch.rand(H, W, 4, generator=gen))
    fp.fill_(7.0); pyr.fill_(7.0); color.fill_(7.0); d_image.zero_(); d_pyr.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = fp.clone(), color.clone(), d_image.clone()
    want_fp = texel_footprint_forward(pts, res, cam)
    assert torch.equal(got[0].view(torch.int32), want_fp.view(torch.int32)) and float(got[0].abs().sum()) > 0
    want = texel_gather_aniso_forward(image, image_pyramid_forward(image), view, want_fp, footprint, max_aniso)
    assert torch.equal(got[1].view(torch.int32), want.view(torch.int32)) and float(got[1].abs().sum()) > 0
    v, f = view.cpu().numpy(), want_fp.cpu().numpy()
    Ns = AR.probes(f[v[..., 0] == 1], footprint, max_aniso)[0]
    assert Ns.max() == max_aniso and Ns.min() == 1
    a64 = AR.gather_aniso_adjoint_ref(g.cpu().numpy(), v, f, res, footprint, max_aniso)
    bar = AC.gather_bar(AR.gather_aniso_adjoint_ref(g.cpu().numpy(), v, f, res, footprint, max_aniso, 0, np.float32), a64)
    err = float(np.abs(got[2].cpu().numpy() - a64).max())
    print(f"[texel aniso graph] replayed full adjoint vs float64 transpose {err:.3e}; bar {bar:.3e}")
    assert err <= bar and float(got[2].abs().sum()) > 0
    del graph
