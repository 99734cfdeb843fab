"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_image_pyramid, zdr_texel_gather_mip,
zdr_texel_gather_mip_backward and zdr_image_pyramid_backward captured in one HIP graph with torch.cuda.graph, on a single stream, and
replayed.  The calls never allocate and never synchronise, so they are captured WITHOUT an eager call before; a replay after the inputs
were overwritten in place gives what the eager calls give on them — bit for bit for the pyramid and the gather, within the adjoint's
bar (its atomics add in an order that varies from run to run) for d_image.  Anything that raises during the capture — an allocation, a
copy, a synchronise hidden in the Python layer — fails the test."""
import numpy as np
import pytest
import torch

import texel_mip_ref as MR
from test_texel_mip_ref_host import synthetic
from zdr_amd import _native as N
from zdr_amd import image_pyramid_backward, image_pyramid_forward, pyramid_layout, texel_gather_mip_backward, texel_gather_mip_forward

pytestmark = pytest.mark.gpu


def test_pyramid_gather_and_both_adjoints_can_be_captured_without_a_warm_up_and_replayed():
    res, n, footprint = (67, 35), 500, 1.5                           # a launch of two levels, then the fused tail
    npix = sum(w * h for w, h, _ in pyramid_layout(res)[1:])
    image, view, g = torch.zeros(res[1], res[0], 4, device="cuda"), torch.zeros(n, 1, 8, device="cuda"), torch.zeros(n, 1, 4, device="cuda")
    pyr, color = torch.zeros(npix, 4, device="cuda"), torch.zeros(n, 1, 4, device="cuda")
    d_image, d_pyr = torch.zeros(res[1], res[0], 4, device="cuda"), torch.zeros(npix, 4, device="cuda")
    N.lib()                                                          # the library is loaded; nothing of it has been launched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        image_pyramid_forward(image, out=pyr)
        texel_gather_mip_forward(image, pyr, view, footprint, out=color)
        texel_gather_mip_backward(g, view, res, footprint, d_image=d_image, d_pyramid=d_pyr)
        image_pyramid_backward(d_pyr, res, d_image=d_image)
    rng = np.random.default_rng(21)
    v = synthetic(rng, n, res, scale=(0.5, 24.0))
    gen = torch.Generator().manual_seed(9)
    image.copy_(torch.rand(res[1], res[0], 4, generator=gen)); g.copy_(torch.randn(n, 1, 4, generator=gen)); view.copy_(torch.from_numpy(v))
    pyr.fill_(7.0); color.fill_(7.0); d_image.zero_(); d_pyr.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = pyr.clone(), color.clone(), d_image.clone()
    want_pyr = image_pyramid_forward(image)
    assert torch.equal(got[0].view(torch.int32), want_pyr.view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), texel_gather_mip_forward(image, want_pyr, view, footprint).view(torch.int32)) and float(got[1].abs().sum()) > 0
    a64 = MR.gather_mip_adjoint_ref(g.cpu().numpy(), v, res, footprint)
    bar = MR.linear_bar(MR.gather_mip_adjoint_ref(g.cpu().numpy(), v, res, footprint, 0, np.float32), a64)
    err = float(np.abs(got[2].cpu().numpy() - a64).max())
    print(f"[texel mip graph] replayed full adjoint vs float64 transpose {err:.3e}; bar {bar:.3e}")
    assert err <= bar and float(got[2].abs().sum()) > 0
    del graph
