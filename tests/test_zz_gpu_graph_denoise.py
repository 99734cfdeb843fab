"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_denoise and zdr_denoise_backward captured in a HIP graph
with torch.cuda.graph and replayed.  The calls never allocate and never synchronise, and the workspace is the caller's, so they are
captured WITHOUT an eager call before; a replay on changed inputs gives, bit for bit, what the eager calls give on them.  Anything
that raises during the capture — an allocation, a copy, a synchronise hidden in the Python layer — fails the test."""
import pytest
import torch

from denoise_ref import synthetic_aovs
from zdr_amd.denoiser import denoise_backward, denoise_forward, workspace_bytes

pytestmark = pytest.mark.gpu


def test_the_denoiser_and_its_adjoint_can_be_captured_without_a_warm_up_and_replayed():
    W, H = 70, 45                                                # a size no other denoiser test uses: nothing was launched at it before
    k = dict(levels=5, sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=0.1)
    gen = torch.Generator().manual_seed(5)
    aovs, image, cot = synthetic_aovs(H, W, 1).cuda(), torch.rand(H, W, 4, generator=gen).cuda(), torch.rand(H, W, 4, generator=gen).cuda()
    out, d_image = torch.zeros_like(image), torch.zeros_like(image)
    ws_f, ws_b = (torch.empty(workspace_bytes((W, H), 5), dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        denoise_forward(image, aovs, out=out, workspace=ws_f, **k)
        denoise_backward(cot, aovs, d_image=d_image, workspace=ws_b, **k)
    for seed in (6, 7):
        gen = torch.Generator().manual_seed(seed)
        aovs.copy_(synthetic_aovs(H, W, seed)); image.copy_(torch.rand(H, W, 4, generator=gen)); cot.copy_(torch.rand(H, W, 4, generator=gen))
        out.zero_(); d_image.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone(), d_image.clone()
        assert torch.equal(got[0], denoise_forward(image, aovs, **k)) and torch.equal(got[1], denoise_backward(cot, aovs, **k))
        assert float(got[0].abs().sum()) > 0 and float(got[1].abs().sum()) > 0
    del graph
