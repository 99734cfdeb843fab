"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_push_pull and zdr_push_pull_backward captured in one HIP
graph with torch.cuda.graph, on a single stream, and replayed.  The calls never allocate and never synchronise, and the workspace is the
caller's, so they are captured WITHOUT an eager call before; a replay after the inputs were overwritten in place gives, bit for bit,
what the eager calls give on them.  Anything that raises during the capture — an allocation, a copy, a synchronise hidden in the Python
layer — fails the test."""
import pytest
import torch

from push_pull_ref import make_weight
from zdr_amd.pushpull import push_pull_backward, push_pull_forward, workspace_bytes

pytestmark = pytest.mark.gpu


def test_push_pull_and_its_adjoint_can_be_captured_without_a_warm_up_and_replayed():
    W, H = 150, 70                                               # three level launches each way around the fused tail (19 x 9)
    gen = torch.Generator().manual_seed(5)
    w, x, g = make_weight("charts", H, W).cuda(), torch.rand(H, W, 4, generator=gen).cuda(), torch.rand(H, W, 4, generator=gen).cuda()
    out, d_x = torch.zeros_like(x), torch.zeros_like(x)
    ws = torch.empty(workspace_bytes((W, H)), dtype=torch.uint8, device="cuda")      # one workspace: the two calls follow each other on one stream
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        push_pull_forward(x, w, out=out, workspace=ws)
        push_pull_backward(g, w, d_x=d_x, workspace=ws)
    for seed, kind in ((6, "binary"), (7, "fractional")):
        gen = torch.Generator().manual_seed(seed)
        w.copy_(make_weight(kind, H, W, seed)); x.copy_(torch.rand(H, W, 4, generator=gen)); g.copy_(torch.rand(H, W, 4, generator=gen))
        out.zero_(); d_x.zero_(); ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone(), d_x.clone()
        assert torch.equal(got[0], push_pull_forward(x, w)) and torch.equal(got[1], push_pull_backward(g, w))
        assert float(got[0].abs().sum()) > 0 and float(got[1].abs().sum()) > 0
        assert torch.equal(got[0][w == 1], x[w == 1])
    del graph
