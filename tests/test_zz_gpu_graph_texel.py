"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_scene_texel_aovs captured in a HIP graph with
torch.cuda.graph and replayed.  The call never allocates and never synchronises, the scene is only read and the workspace is the
caller's, so it is captured WITHOUT an eager call before; the replay gives, bit for bit, what the eager call gives.  The graph is a
straight line of three kernels, no parallel branches.  Anything that raises during the capture — an allocation, a copy, a synchronise
hidden in the Python layer — fails the test."""
import pytest
import torch

import texel_cases as TC
from zdr_amd import Scene
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu


def test_the_texel_buffers_can_be_captured_without_a_warm_up_and_replayed():
    scene = Scene(TC.soup_arrays(), integrator="direct")            # a handle of its own: nothing was launched on it before
    scene.material_slots = [0]                                      # the slot table is uploaded here, before the capture
    H, W = 23, 31                                                   # a size no other texel test uses
    out = torch.zeros(H, W, N.AOV_CHANNELS, device="cuda")
    ws = torch.full((N.lib().zdr_texel_aovs_workspace_bytes(H, W),), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scene.texel_aovs_forward(0, (H, W), out=out, workspace=ws)
    for fill in (0.0, 7.0):
        out.fill_(fill); ws.fill_(0x11)                             # whatever the buffers held: the call overwrites both
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got, scene.texel_aovs_forward(0, (H, W)))
        assert float(got[..., 11].sum()) > 0 and float((got[..., 12] - got[..., 11]).sum()) > 0
    del graph
    scene.check()
