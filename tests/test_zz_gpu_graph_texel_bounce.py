"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_scene_texel_bounce captured in a HIP graph with
torch.cuda.graph and replayed twice.  The call never allocates and never synchronises, its grid does not depend on the list it compacts
on the device, the scene is only read, the workspace is the caller's and the material table is a kernel argument, so it is captured
WITHOUT an eager call before; the replay gives, bit for bit, what the eager call gives.  The graph is a straight line of three kernels,
no parallel branches.  Anything that raises during the capture — an allocation, a copy, a synchronise hidden in the Python layer — fails
the test."""
import pytest
import torch

import texel_bounce_cases as BC
from zdr_amd import Scene
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_the_bounce_can_be_captured_without_a_warm_up_and_replayed(accel):
    name = "multi_k3"
    scene = Scene(BC.CASES[name][0](), integrator="direct", accel=accel)     # a handle of its own: nothing was launched on it before
    scene.material_slots = BC.MULTI_SLOTS                           # (the slot table is the scene's state, set before the capture)
    pts = torch.from_numpy(BC.points(name)).cuda()
    mats = BC.materials(name)
    packed = torch.cat([torch.from_numpy(m).reshape(-1, 4) for m in mats]).cuda()
    dims = [m.shape[:2] for m in mats]
    H, W = pts.shape[:2]
    out = torch.zeros(H, W, 4, device="cuda")
    ws = torch.full((N.lib().zdr_texel_bounce_workspace_bytes(H, W),), 0xAB, dtype=torch.uint8, device="cuda")
    kw = dict(spp=9, bounces=3, seed=5, samples=(1, 8), dims=dims)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scene.texel_bounce_forward(pts, packed, out=out, workspace=ws, **kw)
    for fill in (0.0, 7.0):
        out.fill_(fill); ws.fill_(0x11)                             # whatever the buffers held: the call overwrites both
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got.view(torch.int32), scene.texel_bounce_forward(pts, packed, **kw).view(torch.int32))
        assert float(got[..., :3].sum()) > 0 and 0 < float(got[..., 3].sum())
    del graph
    scene.check()
