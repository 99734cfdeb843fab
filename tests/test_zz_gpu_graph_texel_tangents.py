"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_scene_texel_tangents and zdr_texel_footprint_tangents
captured in one HIP graph with torch.cuda.graph and replayed.  The calls never allocate and never synchronise, the scene is only read
and the workspace is the caller's, so they are captured WITHOUT an eager call before; the replay gives, bit for bit, what the eager
calls give.  The graph is a straight line of five kernels, no parallel branches.  Anything that raises during the capture — an
allocation, a copy, a synchronise hidden in the Python layer — fails the test."""
import pytest
import torch

import texel_cases as TC
import texel_tangent_cases as TT
from zdr_amd import Camera, Scene, float3, texel_footprint_forward
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu


def test_the_tangent_calls_can_be_captured_without_a_warm_up_and_replayed():
    scene = Scene(TC.cbox_arrays(), integrator="direct")            # a handle of its own: nothing was launched on it before
    scene.material_slots = [0, None]                                # the slot table is uploaded here, before the capture
    fov, o, t, up = TT.FOOTPRINT_CASES["cbox_16x64"][1]
    cam = Camera(fov=fov, origin=float3(*o), target=float3(*t), up=float3(*up))
    H, W, res = 19, 45, (40, 24)                                    # a size no other texel test uses
    aovs, tan, fp = (torch.zeros(H, W, c, device="cuda") for c in (N.AOV_CHANNELS, 8, 4))
    ws = torch.full((N.lib().zdr_texel_aovs_workspace_bytes(H, W),), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scene.texel_tangents_forward(0, (H, W), out=tan, aovs_out=aovs, workspace=ws)
        texel_footprint_forward(aovs, res, cam, out=fp, tangents=tan)
    for fill in (0.0, float("nan")):
        aovs.fill_(fill); tan.fill_(fill); fp.fill_(fill); ws.fill_(0x11)      # whatever the buffers held: the calls overwrite all four
        graph.replay()
        torch.cuda.synchronize()
        got = aovs.clone(), tan.clone(), fp.clone()
        want_aovs, want_tan = scene.texel_tangents_forward(0, (H, W))
        want_fp = texel_footprint_forward(want_aovs, res, cam, tangents=want_tan)
        for g, w in zip(got, (want_aovs, want_tan, want_fp)):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
        assert torch.equal(got[0].view(torch.int32), scene.texel_aovs_forward(0, (H, W)).view(torch.int32))
        assert float(got[1][..., 3].sum()) > 0 and float(got[2][..., 3].sum()) > 0
    del graph
    scene.check()
