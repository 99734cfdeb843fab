"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_scene_texel_view, zdr_texel_gather and
zdr_texel_gather_backward captured in one HIP graph with torch.cuda.graph, on a single stream, and replayed.  The calls never allocate
and never synchronise, and the workspace is the caller's, so they are captured WITHOUT an eager call before; a replay after the inputs
were overwritten in place gives what the eager calls give on them — bit for bit for the view buffer and the gather, within the adjoint's
bar (its atomics add in an order that varies from run to run) for d_image.  Anything that raises during the capture — an allocation, a
copy, a synchronise hidden in the Python layer — fails the test."""
import numpy as np
import pytest
import torch

import texel_lighting_cases as LC
import texel_project_cases as PC
from zdr_amd import Camera, Scene, float3, texel_gather_backward, texel_gather_forward
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_view_gather_and_adjoint_can_be_captured_without_a_warm_up_and_replayed(accel):
    name = "cbox_64x64_standard"
    res = PC.CASES[name][2]
    fov, o, t, up = PC.CAMERAS["standard"]
    cam = Camera(fov=fov, origin=float3(*o), target=float3(*t), up=float3(*up))
    scene = Scene(LC.CASES[PC.CASES[name][0]][0](), integrator="direct", accel=accel)       # a fresh handle: nothing ran on it before
    gen = torch.Generator().manual_seed(9)
    pts = torch.zeros(64, 64, 16, device="cuda")
    image, g = torch.zeros(res[1], res[0], 4, device="cuda"), torch.zeros(64, 64, 4, device="cuda")
    view, color, d_image = torch.zeros(64, 64, 8, device="cuda"), torch.zeros(64, 64, 4, device="cuda"), torch.zeros(res[1], res[0], 4, device="cuda")
    ws = torch.empty(N.lib().zdr_texel_view_workspace_bytes(64, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scene.texel_view_forward(pts, res, camera=cam, out=view, workspace=ws)
        texel_gather_forward(image, view, out=color)
        texel_gather_backward(g, view, res, d_image=d_image)
    pts.copy_(torch.from_numpy(PC.points(name)))
    image.copy_(torch.rand(res[1], res[0], 4, generator=gen)); g.copy_(torch.randn(64, 64, 4, generator=gen))
    view.fill_(7.0); color.fill_(7.0); d_image.zero_(); ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    got = view.clone(), color.clone(), d_image.clone()
    want_view = scene.texel_view_forward(pts, res, camera=cam)
    assert torch.equal(got[0].view(torch.int32), want_view.view(torch.int32)) and float(got[0][..., 0].sum()) > 0
    assert torch.equal(got[1].view(torch.int32), texel_gather_forward(image, want_view).view(torch.int32)) and float(got[1].abs().sum()) > 0
    bar, ref = PC.linear_bar(want_view.cpu().numpy(), g.cpu().numpy(), res, True)
    err = float(np.abs(got[2].cpu().numpy() - ref).max())
    print(f"[texel project graph] {accel}: replayed adjoint vs float64 transpose {err:.3e}; bar {bar:.3e}")
    assert err <= bar and float(got[2].abs().sum()) > 0
    del graph
    scene.check()
