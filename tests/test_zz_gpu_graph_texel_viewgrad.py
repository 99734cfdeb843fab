"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_texel_gather_dview (bilinear and mip) and
zdr_texel_view_backward captured in one HIP graph with torch.cuda.graph, on a single stream, and replayed.  The calls never allocate
and never synchronise, and the workspace is the caller's, so they are captured WITHOUT an eager call before; a replay after the inputs
were overwritten in place gives, bit for bit, what the eager calls give on them: neither has an atomic.  Anything that raises during
the capture — an allocation, a copy, a synchronise hidden in the Python layer — fails the test."""
import pytest
import torch

import texel_lighting_cases as LC
import texel_project_cases as PC
import texel_viewgrad_cases as VC
from zdr_amd import Camera, Scene, float3, image_pyramid_forward, texel_gather_dview
from zdr_amd import _native as N
from zdr_amd.mip import pyramid_pixels

pytestmark = pytest.mark.gpu


def test_both_camera_gradient_calls_can_be_captured_without_a_warm_up_and_replayed():
    name = "cbox_64x64_standard"
    res = VC.res_of(name)
    fov, o, t, up = PC.CAMERAS["standard"]
    cam = Camera(fov=fov, origin=float3(*o), target=float3(*t), up=float3(*up))
    scene = Scene(LC.CASES[PC.CASES[name][0]][0](), integrator="direct", accel="bvh")       # a fresh handle: nothing ran on it before
    pts = torch.from_numpy(PC.points(name)).cuda()
    view_in = scene.texel_view_forward(pts, res, camera=cam)
    view, image, g = torch.zeros_like(view_in), torch.zeros(res[1], res[0], 4, device="cuda"), torch.zeros(64, 64, 4, device="cuda")
    pyramid = torch.zeros(pyramid_pixels(res), 4, device="cuda")
    d_view, d_bil, d_mip, d_cam = torch.zeros(64, 64, 8, device="cuda"), torch.zeros(64, 64, 8, device="cuda"), torch.zeros(64, 64, 8, device="cuda"), torch.zeros(10, device="cuda")
    ws = torch.empty(N.lib().zdr_texel_view_backward_workspace_bytes(64, 64), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        texel_gather_dview(image, view, g, out=d_bil)
        texel_gather_dview(image, view, g, filter="mip", pyramid=pyramid, footprint=4.0, out=d_mip)
        scene.texel_view_backward(pts, d_view, res, camera=cam, out=d_cam, workspace=ws)
    view.copy_(view_in); image.copy_(torch.from_numpy(VC.image("noise", res))); g.copy_(torch.from_numpy(VC.d_color(name)))
    image_pyramid_forward(image, out=pyramid)
    d_view.copy_(torch.from_numpy(VC.d_view((64, 64), seed=6)))
    d_bil.fill_(7.0); d_mip.fill_(7.0); d_cam.fill_(7.0); ws.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    got = d_bil.clone(), d_mip.clone(), d_cam.clone()
    assert torch.equal(got[0].view(torch.int32), texel_gather_dview(image, view, g).view(torch.int32)) and float(got[0].abs().sum()) > 0
    assert torch.equal(got[1].view(torch.int32), texel_gather_dview(image, view, g, filter="mip", footprint=4.0).view(torch.int32)) and float(got[1][..., 6].abs().sum()) > 0
    assert torch.equal(got[2].view(torch.int32), scene.texel_view_backward(pts, d_view, res, camera=cam).view(torch.int32)) and float(got[2].abs().sum()) > 0
    del graph
    scene.check()
