"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): the emission setter, a forward and the emission-gradient
backward (zdr_scene_set_emission_values, zdr_render_forward, zdr_render_backward_emission) captured once in a HIP graph after an
eager warm-up and replayed after the device tensor of the emissions was changed in place: the setter is a kernel that reads the
tensor at replay time, so the replay renders and differentiates with the new values.  A runtime that refuses to capture is a skip."""
import pytest
import torch

from conftest import fd_material_np
from gpu_util import make_scene, multi_light_arrays

pytestmark = pytest.mark.gpu


def _skip_unless_ours(e):
    from zdr_amd._native import ZdrError
    if isinstance(e, ZdrError):
        raise e
    pytest.skip(f"stream capture unavailable: {e}")


def test_setter_forward_and_emission_backward_can_be_captured_and_replayed():
    A = multi_light_arrays()
    scene = make_scene("path", arrays=A)
    m = torch.from_numpy(fd_material_np(64, 0)).cuda()
    E = torch.from_numpy(A.inst_emission).cuda()
    W, H, spp, seed = 64, 48, 16, 9
    cot = torch.ones((H, W, 4), device="cuda")
    img = torch.zeros((H, W, 4), device="cuda"); g = torch.zeros_like(m); d_e = torch.zeros_like(E)

    def step():
        scene._apply_emission_values(E)                          # (set_emission_values without the host-side bookkeeping)
        scene.render_forward(m, (W, H), spp, seed, out=img)
        scene.render_backward(cot, g, m, (W, H), spp, seed, d_emission=d_e)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                   # eager calls size the handle's workspaces first (include/zdr.h)
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            g.zero_(); d_e.zero_()
            step()
    except RuntimeError as e:
        _skip_unless_ours(e)
    for scale in (0.5, 3.0):
        E.copy_(torch.from_numpy(A.inst_emission).cuda() * torch.tensor([scale, 1.0, 2.0], device="cuda"))   # in place: the graph keeps its pointer
        img.zero_()
        graph.replay()
        torch.cuda.synchronize()
        got_img, got_g, got_e = img.clone(), g.clone(), d_e.clone()
        g.zero_(); d_e.zero_()
        step()                                                   # eager, the same values
        torch.cuda.synchronize()
        assert torch.equal(got_img, img)
        assert float(got_e.abs().sum()) > 0.0
        torch.testing.assert_close(got_e, d_e, rtol=1e-4, atol=1e-6 * float(d_e.abs().max()))
        torch.testing.assert_close(got_g, g, rtol=1e-4, atol=1e-6 * float(g.abs().max()))
    del graph
    scene.check()
