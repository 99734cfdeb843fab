"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): the feature buffers of a two-material scene and their
adjoint (zdr_render_aovs, zdr_render_aovs_backward) captured in a HIP graph with torch.cuda.graph on one stream and replayed.  The
calls only enqueue, zero their staging cells by a kernel and carry the material table in the kernel arguments, so the replay gives
what the eager calls gave.  A runtime that refuses to capture is a skip."""
import numpy as np
import pytest
import torch

from conftest import cbox_models, fd_material_np
from gpu_util import make_scene
from zdr_amd import geometry

pytestmark = pytest.mark.gpu


def _skip_unless_ours(e):
    from zdr_amd._native import ZdrError
    if isinstance(e, ZdrError):
        raise e
    pytest.skip(f"stream capture unavailable: {e}")


def test_feature_buffers_can_be_captured_and_replayed():
    a = geometry.assemble(cbox_models())
    b = a.inst_tri_begin
    n = int(b[1])
    arrays = geometry.from_arrays(a.verts, a.tris, [0, n // 2, n, int(b[2])], np.concatenate([a.inst_xform[:1], a.inst_xform]),
                                  np.concatenate([a.inst_emission[:1], a.inst_emission]))
    scene = make_scene("path", arrays=arrays)
    scene.material_slots = [0, 1, None]
    mats = [torch.from_numpy(fd_material_np(64, 0)).cuda(), torch.from_numpy(fd_material_np(16, 1)).cuda()]
    dims = [(64, 64), (16, 16)]
    packed = torch.cat([m.reshape(-1, 4) for m in mats])
    W, H, spp, seed = 64, 48, 16, 9
    cot = torch.from_numpy(np.random.default_rng(0).normal(size=(H, W, 16)).astype(np.float32)).cuda()
    buf = torch.zeros((H, W, 16), device="cuda"); g = torch.zeros_like(packed)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                   # eager calls size the handle's workspaces first (include/zdr.h)
        scene.render_aovs_forward(packed, (W, H), spp, seed, dims=dims, out=buf)
        scene.render_aovs_backward(cot, g, packed, (W, H), spp, seed, dims=dims)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ref_buf, ref_g = buf.clone(), g.clone()
    assert ref_g[:64 * 64].abs().sum() > 0 and ref_g[64 * 64:].abs().sum() > 0   # both materials receive their gradient
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            scene.render_aovs_forward(packed, (W, H), spp, seed, dims=dims, out=buf)
            g.zero_()
            scene.render_aovs_backward(cot, g, packed, (W, H), spp, seed, dims=dims)
    except RuntimeError as e:
        _skip_unless_ours(e)
    for _ in range(2):
        buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, ref_buf)
        torch.testing.assert_close(g, ref_g, rtol=1e-4, atol=1e-6 * float(ref_g.abs().max()))
    del graph
    scene.check()
