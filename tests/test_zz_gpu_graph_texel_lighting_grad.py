"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): zdr_scene_texel_lighting_backward captured in a HIP graph with
torch.cuda.graph and replayed.  The call never allocates and never synchronises, its grid does not depend on the list it compacts on the
device, the scene is only read and the workspace — the emission accumulator included — is the caller's, so it is captured WITHOUT an
eager call before, on a handle of its own, with the workspace full of garbage.  The sums use float atomics: a replay is compared with the
float64 reference within the case's bar, like an eager call, not bit for bit.  The graph is a straight line of four kernels, no parallel
branches."""
import numpy as np
import pytest
import torch

import texel_lighting_grad_cases as GC
from test_gpu_texel_lighting_grad import check_parity, new_scene
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_the_adjoint_can_be_captured_without_a_warm_up_and_replayed(accel):
    name = "env_panel_lit_16"
    scene = new_scene(name, accel)                                  # a handle of its own: nothing was launched on it before
    pts, g = torch.from_numpy(GC.points(name)).cuda(), torch.from_numpy(GC.cotangent(name)).cuda()
    H, W = pts.shape[:2]
    d_e = torch.zeros(scene.inst_count, 3, device="cuda")
    d_env = torch.zeros(tuple(scene._envmap[0].shape), device="cuda")
    ws = torch.full((N.lib().zdr_texel_lighting_backward_workspace_bytes(scene._handle, H, W),), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scene.texel_lighting_backward(pts, g, spp=4, seed=GC.SEED, d_emission=d_e, d_env=d_env, workspace=ws)
    eager_e, eager_env = torch.zeros_like(d_e), torch.zeros_like(d_env)
    scene.texel_lighting_backward(pts, g, spp=4, seed=GC.SEED, d_emission=eager_e, d_env=eager_env)
    torch.cuda.synchronize()
    check_parity(name, {"emission": eager_e.cpu().numpy(), "env": eager_env.cpu().numpy()}, GC.reference(name), f"{name} {accel} eager")
    for fill in (0x11, 0xFF):
        d_e.zero_(); d_env.zero_(); ws.fill_(fill)                  # whatever the workspace held: the call clears what it reads
        graph.replay()
        torch.cuda.synchronize()
        got = {"emission": d_e.cpu().numpy(), "env": d_env.cpu().numpy()}
        check_parity(name, got, GC.reference(name), f"{name} {accel} replay after {fill:#x}")
        for target, eager in (("emission", eager_e), ("env", eager_env)):
            diff = np.abs(got[target].astype(np.float64) - eager.cpu().numpy())[..., :3]
            assert (diff <= GC.bar(name, target)).all(), target
    del graph
    scene.check()
