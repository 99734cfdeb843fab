"""-m gpu, run after the other GPU files (see tests/test_zz_gpu_graph.py): the texture setter, the rebuild of the importance-sampling
tables and a forward (zdr_scene_set_envmap_texture, zdr_scene_update_envmap_sampling, zdr_render_forward) captured once in a HIP graph
after an eager warm-up and replayed after the scene's texture was set to another map outside the graph: the replay uploads map B
again, rebuilds ITS tables in the buffers the scene already had and renders with them.  A first rebuild made under capture is
refused: its workspace cannot be allocated then.  A runtime that refuses to capture is a skip."""
import numpy as np
import pytest
import torch

import envmap_tables as T
from conftest import fd_material_np
from zdr_amd import envmap as E
from zdr_amd._native import ZdrError

pytestmark = pytest.mark.gpu


def _skip_unless_ours(e):
    if isinstance(e, ZdrError):
        raise e
    pytest.skip(f"stream capture unavailable: {e}")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def test_setter_rebuild_and_forward_can_be_captured_and_replayed():
    A, B = cuda(E.prepare_image(T.sun_map((32, 64), T.SUN_A))), cuda(E.prepare_image(T.sun_map((32, 64), T.SUN_B)))
    scene = T.set_map_with_uniform_tables(T.env_only_scene("path"), T.sun_map((32, 64), T.SUN_A))
    m = cuda(fd_material_np(64, 0))
    Wd, Hd, spp, seed = 64, 48, 16, 9
    img = torch.zeros((Hd, Wd, 4), device="cuda")
    src = B.clone()                                               # the graph reads this tensor at replay time

    def step():
        scene.update_envmap_sampling(src, on_device=True)          # set_envmap_texture + the four table kernels
        scene.render_forward(m, (Wd, Hd), spp, seed, out=img)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                     # the warm call: workspaces of the rebuild and of the render
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    want_tables = scene.envmap_sampling_tables()
    want_img = img.clone()
    bytes_warm = scene.info()["device_bytes"]
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph):
            step()
    except RuntimeError as e:
        _skip_unless_ours(e)
    # outside the graph the map becomes A, tables and all
    scene.update_envmap_sampling(A, on_device=True)
    other = scene.render_forward(m, (Wd, Hd), spp, seed).clone()
    assert not torch.equal(other, want_img)
    assert not np.array_equal(scene.envmap_sampling_tables()[2], want_tables[2])
    img.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, ref in zip(scene.envmap_sampling_tables(), want_tables):
        assert np.array_equal(got, ref)
    assert torch.equal(img, want_img)
    # the graph reads its source in place: with A in it, the replay is the eager rebuild from A
    src.copy_(A)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(img, other)
    assert scene.info()["device_bytes"] == bytes_warm
    del graph
    scene.check()


def test_a_first_rebuild_under_capture_is_refused():
    scene = T.set_map_with_uniform_tables(T.env_only_scene("path"), T.sun_map((32, 64), T.SUN_A))
    before = scene.info()["device_bytes"]
    graph = torch.cuda.CUDAGraph()
    refused, pad = None, torch.zeros(4, device="cuda")
    try:
        with torch.cuda.graph(graph):
            pad.add_(1.0)                                          # (the graph is not empty)
            try:
                scene.update_envmap_sampling(None, on_device=True)
            except ZdrError as e:                                  # (caught inside: the capture ends in order)
                refused = e
    except RuntimeError as e:
        _skip_unless_ours(e)
    assert refused is not None and "before capturing" in str(refused) and "error -1" in str(refused), refused
    assert scene.info()["device_bytes"] == before
    del graph
    scene.update_envmap_sampling(None, on_device=True)             # eager: fine
    T.check_tables(*scene.envmap_sampling_tables(), bar=T.Q_BAR)
    scene.check()
