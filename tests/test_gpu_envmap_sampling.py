"""The environment map's importance-sampling tables rebuilt on the GPU (zdr_scene_update_envmap_sampling;
Scene.update_envmap_sampling(..., on_device=True), render(..., update_sampling=True)): the tables are valid (tests/envmap_tables.py,
check_tables, with bars measured on the host), agree with the host's build_tables, the kernels sample correctly from them (the oracle
given the downloaded tables), the rebuild is in place and reproducible, and it does what it is for: a map that moved is sampled
with less variance after it."""
import numpy as np
import pytest
import torch

import envmap_tables as T
import oracle
from conftest import cbox_models, fd_material_np
from gpu_util import Flips, assert_grad_parity, assert_image_parity, make_scene, oracle_params
from test_envmap import sun_sky
from zdr_amd import _native as N
from zdr_amd import envmap as E
from zdr_amd import geometry

pytestmark = pytest.mark.gpu
W, H = T.W, T.H
MAPS = T.all_maps()
IDS = [f"{f}-{s[0]}x{s[1]}" for f, s in MAPS]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


_SCENES = {}


def scene_of(shape):
    """one environment-only scene per texture size, given its first map with tables that the device has to replace"""
    if shape not in _SCENES:
        _SCENES[shape] = T.set_map_with_uniform_tables(T.env_only_scene("path"), np.zeros(shape + (3,), np.float32))
    return _SCENES[shape]


def device_tables(img, comp):
    s = scene_of(img.shape[:2])
    s.update_envmap_sampling(cuda(img), compensate_mis=comp, on_device=True)
    return s.envmap_sampling_tables()


@pytest.mark.parametrize("family,shape", MAPS, ids=IDS)
def test_device_tables_are_valid(family, shape):
    img = T.make_map(family, shape)
    for comp in (True, False):
        prob, alias, pdf = device_tables(img, comp)
        q = T.check_tables(prob, alias, pdf, bar=T.Q_BAR)
        print(f"[envmap sampling] {family} {shape} compensate_mis {int(comp)}: table residual {q:.3e} (bar {T.Q_BAR:.3e}), "
              f"pdf == 0: {float((pdf == 0).mean()):.3f}, max pdf {float(pdf.max()):.4g}")
        if family == "black":                                        # every total 0: everything uniform
            assert (pdf == 1.0).all() and (prob == 1.0).all() and np.array_equal(alias, T.uniform_tables()[1])
        if family in ("sun_sky", "black_rows") and comp:
            assert float((pdf == 0).mean()) > 0.5                    # the exact zeros of check_tables are exercised
    scene_of(shape).check()


@pytest.mark.parametrize("family,shape", [m for m in MAPS if m[0] != "constant"], ids=[i for i in IDS if not i.startswith("constant")])
def test_device_pdf_agrees_with_the_host_pipeline(family, shape):
    img = T.make_map(family, shape)
    for comp in (True, False):
        host = T.host_tables(img, comp)[2]
        pdf = device_tables(img, comp)[2]
        a = T.agreement(pdf, host)
        print(f"[envmap sampling] {family} {shape} compensate_mis {int(comp)}: max |pdf_device - pdf_host| / max(pdf_host) = {a:.3e} "
              f"(bar {T.AGREE_BAR:.3e}; host vs float64 {T.agreement(T.pdf64(img, comp), host):.3e}); "
              f"zero on one side only: {int(((pdf == 0) != (host == 0)).sum())} texels")
        assert a <= T.AGREE_BAR, (family, shape, comp, a)


def _oracle_pair(arrays, I, tables):
    S = oracle.OracleScene.from_arrays(arrays); Sf = oracle.OracleScene.from_arrays(arrays, variant="fma")
    S.set_envmap(I, *tables); Sf.set_envmap(I, *tables)
    return S, Sf


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("which", ["env_only", "cbox"])
def test_the_kernels_sample_correctly_from_device_built_tables(which, integrator):
    """forward, and backward with d_env, against the oracle given the DOWNLOADED tables"""
    models = [(cbox_models()[0][0], None, 0.0)] if which == "env_only" else cbox_models()
    scene = T.set_map_with_uniform_tables(make_scene(integrator, models=models), sun_sky())
    scene.update_envmap_sampling(None, on_device=True)
    tables = scene.envmap_sampling_tables()
    T.check_tables(*tables, bar=T.Q_BAR)
    assert scene._envmap[1] is tables[0] and float((tables[2] == 0).mean()) > 0.5          # refreshed; not the uniform tables any more
    I = scene._envmap[0]
    S, Sf = _oracle_pair(geometry.assemble(models), I, tables)
    mat = fd_material_np(64, 1)
    Wd, spp, seed = 32, 16, 3
    m = cuda(mat)
    img = scene.render_forward(m, (Wd, Wd), spp, seed).cpu().numpy()
    p = oracle_params(scene, Wd, Wd, spp, seed, mat.shape[:2])
    ref = S.render_forward(p, mat)
    assert ref[..., :3].mean() > 0.01
    what = f"device tables, {which} {integrator}"

    def flips(sd, cot=None, tag=""):                                 # (path traces exist for the path integrator only)
        return Flips(scene, S, Sf, mat, (Wd, Wd), spp, sd, cot=cot, what=what + tag) if integrator == "path" else None

    assert_image_parity(img[..., :3], ref[..., :3], what + " forward", floor=Sf.render_forward(p, mat)[..., :3], flips=flips(seed, tag=" forward"))
    g = np.ones((Wd, Wd, 4), np.float32)
    d_m, d_env = torch.zeros_like(m), torch.zeros((I.shape[0], I.shape[1], 4), device="cuda")
    scene.render_backward(cuda(g), d_m, m, (Wd, Wd), spp, seed, d_env=d_env)
    pb = oracle_params(scene, Wd, Wd, spp, seed + 1, mat.shape[:2])
    assert_grad_parity(d_m.cpu().numpy(), S.render_backward(pb, g, mat), what + " backward", floor=Sf.render_backward(pb, g, mat),
                       flips=flips(seed + 1, cot=g, tag=" backward"))
    assert float(d_env[..., :3].abs().sum()) > 0.0 and float(d_env[..., 3].abs().max()) == 0.0
    # the map's gradient with these tables: the estimator is linear in the map, so <g, I(E + D) - I(E)> = <d_env, D> without noise
    Et = cuda(I)
    D = torch.rand(Et.shape, generator=torch.Generator().manual_seed(1)).cuda() * 0.05
    D[..., 3] = 0.0
    scene.set_envmap_texture(Et + D)
    hi = scene.render_forward(m, (Wd, Wd), spp, seed + 1).double()
    scene.set_envmap_texture(Et)
    lo = scene.render_forward(m, (Wd, Wd), spp, seed + 1).double()
    lhs, rhs = float((hi - lo)[..., :3].sum()), float((d_env.double() * D.double()).sum())
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    scene.check()


def _table_bytes(scene):
    return tuple(t.tobytes() for t in scene.envmap_sampling_tables())


def test_the_rebuild_is_in_place_and_reproducible():
    img = T.make_map("sun_sky", (24, 48))
    scene = T.set_map_with_uniform_tables(T.env_only_scene("path"), img)
    before = scene.info()["device_bytes"]
    scene.update_envmap_sampling(None, on_device=True)
    first = _table_bytes(scene)
    after = scene.info()["device_bytes"]
    assert 0 < after - before <= 600 * 1024                         # the workspace of the first call, about 0.5 MiB
    scene.update_envmap_sampling(None, on_device=True)
    assert _table_bytes(scene) == first                              # two rebuilds, identical bytes (no float atomics)
    scene.update_envmap_sampling(cuda(img), compensate_mis=False, on_device=True)
    assert _table_bytes(scene) != first
    scene.update_envmap_sampling(cuda(T.make_map("random_hdr", (24, 48))), on_device=True)
    scene.update_envmap_sampling(cuda(img), on_device=True)
    assert _table_bytes(scene) == first
    assert scene.info()["device_bytes"] == after                     # nothing allocated once warm
    # garbage in the tables: valid but wrong ones through the C-ABI, then a rebuild
    I = scene._envmap[0]
    prob, alias, pdf = T.uniform_tables()
    N.check(N.lib().zdr_scene_set_envmap(scene._handle, I.ctypes.data, I.shape[0], I.shape[1], prob.ctypes.data, alias.ctypes.data, pdf.ctypes.data, W, H))
    assert _table_bytes(scene) == tuple(t.tobytes() for t in (prob, alias, pdf))
    scene.update_envmap_sampling(None, on_device=True)
    assert _table_bytes(scene) == first
    scene.check()


def test_refusals_and_the_default_path():
    m = cuda(fd_material_np(64, 0))
    bare = make_scene("path")
    with pytest.raises(ValueError, match="add_envmap"):
        bare.update_envmap_sampling(None, on_device=True)
    with pytest.raises(ValueError, match="add_envmap"):
        bare.update_envmap_sampling(cuda(sun_sky()), on_device=True)
    with pytest.raises(ValueError, match="add_envmap"):
        bare.envmap_sampling_tables()
    assert N.lib().zdr_scene_update_envmap_sampling(bare._handle, 1, bare._stream()) == -1
    assert b"no environment map" in N.lib().zdr_last_error()
    buf = np.zeros(H + H * W, np.float32)
    assert N.lib().zdr_scene_get_envmap_sampling(bare._handle, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, bare._stream()) == -1
    img = T.make_map("sun_sky", (16, 32))
    scene = T.set_map_with_uniform_tables(bare, img)
    with pytest.raises(ValueError, match="size"):
        scene.update_envmap_sampling(cuda(sun_sky()), on_device=True)
    with pytest.raises(ValueError, match="float32 tensor on"):
        scene.update_envmap_sampling(torch.from_numpy(img), on_device=True)
    with pytest.raises(ValueError, match="float32 tensor on"):
        scene.update_envmap_sampling(img, on_device=True)
    with pytest.raises(ValueError, match="update_sampling"):
        scene.render(m, res=(16, 16), spp=1, update_sampling=True)
    assert _table_bytes(scene) == tuple(t.tobytes() for t in T.uniform_tables())     # nothing was rebuilt by a refused call
    # the default path: host-built tables, bit for bit those of build_tables, as before
    scene.update_envmap_sampling(torch.from_numpy(img), compensate_mis=False)
    want = T.host_tables(img, False)
    for got, ref, kept in zip(scene.envmap_sampling_tables(), want, scene._envmap[1:]):
        assert got.dtype == ref.dtype and np.array_equal(got, ref) and np.array_equal(kept, ref)
    with pytest.raises(ValueError, match="needs a map"):
        scene.update_envmap_sampling(None)


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_a_map_that_moved_is_sampled_with_less_variance_after_the_rebuild(integrator):
    """Tables of map A (the sun upper left of the box's opening), then the map becomes B (the sun upper right).  With A's tables the
    light samples go where the sun was, and B's sun is found by BSDF sampling alone; after the rebuild they go to the sun.  On the CPU,
    oracle and host tables, 64 x 64 at spp 4 against spp 1024, seeds 1 - 3: RMSE 9.95 / 9.47 / 9.92 stale against 0.478 / 0.497 / 0.507
    fresh (path, ratio 0.05), 8.38 / 7.92 / 8.81 against 0.197 / 0.205 / 0.198 (direct, ratio 0.02): the condition below is far from
    noise.  On an MI355X with device-built tables: 9.95 / 9.47 / 9.92 against 0.478 / 0.497 / 0.509 (path), 8.38 / 7.92 / 8.81 against
    0.197 / 0.205 / 0.198 (direct) (profiles/envmap_sampling_cost.txt)."""
    A, B = T.sun_map((32, 64), T.SUN_A), T.sun_map((32, 64), T.SUN_B)
    scene = T.set_map_with_uniform_tables(T.env_only_scene(integrator), A)
    m = cuda(fd_material_np(64, 0))
    Wd = 64
    scene.update_envmap_sampling(None, on_device=True)               # tables of A
    scene.set_envmap_texture(cuda(E.prepare_image(B)))
    stale = [scene.render_forward(m, (Wd, Wd), 4, seed)[..., :3].double() for seed in (1, 2, 3)]
    scene.update_envmap_sampling(None, on_device=True)               # tables of B
    fresh = [scene.render_forward(m, (Wd, Wd), 4, seed)[..., :3].double() for seed in (1, 2, 3)]
    ref = scene.render_forward(m, (Wd, Wd), 1024, 100)[..., :3].double()
    assert float(ref.mean()) > 0.1
    for seed, s, f in zip((1, 2, 3), stale, fresh):
        rs, rf = float(((s - ref) ** 2).mean().sqrt()), float(((f - ref) ** 2).mean().sqrt())
        print(f"[envmap sampling] {integrator} 64 x 64 spp 4 seed {seed}: RMSE against spp 1024 with stale tables {rs:.4g}, after the rebuild {rf:.4g}, ratio {rf / rs:.3f}")
        assert rf < rs, (integrator, seed, rs, rf)
    scene.check()


def test_render_with_update_sampling_is_the_explicit_rebuild_followed_by_render():
    img, other = sun_sky() * np.float32(0.1), T.make_map("random_hdr", (32, 64))
    g = cuda(np.random.default_rng(4).normal(size=(32, 32, 4)))
    m = cuda(fd_material_np(64, 0))

    def run(update):
        scene = T.set_map_with_uniform_tables(make_scene("path"), other)
        scene.update_envmap_sampling(None, on_device=True)           # tables of another map first
        env = cuda(img).requires_grad_()
        mm = m.clone().requires_grad_()
        if not update:
            scene.update_envmap_sampling(env.detach(), on_device=True)
        out = scene.render(mm, res=(32, 32), spp=16, seed=5, envmap=env, update_sampling=update)
        (out * g).sum().backward()
        return out.detach(), env.grad, mm.grad, scene.envmap_sampling_tables(), scene

    a, b = run(True), run(False)
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(x, y)
    T.check_tables(*a[3], bar=T.Q_BAR)
    assert torch.equal(a[0], b[0])
    assert a[1].shape == img.shape and float(a[1].abs().sum()) > 0.0
    torch.testing.assert_close(a[1], b[1], rtol=1e-4, atol=1e-6 * float(b[1].abs().max()))     # float atomics: arrival order
    torch.testing.assert_close(a[2], b[2], rtol=1e-4, atol=1e-6 * float(b[2].abs().max()))
    # without the keyword the tables stay what they were
    scene = a[4]
    scene.render(m, res=(32, 32), spp=1, seed=5, envmap=cuda(other))
    for x, y in zip(scene.envmap_sampling_tables(), a[3]):
        assert np.array_equal(x, y)
    scene.check()
