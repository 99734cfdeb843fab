"""Gradient of renders w.r.t. the environment map (zdr_render_backward_env, Scene.render(..., envmap=)).

The estimator is linear in the map once the importance-sampling tables are held fixed, so for one seed the forward pass is
I(E) = A E + b exactly, and the backward pass must return A^T g: <g, I(E + D) - I(E)> = <A^T g, D> for any cotangent g and any
direction D, with no Monte Carlo noise at all (the same camera samples, paths and decisions on both sides)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import cbox_models, fd_material_np
from gpu_util import make_scene
from test_envmap import sun_sky
from zdr_amd import _native as N
from zdr_amd import envmap

W, SPP, SEED = 32, 16, 5


def sky(scale=0.1):
    """sun_sky of test_envmap.py scaled so that no sample comes near the per-sample clamp of 1e5"""
    return sun_sky() * np.float32(scale)


def scene_with_env(integrator, accel="auto", sampler="cmj", models=None, img=None):
    s = make_scene(integrator, accel=accel, models=models)
    if sampler == "pmj02bn":
        from zdr_amd import pmj02bn_tables as T
        s.sampler = "pmj02bn"
        s.set_pmj02bn_tables(T.pmj02_sets(n_sets=5, n_samples=256, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2))
    s.add_envmap(sky() if img is None else img)
    return s


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


class Case:
    """One scene and its materials: forward(E) renders with map E (seed + 1, the backward's samples), backward(g, E) returns
    (d_materials, d_env) of the same samples."""

    def __init__(self, scene, mats=None, slots=None):
        self.s = scene
        self.mats = mats if mats is not None else [cuda(fd_material_np(64, 0))]
        self.slots = slots
        if slots is not None:
            scene.material_slots = slots

    def forward(self, E):
        self.s.set_envmap_texture(E)
        if self.slots is None:
            img = self.s.render_forward(self.mats[0], (W, W), SPP, SEED + 1)
        else:
            img = self.s.render_forward_materials(self.mats, (W, W), SPP, SEED + 1)
        return img.double().cpu().numpy()

    def backward(self, g, E, with_env=True):
        self.s.set_envmap_texture(E)
        d_env = torch.zeros_like(E) if with_env else None
        dm = [torch.zeros_like(m) for m in self.mats]
        if self.slots is None:
            self.s.render_backward(g, dm[0], self.mats[0], (W, W), SPP, SEED, d_env=d_env)
        else:
            self.s.render_backward_materials(g, dm, self.mats, (W, W), SPP, SEED, d_env=d_env)
        torch.cuda.synchronize()
        return dm, d_env


def adjoint_identity(case, E, D, seed=0):
    """(<g, I(E + D) - I(E)>, <d_env, D>) in float64"""
    g = np.random.default_rng(seed).normal(size=(W, W, 4)).astype(np.float32)
    g[..., 3] = 0.0
    dI = case.forward(E + D) - case.forward(E)
    lhs = float((g.astype(np.float64) * dI).sum())
    _, d_env = case.backward(cuda(g), E)
    rhs = float((d_env.double() * D.double()).sum())
    return lhs, rhs, d_env


def direction(E, seed=1):
    D = torch.rand(E.shape, generator=torch.Generator().manual_seed(seed)).cuda() * 0.05
    D[..., 3] = 0.0
    return D


CASES = [("path", "brute", "cmj"), ("path", "bvh", "cmj"), ("direct", "brute", "cmj"), ("direct", "bvh", "cmj"), ("path", "brute", "pmj02bn")]


@pytest.mark.gpu
@pytest.mark.parametrize("integrator,accel,sampler", CASES)
def test_adjoint_identity(integrator, accel, sampler):
    s = scene_with_env(integrator, accel, sampler)
    E = cuda(envmap.prepare_image(sky()))
    lhs, rhs, d_env = adjoint_identity(Case(s), E, direction(E))
    s.check()
    assert abs(lhs) > 1e-3, lhs                                 # the map reaches the image
    assert float(d_env[..., 3].abs().max()) == 0.0              # alpha is not read
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_adjoint_identity_on_the_environment_only_scene(integrator):
    """test_envmap.py's scene without a mesh light: most camera rays miss and every light sample goes to the environment"""
    s = scene_with_env(integrator, models=[(cbox_models()[0][0], None, 0.0)])
    E = cuda(envmap.prepare_image(sky()))
    lhs, rhs, _ = adjoint_identity(Case(s), E, direction(E))
    s.check()
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)


@pytest.mark.gpu
def test_adjoint_identity_with_several_materials():
    from test_gpu_materials import split_arrays
    s = make_scene("path", arrays=split_arrays())                # cboxuv.obj in two instances, the light third
    s.add_envmap(sky())
    mats = [cuda(fd_material_np(64, 0)), cuda(fd_material_np(16, 1))]
    case = Case(s, mats, [0, 1, None])
    E = cuda(envmap.prepare_image(sky()))
    lhs, rhs, _ = adjoint_identity(case, E, direction(E))
    s.check()
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("integrator,accel", [("path", "bvh"), ("path", "brute"), ("direct", "brute")])
def test_adjoint_identity_where_the_map_is_zero_but_the_tables_sample(integrator, accel):
    """Tables of the full map (every texel has a positive pdf), rendered with the 8 x 8 texels that matter most to this view set
    to zero, D on those texels only: a light sample that lands there carries no radiance now, yet its gradient does not vanish —
    the BVH kernels must trace its shadow ray all the same, and the direct kernel must weigh a BSDF sample that escapes there."""
    s = scene_with_env(integrator, accel)
    case = Case(s)
    E = cuda(envmap.prepare_image(sky()))
    g = cuda(np.random.default_rng(0).normal(size=(W, W, 4)))
    _, d_env = case.backward(g, E)
    heat = torch.nn.functional.avg_pool2d(d_env[..., :3].abs().sum(-1)[None, None], 8, stride=1)[0, 0]
    y, x = divmod(int(heat.argmax()), heat.shape[1])
    E[y:y + 8, x:x + 8, :3] = 0.0
    D = torch.zeros_like(E)
    D[y:y + 8, x:x + 8, :3] = 1.0
    lhs, rhs, _ = adjoint_identity(case, E, D)
    s.check()
    assert abs(lhs) > 1e-3, lhs
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "brute")])
def test_material_gradient_is_that_of_the_plain_call(integrator, accel):
    s = scene_with_env(integrator, accel)
    case = Case(s)
    E = cuda(envmap.prepare_image(sky()))
    g = cuda(np.random.default_rng(3).normal(size=(W, W, 4)))
    (dm_env,), d_env = case.backward(g, E)
    (dm,), none = case.backward(g, E, with_env=False)
    assert none is None and float(d_env.abs().sum()) > 0.0
    a, b = dm_env.double(), dm.double()
    assert float((a - b).norm() / b.norm()) <= 1e-6


@pytest.mark.gpu
def test_autograd_returns_the_gradient_in_the_callers_shape():
    s = scene_with_env("path")
    img = sky()                                                 # (32, 64, 3)
    m = cuda(fd_material_np(64, 0)).requires_grad_()
    env = cuda(img).requires_grad_()
    g = cuda(np.random.default_rng(4).normal(size=(W, W, 4)))
    out = s.render(m, res=(W, W), spp=SPP, seed=SEED, envmap=env)
    (out * g).sum().backward()
    assert env.grad.shape == img.shape
    # the low-level call on the same samples, folded by hand: square rows 2i and 2i + 1 are row i, alpha is dropped
    d_env = torch.zeros((64, 64, 4), device="cuda")
    d_m = torch.zeros_like(m)
    s.render_backward(g, d_m, m.detach(), (W, W), SPP, SEED, d_env=d_env)
    folded = d_env[0::2, :, :3] + d_env[1::2, :, :3]
    torch.testing.assert_close(env.grad, folded, rtol=1e-5, atol=1e-6 * float(folded.abs().max()))
    torch.testing.assert_close(m.grad, d_m, rtol=1e-5, atol=1e-6 * float(d_m.abs().max()))
    # render() without envmap= is unchanged: the same image as a scene that was only given the map by add_envmap
    plain = scene_with_env("path", img=img)
    a = plain.render(m.detach(), res=(W, W), spp=SPP, seed=SEED)
    assert torch.equal(a, out.detach())
    assert torch.equal(s.render(m.detach(), res=(W, W), spp=SPP, seed=SEED), a)


@pytest.mark.gpu
def test_envmap_argument_is_checked():
    s = make_scene("path")
    m = cuda(fd_material_np(64, 0))
    with pytest.raises(ValueError, match="add_envmap"):
        s.render(m, res=(W, W), spp=4, envmap=cuda(sky()))
    s.add_envmap(sky())
    with pytest.raises(ValueError, match="size"):
        s.render(m, res=(W, W), spp=4, envmap=cuda(sky()[:16, :32]))
    s.material_slots = [0, None]
    with pytest.raises(ValueError, match="at most 15"):               # refused before anything is rendered
        s.render([m] * 16, res=(W, W), spp=4, envmap=cuda(sky()))


@pytest.mark.gpu
def test_the_texture_setter_takes_any_contiguous_view_and_the_c_abi_refuses_a_misaligned_one():
    s = scene_with_env("path")
    m = cuda(fd_material_np(64, 0))
    E = cuda(envmap.prepare_image(sky()))
    buf = torch.zeros(E.numel() + 1, device="cuda")
    view = buf[1:].view(E.shape)                                  # contiguous, 4 bytes past a 16-byte boundary
    view.copy_(E)
    assert view.data_ptr() % 16 == 4
    assert N.lib().zdr_scene_set_envmap_texture(s._handle, view.data_ptr(), s._stream()) == -1
    s.set_envmap_texture(view)
    a = s.render_forward(m, (W, W), SPP, SEED)
    s.set_envmap_texture(E)
    assert torch.equal(a, s.render_forward(m, (W, W), SPP, SEED))


@pytest.mark.gpu
def test_collocated_leaves_d_env_alone_and_a_null_d_env_is_the_plain_call():
    L = N.lib()
    s = scene_with_env("collocated")
    m = cuda(fd_material_np(64, 0))
    g = cuda(np.random.default_rng(5).normal(size=(W, W, 4)))
    d_env = torch.zeros((64, 64, 4), device="cuda")
    a, b = torch.zeros_like(m), torch.zeros_like(m)
    s.render_backward(g, a, m, (W, W), SPP, SEED, d_env=d_env)
    s.render_backward(g, b, m, (W, W), SPP, SEED)
    torch.cuda.synchronize()
    assert float(d_env.abs().max()) == 0.0
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    for integrator in ("path", "direct"):
        s = scene_with_env(integrator)
        a, b = torch.zeros_like(m), torch.zeros_like(m)
        p = s._params((W, W), SPP, SEED + 1, m.shape[:2])
        N.check(L.zdr_render_backward_env(s._handle, C.byref(p), g.data_ptr(), m.data_ptr(), a.data_ptr(), None, s._stream()))
        s.render_backward(g, b, m, (W, W), SPP, SEED)
        torch.cuda.synchronize()
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    # no map: the texture setter and the env-gradient call refuse
    for integrator in ("path", "collocated"):
        bare = make_scene(integrator)
        assert L.zdr_scene_set_envmap_texture(bare._handle, d_env.data_ptr(), bare._stream()) == -1
        p = bare._params((W, W), SPP, SEED + 1, m.shape[:2])
        assert L.zdr_render_backward_env(bare._handle, C.byref(p), g.data_ptr(), m.data_ptr(), a.data_ptr(), d_env.data_ptr(), bare._stream()) == -1
