"""Gradient of renders w.r.t. the lights' emissions (zdr_render_backward_emission, Scene.render(..., emissions=)).

With the set of emitting models fixed nothing a path decides reads an emission value, so for one seed the forward pass is exactly
linear in the emissions, I(e) = A e (+ b with an environment map), and the backward pass must return A^T g.  That is checked
without any Monte Carlo noise: against the product's own forward (Euler's identity <g, I(e)> = <d_e, e>, and differences), and
light by light against the CPU oracle's forward as it stands (OracleScene.set_emissions + render_forward).

Cotangents are drawn from U(0.5, 1.5) with alpha 0; a backward call with seed s draws the samples of a forward with seed s + 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from conftest import cbox_material_np, fd_material_np
from gpu_util import make_scene, multi_light_arrays, oracle_params
from zdr_amd import Scene, geometry
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

W, SPP, SEED = 32, 16, 5


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b), 1e-30)


def cotangent(w, h, seed=0):
    g = np.random.default_rng(seed).uniform(0.5, 1.5, (h, w, 4)).astype(np.float32)
    g[..., 3] = 0.0
    return g


def with_sampler(s, sampler):
    if sampler == "pmj02bn":
        from zdr_amd import pmj02bn_tables as T
        s.sampler = "pmj02bn"
        s.set_pmj02bn_tables(T.pmj02_sets(n_sets=5, n_samples=256, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2))
    return s


def light_stage(integrator):
    from test_gpu_lightstage import CAMERA, models
    s = Scene(models(), integrator=integrator)
    s.camera = CAMERA
    return s


def build(scene_name, integrator, accel="auto", sampler="cmj"):
    if scene_name == "cbox":
        s = make_scene(integrator, accel=accel)
    elif scene_name == "lights3":
        s = make_scene(integrator, accel=accel, arrays=multi_light_arrays())
    else:
        s = light_stage(integrator)
    if accel != "auto":
        assert s.info()["accel"] == accel
    return with_sampler(s, sampler)


def emissions_of(scene):
    return cuda(scene._arrays.inst_emission)


class Case:
    """One scene and its materials: forward(e) renders with emission values e (seed + 1, the backward's samples), backward(g, e)
    returns (d_materials, d_emission) of the same samples."""

    def __init__(self, scene, mats=None, slots=None, w=W, spp=SPP, seed=SEED, h=None):
        self.s = scene
        self.mats = mats if mats is not None else [cuda(fd_material_np(64, 0))]
        self.slots = slots
        self.res, self.spp, self.seed = (w, w if h is None else h), spp, seed
        if slots is not None:
            scene.material_slots = slots

    def forward(self, e):
        self.s.set_emission_values(e)
        if self.slots is None:
            img = self.s.render_forward(self.mats[0], self.res, self.spp, self.seed + 1)
        else:
            img = self.s.render_forward_materials(self.mats, self.res, self.spp, self.seed + 1)
        return img.double().cpu().numpy()

    def backward(self, g, e, with_emission=True):
        self.s.set_emission_values(e)
        d_e = torch.zeros_like(e) if with_emission else None
        dm = [torch.zeros_like(m) for m in self.mats]
        if self.slots is None:
            self.s.render_backward(g, dm[0], self.mats[0], self.res, self.spp, self.seed, d_emission=d_e)
        else:
            self.s.render_backward_materials(g, dm, self.mats, self.res, self.spp, self.seed, d_emission=d_e)
        torch.cuda.synchronize()
        return dm, d_e


def euler(case, e, seed=0):
    """(<g, I(e)>, <d_e, e>) in float64, and d_e"""
    g = cotangent(case.res[0], case.res[1], seed)
    lhs = float((g.astype(np.float64) * case.forward(e)).sum())
    _, d_e = case.backward(cuda(g), e)
    rhs = float((d_e.double() * e.double()).sum())
    return lhs, rhs, d_e


def difference(case, e, D, seed=0):
    """(<g, I(e + D) - I(e)>, <d_e, D>) in float64, and d_e"""
    g = cotangent(case.res[0], case.res[1], seed)
    dI = case.forward(e + D) - case.forward(e)
    lhs = float((g.astype(np.float64) * dI).sum())
    _, d_e = case.backward(cuda(g), e)
    rhs = float((d_e.double() * D.double()).sum())
    return lhs, rhs, d_e


def rows_outside_the_light_list_are_zero(scene, d_e):
    dark = ~(scene._arrays.inst_emission > 0).any(axis=1)
    assert float(d_e[torch.from_numpy(dark).cuda()].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------- 1. Euler's identity
KERNELS = [("path", "brute", "cmj"), ("path", "bvh", "cmj"), ("direct", "brute", "cmj"), ("direct", "bvh", "cmj"), ("path", "brute", "pmj02bn")]


@pytest.mark.parametrize("integrator,accel,sampler", KERNELS)
@pytest.mark.parametrize("scene_name", ["cbox", "lights3"])
def test_euler_identity(scene_name, integrator, accel, sampler):
    s = build(scene_name, integrator, accel, sampler)
    e = emissions_of(s)
    lhs, rhs, d_e = euler(Case(s), e)
    s.check()
    print(f"[euler] {scene_name} {integrator} {accel} {sampler}: <g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3, lhs
    rows_outside_the_light_list_are_zero(s, d_e)
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_euler_identity_on_the_light_stage(integrator):
    s = build("stage", integrator)
    assert s.info()["accel"] == "bvh" and s.light_count == 4
    e = emissions_of(s)
    case = Case(s, [cuda(fd_material_np(64, 3))], w=64)
    lhs, rhs, d_e = euler(case, e)
    s.check()
    print(f"[euler] light stage {integrator}: <g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3, lhs
    # (not every light of the stage lights what this camera sees: test_gpu_lightstage.py's switching test finds the same)
    assert float(d_e[0].abs().sum()) == 0.0 and int((d_e[1:].abs().sum(dim=1) > 0).sum()) >= 2
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


# ------------------------------------------------------------------------------- 2. light by light against the oracle
OW, OSPP, OSEED = 48, 16, 6        # the oracle's forward (and the product's) runs with seed 6: the backward is called with seed 5


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("material", ["cbox", "fd64"])
def test_each_component_against_the_oracles_forward(integrator, material):
    A = multi_light_arrays()
    S = oracle.OracleScene.from_arrays(A)
    s = make_scene(integrator, arrays=A)
    mat = cbox_material_np() if material == "cbox" else fd_material_np(64, 0)
    e0 = A.inst_emission.astype(np.float32)
    g = cotangent(OW, OW, 1)
    g64 = g.astype(np.float64)
    p = oracle_params(s, OW, OW, OSPP, OSEED, mat.shape[:2])
    S.set_emissions(e0)
    base, cnt = S.render_forward(p, mat, counters=True)
    assert cnt["nan_samples"] == 0 and float(base[..., :3].max()) < 1e4, (cnt, float(base.max()))   # preconditions: no dropped sample, no clamp
    case = Case(s, [cuda(mat)], w=OW, spp=OSPP, seed=OSEED - 1)
    _, d_e = case.backward(cuda(g), cuda(e0))
    s.check()
    d_e = d_e.double().cpu().numpy()
    base_hip = case.forward(cuda(e0))
    comps = [(k, c) for k in range(A.ninst) for c in range(3) if e0[k, c] > 0]
    assert len(comps) == 9
    ours, orc, hip = [], [], []
    for k, c in comps:
        e = e0.copy(); e[k, c] *= 2
        S.set_emissions(e)
        img, cnt = S.render_forward(p, mat, counters=True)
        assert cnt["nan_samples"] == 0 and float(img[..., :3].max()) < 1e4
        orc.append(float((g64 * (img.astype(np.float64) - base.astype(np.float64))).sum()))
        hip.append(float((g64 * (case.forward(cuda(e)) - base_hip)).sum()))
        ours.append(float(d_e[k, c] * e0[k, c]))
    S.set_emissions(e0)
    total = float(np.abs(orc).sum())
    for (k, c), a, o, h in zip(comps, ours, orc, hip):
        print(f"[oracle] {integrator} {material} e[{k},{c}]: d_e * e = {a!r}, oracle difference {o!r} ({abs(a - o) / total:.3e} of the total), "
              f"product difference {h!r} (rel {rel(a, h):.3e})")
    assert (d_e[0] == 0).all() and (d_e[3] == 0).all()                 # the textured model and the blocker
    for (k, c), a, o, h in zip(comps, ours, orc, hip):
        assert abs(a - o) <= 1e-4 * total, (k, c, a, o, total)
        assert rel(a, h) <= 1e-4, (k, c, a, h)


# ------------------------------------------------------------------------------------ 3. a zero channel has a gradient
@pytest.mark.parametrize("integrator,accel", [("path", "bvh"), ("path", "brute"), ("direct", "bvh"), ("direct", "brute")])
def test_a_zero_channel_has_a_gradient(integrator, accel):
    A = multi_light_arrays(emissions=((0, 0, 0), (20, 20, 20), (6, 2, 0), (0, 0, 0), (1, 3, 8)))
    s = make_scene(integrator, accel=accel, arrays=A)
    assert s.info()["accel"] == accel and s.light_count == 3
    e = emissions_of(s)
    D = torch.zeros_like(e)
    D[2, 2] = 1.5                                                       # blue of the light at (6, 2, 0)
    lhs, rhs, _ = difference(Case(s), e, D)
    s.check()
    print(f"[zero channel] {integrator} {accel}: {lhs!r} vs {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3, lhs
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


# ----------------------------------------------------------------- 4. environment map in the scene; several materials
def direction(e, seed=1):
    D = torch.rand(e.shape, generator=torch.Generator().manual_seed(seed)).cuda() * 2.0 + 0.5
    return D * (e > 0).any(dim=1, keepdim=True)                       # (a row outside the light list is ignored anyway)


@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "brute"), ("direct", "bvh")])
def test_difference_identity_with_an_environment_map_in_the_scene(integrator, accel):
    from test_gpu_envmap_grad import sky
    s = make_scene(integrator, accel=accel, arrays=multi_light_arrays())
    s.add_envmap(sky())
    case = Case(s)
    e = emissions_of(s)
    lhs, rhs, d_e = difference(case, e, direction(e))
    s.check()
    print(f"[env] {integrator} {accel}: {lhs!r} vs {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)
    rows_outside_the_light_list_are_zero(s, d_e)
    g = cuda(cotangent(W, W, 3))
    (dm_e,), _ = case.backward(g, e)
    (dm,), none = case.backward(g, e, with_emission=False)
    assert none is None
    assert float((dm_e.double() - dm.double()).norm() / dm.double().norm()) <= 1e-6


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_difference_identity_with_two_materials(integrator):
    from test_gpu_materials import split_arrays
    s = make_scene(integrator, arrays=split_arrays())                  # cboxuv.obj in two instances, the light third
    mats = [cuda(fd_material_np(64, 0)), cuda(fd_material_np(16, 1))]
    case = Case(s, mats, [0, 1, None])
    e = emissions_of(s)
    lhs, rhs, d_e = difference(case, e, direction(e))
    s.check()
    print(f"[two materials] {integrator}: {lhs!r} vs {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)
    assert float(d_e[:2].abs().sum()) == 0.0
    g = cuda(cotangent(W, W, 3))
    dm_e, _ = case.backward(g, e)
    dm, _ = case.backward(g, e, with_emission=False)
    for a, b in zip(dm_e, dm):
        assert float(b.abs().sum()) > 0.0
        assert float((a.double() - b.double()).norm() / b.double().norm()) <= 1e-6


# --------------------------------------------------------------------------------------------- 5. accumulation at size
def test_euler_identity_at_size():
    """Cornell box, path, 512^2, spp 64: 16.8 M samples and about twice as many terms onto three floats.  If this fails where the
    small cases pass, the accumulation is losing bits."""
    s = make_scene("path")
    e = emissions_of(s)
    lhs, rhs, _ = euler(Case(s, w=512, spp=64), e)
    s.check()
    print(f"[euler at size] <g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)


# ---------------------------------------------------------------------------------------------------------- 6. autograd
@pytest.mark.parametrize("several", [False, True])
def test_autograd(several):
    A = multi_light_arrays()
    s = make_scene("path", arrays=A)
    m = cuda(fd_material_np(64, 0)).requires_grad_()
    if several:
        s.material_slots = [0, None, None, None, None]
    E = emissions_of(s).requires_grad_()
    g = cuda(cotangent(W, W, 4))
    fresh = make_scene("path", arrays=A)
    if several:
        fresh.material_slots = [0, None, None, None, None]
    plain = fresh.render(m.detach(), res=(W, W), spp=SPP, seed=SEED)
    out = s.render(m, res=(W, W), spp=SPP, seed=SEED, emissions=E)
    assert torch.equal(out.detach(), plain)                            # the scene's own values: the same image, bit for bit
    with torch.no_grad():
        E *= 3.0                                                        # changed in place between forward and backward
    (out * g).sum().backward()
    assert E.grad.shape == (A.ninst, 3)
    d_e, d_m = torch.zeros((A.ninst, 3), device="cuda"), torch.zeros_like(m)
    s.render_backward(g, d_m, m.detach(), (W, W), SPP, SEED, d_emission=d_e)    # the scene holds the forward's values again
    torch.testing.assert_close(E.grad, d_e, rtol=1e-5, atol=1e-6 * float(d_e.abs().max()))
    torch.testing.assert_close(m.grad, d_m, rtol=1e-5, atol=1e-6 * float(d_m.abs().max()))
    assert float(E.grad[0].abs().sum()) == 0.0 and float(E.grad[3].abs().sum()) == 0.0
    # a later render() without emissions= keeps the values: the image of a scene that was given them through update_lights
    E2 = emissions_of(s) * torch.tensor([1.0, 0.5, 2.0], device="cuda")
    s.render(m.detach(), res=(W, W), spp=SPP, seed=SEED, emissions=E2)
    later = s.render(m.detach(), res=(W, W), spp=SPP, seed=SEED)
    fresh.update_lights([tuple(r) for r in E2.cpu().numpy().tolist()])
    assert torch.equal(later, fresh.render(m.detach(), res=(W, W), spp=SPP, seed=SEED))
    # and update_lights replaces them, and the light list, as before
    s.update_lights([tuple(r) for r in A.inst_emission.tolist()])
    assert torch.equal(s.render(m.detach(), res=(W, W), spp=SPP, seed=SEED), plain)


def test_an_older_render_is_differentiated_with_its_own_emissions():
    """Two renders with different emissions, then the backward of the first: the node applies its snapshot again."""
    s = make_scene("path", arrays=multi_light_arrays())
    m = cuda(fd_material_np(64, 0)).requires_grad_()
    E1 = emissions_of(s).requires_grad_()
    E2 = (emissions_of(s) * 0.25).requires_grad_()
    g = cuda(cotangent(W, W, 5))
    out1 = s.render(m, res=(W, W), spp=SPP, seed=SEED, emissions=E1)
    s.render(m, res=(W, W), spp=SPP, seed=SEED, emissions=E2)
    (out1 * g).sum().backward()
    d_m = torch.zeros_like(m)
    d_e = torch.zeros_like(E1)
    s.set_emission_values(E1.detach())
    s.render_backward(g, d_m, m.detach(), (W, W), SPP, SEED, d_emission=d_e)
    torch.testing.assert_close(m.grad, d_m, rtol=1e-5, atol=1e-6 * float(d_m.abs().max()))
    torch.testing.assert_close(E1.grad, d_e, rtol=1e-5, atol=1e-6 * float(d_e.abs().max()))


def test_collocated_accepts_the_argument_and_returns_a_zero_gradient():
    s = make_scene("collocated")
    m = cuda(fd_material_np(64, 0)).requires_grad_()
    E = emissions_of(s).requires_grad_()
    out = s.render(m, res=(W, W), spp=SPP, seed=SEED, emissions=E)
    out.sum().backward()
    assert E.grad.shape == (2, 3) and float(E.grad.abs().sum()) == 0.0 and float(m.grad.abs().sum()) > 0.0


# ------------------------------------------------------------------------------------------- 7. C-ABI, argument checks
def test_a_null_d_emission_is_the_sibling_call_and_collocated_leaves_it_alone():
    L = N.lib()
    m = cuda(fd_material_np(64, 0))
    g = cuda(cotangent(W, W, 6))
    for integrator in ("path", "direct"):
        s = make_scene(integrator)
        a, b = torch.zeros_like(m), torch.zeros_like(m)
        p = s._params((W, W), SPP, SEED + 1, m.shape[:2])
        N.check(L.zdr_render_backward_emission(s._handle, C.byref(p), g.data_ptr(), m.data_ptr(), a.data_ptr(), None, s._stream()))
        s.render_backward(g, b, m, (W, W), SPP, SEED)
        torch.cuda.synchronize()
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)
    s = make_scene("collocated")
    d_e = torch.full((2, 3), 7.0, device="cuda")
    a, b = torch.zeros_like(m), torch.zeros_like(m)
    s.render_backward(g, a, m, (W, W), SPP, SEED, d_emission=d_e)
    s.render_backward(g, b, m, (W, W), SPP, SEED)
    torch.cuda.synchronize()
    assert bool((d_e == 7.0).all())
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)


def test_the_gradient_is_accumulated_into_d_emission():
    s = make_scene("path")
    case = Case(s)
    e = emissions_of(s)
    g = cuda(cotangent(W, W, 7))
    _, once = case.backward(g, e)
    twice = torch.full_like(e, 1.0)
    dm = torch.zeros_like(case.mats[0])
    s.render_backward(g, dm, case.mats[0], (W, W), SPP, SEED, d_emission=twice)
    torch.cuda.synchronize()
    assert bool((twice[0] == 1.0).all())                                # the row of the textured model: untouched
    torch.testing.assert_close(twice[1], once[1] + 1.0, rtol=1e-5, atol=0.0)


def test_arguments_are_checked():
    from test_gpu_envmap_grad import sky
    s = make_scene("path")
    s.add_envmap(sky())
    m = cuda(fd_material_np(64, 0))
    e = emissions_of(s)
    with pytest.raises(ValueError, match="envmap"):
        s.render(m, res=(W, W), spp=4, emissions=e, envmap=cuda(sky()))
    for bad in (e[:1], e.double(), e.cpu(), torch.zeros((2, 4), device="cuda")):
        with pytest.raises(ValueError):
            s.render(m, res=(W, W), spp=4, emissions=bad)
        with pytest.raises(ValueError):
            s.set_emission_values(bad)
    dm = torch.zeros_like(m)
    g = cuda(cotangent(W, W))
    with pytest.raises(ValueError, match="d_env"):
        s.render_backward(g, dm, m, (W, W), 4, 0, d_emission=torch.zeros_like(e), d_env=torch.zeros((64, 64, 4), device="cuda"))
    with pytest.raises(ValueError, match="d_emission"):
        s.render_backward(g, dm, m, (W, W), 4, 0, d_emission=torch.zeros((3, 3), device="cuda"))
