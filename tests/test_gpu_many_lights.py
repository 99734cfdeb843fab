"""-m gpu: the light paths with more lights than the emission-gradient kernels' on-chip table holds (ZDR_EMIT_LDS_LIGHTS = 10,
zdr_kernels.hip: a light with list index >= 10 adds into the accumulator with global atomics, emit_add's other branch), on the two
scenes of many_lights.py: the chandelier (Cornell box, 15 lights, a blocker in the middle of the instance list) and the light stage
with all 30 lights.  test_many_lights_host.py holds the preconditions: the lights beyond the table carry 39 - 42 % of the gradient
on the chandelier and most of it on the stage.

Forward and material gradient against the oracle; the emission gradient light by light against the oracle's forward, by Euler's
identity across prb_mode, sampler, image shape, sample count, filter and depth, and at size; the shards of the emission and the
environment gradient against the unsharded call; update_lights followed by a gradient.  The helpers and the bars are those of
test_gpu_emission_grad.py, test_gpu_lights.py, test_gpu_lightstage.py and test_gpu_render.py.

Measured: see DESIGN.md, section 2."""
import numpy as np
import pytest
import torch

import oracle
from conftest import cbox_material_np, fd_material_np
from gpu_util import Flips, assert_grad_parity, assert_image_parity, make_scene, oracle_params
from many_lights import (CAMERA, LDS_LIGHTS, NLIGHT, OSEED, OSPP, OW, chandelier_arrays, cotangent_planes, light_rows, oracle_terms,
                         panel_instance, shares, stage30_arrays, stage30_models)
from test_gpu_emission_grad import (Case, cotangent, cuda, difference, direction, emissions_of, euler, rel, rows_outside_the_light_list_are_zero,
                                    with_sampler)
from zdr_amd import Scene

pytestmark = pytest.mark.gpu

TAG = "[many lights]"


def chandelier(integrator, accel="auto", sampler="cmj", arrays=None, lights=15):
    s = make_scene(integrator, accel=accel, arrays=chandelier_arrays() if arrays is None else arrays)
    if accel != "auto":
        assert s.info()["accel"] == accel
    assert s.light_count == lights == s.info()["light_count"]
    return with_sampler(s, sampler)


def stage30(integrator):
    s = Scene(stage30_models(), integrator=integrator)
    s.camera = CAMERA
    assert s.info()["accel"] == "bvh" and s.light_count == NLIGHT == s.info()["light_count"]
    return s


@pytest.fixture(scope="module")
def chandelier_oracles():
    A = chandelier_arrays()
    return A, oracle.OracleScene.from_arrays(A), oracle.OracleScene.from_arrays(A, variant="fma")


@pytest.fixture(scope="module")
def stage_oracles():
    A = stage30_arrays()
    return A, oracle.OracleScene.from_arrays(A), oracle.OracleScene.from_arrays(A, variant="fma")


def material(name):
    if name == "cbox":
        return cbox_material_np()
    if name == "fd64":
        return fd_material_np(64, 0)
    mat = fd_material_np(256, 3); mat[..., 3] = 0.6 + 0.4 * mat[..., 3]     # "rough": the light stage's, roughness 0.72 - 0.96
    return mat


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ a. forward and material gradient against the oracle
def against_the_oracle(scene, oracles, name, mat, W, spp, seed):
    """test_light_stage_matches_the_oracle's comparison: image and material gradient against the oracle, the oracle's FMA build as
    the ruler, the measurably flipped paths of `path` set aside (direct has no per-path dump)."""
    A, S, Sf = oracles
    S.set_emissions(A.inst_emission); Sf.set_emissions(A.inst_emission)
    integrator = scene.integrator
    m = torch.from_numpy(mat).cuda().requires_grad_()
    cot = np.random.default_rng(5).uniform(0.5, 1.5, (W, W, 4)).astype(np.float32)
    img = scene.render(m, res=(W, W), spp=spp, seed=seed)
    (img * torch.from_numpy(cot).cuda()).sum().backward()
    scene.check()
    p, pb = oracle_params(scene, W, W, spp, seed, mat.shape[:2]), oracle_params(scene, W, W, spp, seed + 1, mat.shape[:2])
    ref, gref, floor, gfloor = cached((name, integrator, "parity"), lambda: (S.render_forward(p, mat), S.render_backward(pb, cot, mat),
                                                                            Sf.render_forward(p, mat), Sf.render_backward(pb, cot, mat)))
    assert ref[..., :3].mean() > 0.01 and np.abs(gref).sum() > 0
    path = integrator == "path"
    what = f"{TAG} {name} {integrator}/{scene.info()['accel']}"
    ff = Flips(scene, S, Sf, mat, (W, W), spp, seed, what=f"{what} forward") if path else None
    fb = Flips(scene, S, Sf, mat, (W, W), spp, seed + 1, cot=cot, what=f"{what} backward") if path else None
    assert_image_parity(img.detach().cpu().numpy()[..., :3], ref[..., :3], f"{what} forward", flips=ff, floor=floor[..., :3])
    assert_grad_parity(m.grad.cpu().numpy(), gref, f"{what} backward", flips=fb, floor=gfloor)


@pytest.mark.parametrize("integrator", ["direct", "path"])
@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_chandelier_forward_and_backward(integrator, accel, chandelier_oracles):
    against_the_oracle(chandelier(integrator, accel), chandelier_oracles, "chandelier", material("cbox"), 96, 16, 11)


@pytest.mark.parametrize("integrator", ["direct", "path"])
def test_stage_of_thirty_lights_forward_and_backward(integrator, stage_oracles):
    against_the_oracle(stage30(integrator), stage_oracles, "stage", material("rough"), 96, 16, 8)


# ------------------------------------------------------------------------- b. the shadow pair mask changes no answer
@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_shadow_pair_mask_changes_no_answer_under_the_chandelier(integrator, monkeypatch):
    """test_gpu_render.py's test_shadow_pair_mask_changes_no_answer with 14 lights hanging just below the ceiling: the mask rules out
    the pairs that keep their distance from EVERY light.  Images and per-path traces bit for bit, gradients up to the order of the
    float atomics."""
    from path_trace import all_queries
    A = chandelier_arrays()
    monkeypatch.delenv("ZDR_NO_SHADOW_MASK", raising=False)
    a = chandelier(integrator, "brute", arrays=A)
    monkeypatch.setenv("ZDR_NO_SHADOW_MASK", "1")
    b = chandelier(integrator, "brute", arrays=A)
    monkeypatch.delenv("ZDR_NO_SHADOW_MASK", raising=False)
    W, H, spp = 72, 56, 8
    cot = torch.rand((H, W, 4), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) + 0.5
    e = emissions_of(a)
    for name in ("cbox", "rough"):
        m = torch.from_numpy(material(name)).cuda()
        for seed in (1, 2):
            ia, ib = a.render_forward(m, (W, H), spp, seed), b.render_forward(m, (W, H), spp, seed)
            assert torch.equal(ia, ib), (name, seed)
            ga, gb, ea, eb = torch.zeros_like(m), torch.zeros_like(m), torch.zeros_like(e), torch.zeros_like(e)
            a.render_backward(cot, ga, m, (W, H), spp, seed, d_emission=ea); b.render_backward(cot, gb, m, (W, H), spp, seed, d_emission=eb)
            torch.testing.assert_close(ga, gb, rtol=1e-4, atol=1e-6 * float(gb.abs().max()))   # float atomics: same terms, free order
            torch.testing.assert_close(ea, eb, rtol=1e-4, atol=1e-6 * float(eb.abs().max()))
            assert float(eb[light_rows(A.inst_emission)].abs().min()) > 0.0
            if integrator == "path":
                q = torch.from_numpy(all_queries(W, H, spp)).cuda()
                assert torch.equal(a.path_dump(m, q, (W, H), spp, seed + 1, d_image=cot).view(torch.int32),
                                   b.path_dump(m, q, (W, H), spp, seed + 1, d_image=cot).view(torch.int32)), (name, seed)
        assert float(ia[..., :3].sum()) > 0.0
    a.check(); b.check()


# ---------------------------------------------------------------------- c. light by light against the oracle's forward
def light_by_light(s, S, mat, e0, what, key=None, share_floor=0.0):
    """test_each_component_against_the_oracles_forward's scheme, a light at a time: one oracle render with row k doubled gives the
    three components of light k through the cotangent's channel planes.  Per component |d_e e - oracle difference| <= 1e-4 of
    sum |oracle terms|; rel <= 1e-4 against the product's own forward difference for the lights whose share of the oracle's total is
    at least `share_floor`.  Returns (shares, worst residual against the oracle, worst against the product)."""
    e0 = np.ascontiguousarray(e0, np.float32)
    g = cotangent(OW, OW, 1)
    p = oracle_params(s, OW, OW, OSPP, OSEED, mat.shape[:2])
    terms = cached(key, lambda: oracle_terms(S, p, mat, e0, g)[0]) if key is not None else oracle_terms(S, p, mat, e0, g)[0]
    case = Case(s, [cuda(mat)], w=OW, spp=OSPP, seed=OSEED - 1)
    _, d_e = case.backward(cuda(g), cuda(e0))
    s.check()
    d = d_e.double().cpu().numpy()
    base_hip = case.forward(cuda(e0))
    planes = cotangent_planes(g)
    total, sh = float(np.abs(terms).sum()), shares(terms)
    rows = []
    for k in light_rows(e0):
        e = e0.copy(); e[k] *= 2
        dI = case.forward(cuda(e)) - base_hip
        for c in range(3):
            if e0[k, c] > 0:
                rows.append((k, c, float(d[k, c] * e0[k, c]), float(terms[k, c]), float((planes[c] * dI).sum())))
    s.check()
    worst_o = max(abs(a - o) / total for _, _, a, o, _ in rows)
    worst_h = max(rel(a, h) for k, _, a, _, h in rows if sh[k] >= share_floor)
    for k, c, a, o, h in rows:
        print(f"{TAG} {what} e[{k},{c}] (light {light_rows(e0).index(k)}, share {sh[k]:.4f}): d_e * e = {a!r}, oracle difference {o!r} "
              f"({abs(a - o) / total:.3e} of the total), product difference {h!r} (rel {rel(a, h):.3e})")
    print(f"{TAG} {what}: worst against the oracle {worst_o:.3e} of the total, worst against the product's forward {worst_h:.3e}")
    dark = ~(e0 > 0).any(axis=1)
    assert (d[dark] == 0).all(), d[dark]                                # the textured model, the blocker, lights switched off
    for k, c, a, o, h in rows:
        assert abs(a - o) <= 1e-4 * total, (k, c, a, o, total)
        if sh[k] >= share_floor:
            assert rel(a, h) <= 1e-4, (k, c, a, h)
    return sh, worst_o, worst_h


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("accel", ["brute", "bvh"])
@pytest.mark.parametrize("mat_name", ["cbox", "fd64"])
def test_each_light_of_the_chandelier_against_the_oracles_forward(integrator, accel, mat_name, chandelier_oracles):
    A, S, _ = chandelier_oracles
    s = chandelier(integrator, accel, arrays=A)
    sh, _, _ = light_by_light(s, S, material(mat_name), A.inst_emission, f"chandelier {integrator}/{accel} {mat_name}",
                              key=("chandelier", integrator, mat_name))
    assert (sh[light_rows(A.inst_emission)] >= 0.01).all()              # (test_many_lights_host.py) every light counts, so every rel bar is live


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_each_light_of_the_stage_against_the_oracles_forward(integrator, stage_oracles):
    """All 30 lights: the absolute bar for each, the relative one where the oracle's share is at least 1e-3 (several lights sit behind
    the sphere and carry nothing); at least 10 of those lie beyond the table."""
    A, S, _ = stage_oracles
    s = stage30(integrator)
    mat = material("rough")
    sh, _, _ = light_by_light(s, S, mat, A.inst_emission, f"stage {integrator}", key=("stage", integrator), share_floor=1e-3)
    beyond = [l for l in range(LDS_LIGHTS, NLIGHT) if sh[1 + l] >= 1e-3]
    print(f"{TAG} stage {integrator}: lights beyond the table under the relative bar: {beyond}")
    assert len(beyond) >= 10, sh


# ------------------------------------------------------------------------------------------------ d. Euler's identity
def euler_on_the_chandelier(integrator, accel="auto", sampler="cmj", prb_mode=None, w=32, h=32, spp=16, tent=True, depth=None):
    s = chandelier(integrator, accel, sampler)
    if prb_mode is not None:
        s.prb_mode = prb_mode
    s.use_tent_filter = tent
    if depth is not None:
        s.max_depth, s.rr_depth = depth
    e = emissions_of(s)
    lhs, rhs, d_e = euler(Case(s, w=w, h=h, spp=spp), e)
    s.check()
    print(f"{TAG} euler {integrator} {accel} {sampler} prb_mode={prb_mode} {w}x{h} spp {spp} tent={tent} depth={depth}: "
          f"<g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3, lhs
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)
    rows_outside_the_light_list_are_zero(s, d_e)
    assert float(d_e[light_rows(s._arrays.inst_emission)[LDS_LIGHTS:]].abs().min()) > 0.0     # the lights beyond the table receive something


@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "brute"), ("direct", "bvh")])
@pytest.mark.parametrize("sampler", ["cmj", "pmj02bn"])
@pytest.mark.parametrize("prb_mode", [None, "detached", "literal"])
def test_euler_identity_in_every_prb_mode(integrator, accel, sampler, prb_mode):
    euler_on_the_chandelier(integrator, accel, sampler, prb_mode)


@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "brute"), ("direct", "bvh")])
@pytest.mark.parametrize("w,h,spp", [(32, 32, 16), (77, 52, 12), (40, 24, 48), (33, 47, 2)])
def test_euler_identity_at_other_shapes_and_sample_counts(integrator, accel, w, h, spp):
    """Non-square images and sample counts that are not powers of two (the cotangent is then divided by spp, not scaled by C.inv_spp)."""
    euler_on_the_chandelier(integrator, accel, w=w, h=h, spp=spp)


@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "brute"), ("direct", "bvh")])
def test_euler_identity_with_the_box_filter(integrator, accel):
    euler_on_the_chandelier(integrator, accel, tent=False, w=40, h=24, spp=12)


@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "bvh")])
@pytest.mark.parametrize("depth", [(1, 2), (2, 0), (16, 0)])
def test_euler_identity_at_other_depths(integrator, accel, depth):
    euler_on_the_chandelier(integrator, accel, depth=depth)


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_euler_identity_with_two_materials(integrator):
    from test_gpu_materials import split_arrays
    A = chandelier_arrays(base=split_arrays())                          # cboxuv.obj in two instances, the ceiling light third, then the panels
    s = chandelier(integrator, arrays=A)
    assert A.ninst == 18 and light_rows(A.inst_emission)[LDS_LIGHTS] == panel_instance(9, first=3)
    mats = [cuda(fd_material_np(64, 0)), cuda(fd_material_np(16, 1))]
    e = emissions_of(s)
    lhs, rhs, d_e = euler(Case(s, mats, [0, 1] + [None] * 16), e)
    s.check()
    print(f"{TAG} euler two materials {integrator}: <g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)
    rows_outside_the_light_list_are_zero(s, d_e)
    assert float(d_e[light_rows(A.inst_emission)].abs().min()) > 0.0


@pytest.mark.parametrize("integrator,accel", [("path", "brute"), ("path", "bvh"), ("direct", "brute"), ("direct", "bvh")])
def test_difference_identity_with_an_environment_map_over_the_chandelier(integrator, accel):
    from test_gpu_envmap_grad import sky
    s = chandelier(integrator, accel)
    s.add_envmap(sky())
    e = emissions_of(s)
    lhs, rhs, d_e = difference(Case(s), e, direction(e))
    s.check()
    print(f"{TAG} env {integrator} {accel}: {lhs!r} vs {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)
    rows_outside_the_light_list_are_zero(s, d_e)


def per_light_euler(case, e, what, rows):
    """<d_e[k], e[k]> against the product's forward difference <g, I(row k doubled) - I(e)>, light by light: (light, lhs, rhs)."""
    g = cotangent(case.res[0], case.res[1], 2)
    g64 = g.astype(np.float64)
    base = case.forward(e)
    _, d_e = case.backward(cuda(g), e)
    out = []
    for k in rows:
        e2 = e.clone(); e2[k] *= 2
        lhs = float((g64 * (case.forward(e2) - base)).sum())
        rhs = float((d_e[k].double() * e[k].double()).sum())
        print(f"{TAG} {what} row {k}: <g, dI> = {lhs!r}, <d_e[k], e[k]> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
        out.append((k, lhs, rhs))
    return out, d_e


@pytest.mark.parametrize("integrator,accel", [("path", "bvh"), ("direct", "brute")])
def test_euler_identity_of_each_light_beyond_the_table(integrator, accel):
    """A fault confined to the rows of the fallback cannot hide in a sum the ceiling light dominates."""
    s = chandelier(integrator, accel)
    e = emissions_of(s)
    rows = light_rows(s._arrays.inst_emission)[LDS_LIGHTS:]
    assert len(rows) == 5
    out, _ = per_light_euler(Case(s), e, f"beyond the table {integrator}/{accel}", rows)
    s.check()
    for k, lhs, rhs in out:
        assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (k, lhs, rhs)


# --------------------------------------------------------------------------------------------- e. accumulation at size
def test_euler_identity_of_each_light_at_size():
    """Chandelier, path, 512^2, spp 64: test_euler_identity_at_size for the fallback's global atomics, where the waves whose block
    index agrees modulo 256 share a row of the accumulator."""
    s = chandelier("path")
    e = emissions_of(s)
    out, _ = per_light_euler(Case(s, w=512, spp=64), e, "at size", light_rows(s._arrays.inst_emission))
    s.check()
    print(f"{TAG} at size: worst rel {max(rel(l, r) for _, l, r in out):.3e}")
    for k, lhs, rhs in out:
        assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (k, lhs, rhs)


# ------------------------------------------------------------------------------------------------------ f. shards add up
def shard_scene(kind, integrator):
    """(scene, a zero gradient of `kind`): the chandelier for d_emission, the Cornell box under sky() for d_env"""
    if kind == "d_emission":
        s = chandelier(integrator)
        return s, torch.zeros_like(emissions_of(s))
    from test_gpu_envmap_grad import sky
    s = make_scene(integrator)
    s.add_envmap(sky())
    return s, torch.zeros(tuple(s._envmap[0].shape), device="cuda")


def shards_add_up(s, kind, zero, m, res, spp, seed, shards, what, common=None):
    """The gradient `kind` (and the material's) of one call against the sum over `shards`, a list of keyword sets: the bar the material
    gradient has in test_shard_unions / test_interleaved_tile_shards_union."""
    common = common or {}
    cot = cuda(cotangent(res[0], res[1], 2))
    whole, parts = torch.zeros_like(zero), torch.zeros_like(zero)
    g_whole, g_parts = torch.zeros_like(m), torch.zeros_like(m)
    s.render_backward(cot, g_whole, m, res, spp, seed, **{kind: whole}, **common)
    for kw in shards:
        s.render_backward(cot, g_parts, m, res, spp, seed, **{kind: parts}, **common, **kw)
    s.check()
    top = float(whole.abs().max())
    print(f"{TAG} shards {what}: max |sum of shards - whole| = {float((parts - whole).abs().max()) / top:.3e} of max |whole| = {top!r}")
    assert top > 0.0
    torch.testing.assert_close(parts, whole, rtol=1e-4, atol=1e-6 * top)
    torch.testing.assert_close(g_parts, g_whole, rtol=1e-4, atol=1e-6 * float(g_whole.abs().max()))
    return whole


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("kind", ["d_emission", "d_env"])
def test_shards_add_up(kind, integrator):
    s, zero = shard_scene(kind, integrator)
    m = cuda(fd_material_np(64, 0))
    what = f"{kind} {integrator}"
    whole = shards_add_up(s, kind, zero, m, (64, 64), 64, 4, [dict(rect=(0, 0, 64, 32)), dict(rect=(0, 32, 64, 64))], f"{what} halves")
    if kind == "d_emission":
        assert float(whole[light_rows(s._arrays.inst_emission)].abs().min()) > 0.0 and float(whole[[0, 7]].abs().sum()) == 0.0
    shards_add_up(s, kind, zero, m, (64, 64), 64, 4, [dict(rect=r) for r in [(0, 0, 40, 64), (40, 0, 64, 24), (40, 24, 64, 64)]], f"{what} ragged thirds")
    shards_add_up(s, kind, zero, m, (64, 64), 64, 4, [dict(samples=r) for r in [(0, 16), (16, 48), (48, 64)]], f"{what} sample ranges")
    for count in (2, 3, 8):
        shards_add_up(s, kind, zero, m, (77, 52), 32, 6, [dict(tile_shard=(r, count)) for r in range(count)], f"{what} {count} tile shards")
    shards_add_up(s, kind, zero, m, (61, 45), 16, 3, [dict(tile_shard=(r, 3)) for r in range(3)], f"{what} tile shards inside a rectangle",
                  common=dict(rect=(13, 7, 58, 41)))


@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("kind", ["d_emission", "d_env"])
def test_a_shard_without_tiles_leaves_the_gradient_untouched(kind, integrator):
    s, zero = shard_scene(kind, integrator)
    m = cuda(fd_material_np(64, 0))
    W, H, spp = 24, 16, 8                                               # 3 x 2 = 6 tiles: shard 6 of 7 owns none
    d, g = torch.full_like(zero, 7.0), torch.zeros_like(m)
    s.render_backward(torch.ones((H, W, 4), device="cuda"), g, m, (W, H), spp, 5, tile_shard=(6, 7), **{kind: d})
    s.check()
    assert bool((d == 7.0).all()) and bool((g == 0).all())
    s.render_backward(torch.ones((H, W, 4), device="cuda"), g, m, (W, H), spp, 5, tile_shard=(0, 7), **{kind: d})    # and a shard that owns one does not
    s.check()
    assert bool((d != 7.0).any()) and float(g.abs().sum()) > 0.0


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_the_material_gradient_of_a_shard_does_not_depend_on_d_emission(integrator):
    s = chandelier(integrator)
    m = cuda(fd_material_np(64, 0))
    cot = cuda(cotangent(77, 52, 3))
    for kw in (dict(rect=(13, 7, 58, 41)), dict(samples=(5, 21)), dict(tile_shard=(1, 3)), dict(rect=(13, 7, 58, 41), tile_shard=(2, 3), samples=(0, 7))):
        a, b = torch.zeros_like(m), torch.zeros_like(m)
        s.render_backward(cot, a, m, (77, 52), 32, 6, d_emission=torch.zeros_like(emissions_of(s)), **kw)
        s.render_backward(cot, b, m, (77, 52), 32, 6, **kw)
        s.check()
        r = float((a.double() - b.double()).norm() / b.double().norm())
        print(f"{TAG} material gradient with and without d_emission, {integrator} {kw}: {r:.3e}")
        assert float(b.abs().sum()) > 0.0 and r <= 1e-6


# ------------------------------------------------------------------------------------ g. update_lights, then a gradient
@pytest.mark.parametrize("integrator", ["path", "direct"])
@pytest.mark.parametrize("values_between", [False, True])
def test_update_lights_then_a_gradient(integrator, values_between, chandelier_oracles):
    """update_lights changes the light list and the light index kept in emission4[..].w: the ceiling light and panels 2, 7 and 11 go
    dark, panel 4 keeps a single channel.  11 lights remain, and panel 13 moves from list index 14 to 10 — still beyond the table."""
    A, S, _ = chandelier_oracles
    s = chandelier(integrator, arrays=A)
    mat = material("fd64")
    e_all = A.inst_emission.astype(np.float32)
    case = Case(s, [cuda(mat)], w=OW, spp=OSPP, seed=OSEED - 1)
    g = cuda(cotangent(OW, OW, 1))
    _, before = case.backward(g, cuda(e_all))
    subset = e_all.copy()
    subset[[1, panel_instance(2), panel_instance(7), panel_instance(11)]] = 0.0
    subset[panel_instance(4)] = (0.0, 7.5, 0.0)
    last = panel_instance(13)
    assert light_rows(e_all).index(last) == 14 and light_rows(subset).index(last) == LDS_LIGHTS
    if values_between:
        s.set_emission_values(cuda(e_all * np.float32(3.0)))
    s.update_lights([tuple(r) for r in subset.tolist()])
    assert s.light_count == 11 == s.info()["light_count"]
    try:
        lhs, rhs, d_e = euler(case, cuda(subset))
        s.check()
        print(f"{TAG} update_lights {integrator}: <g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
        dark = torch.from_numpy(~(subset > 0).any(axis=1)).cuda()
        assert float(d_e[dark].abs().sum()) == 0.0
        assert float(d_e[~dark].abs().sum(dim=1).min()) > 0.0
        assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)
        light_by_light(s, S, mat, subset, f"update_lights {integrator}")
    finally:
        S.set_emissions(e_all)
    if values_between:
        s.set_emission_values(cuda(subset * np.float32(0.25)))
    s.update_lights([tuple(r) for r in e_all.tolist()])
    assert s.light_count == 15 == s.info()["light_count"]
    _, after = case.backward(g, cuda(e_all))
    s.check()
    print(f"{TAG} update_lights {integrator}: back to 15 lights, max rel change of the gradient {float(((after - before).abs() / before.abs().clamp_min(1e-30)).max()):.3e}")
    torch.testing.assert_close(after, before, rtol=1e-5, atol=0.0)
