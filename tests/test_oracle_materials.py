"""Pins the oracle's material table (zdro_scene_set_material_slots, zdro_render_*_materials), the reference the GPU tests of
per-model materials compare against (tests/test_gpu_materials_oracle.py): the legacy table reproduces the single-material calls
bit for bit, permuting the materials together with the slots permutes nothing else, a mesh split in two renders as it did whole,
and the direct integrator's gradient of a second, non-square material is exact for its diffuse texels."""
import numpy as np
import pytest

import oracle
from conftest import CBOX_CAMERA, cbox_models, fd_material_np
from test_oracle_render import _weights
from zdr_amd import geometry

INTEGRATORS = ["path", "direct", "collocated"]


def split_box(bounds):
    """The Cornell box with cboxuv.obj's 30 triangles cut into instances [bounds[i], bounds[i + 1]) (same vertices, same triangle
    order), the light last."""
    a = geometry.assemble(cbox_models())
    b = a.inst_tri_begin
    n = int(b[1])
    assert bounds[0] == 0 and bounds[-1] == n and list(bounds) == sorted(set(bounds))
    k = len(bounds) - 1
    return geometry.from_arrays(a.verts, a.tris, list(bounds) + [int(b[2])],
                                np.concatenate([np.repeat(a.inst_xform[:1], k, 0), a.inst_xform[1:]]),
                                np.concatenate([np.repeat(a.inst_emission[:1], k, 0), a.inst_emission[1:]]))


def textured(h, w, seed):
    """A non-constant (h, w) material of its own content: diffuse in [0.2, 0.8], roughness in [0.6, 1]."""
    rng = np.random.default_rng(seed)
    m = np.empty((h, w, 4), np.float32)
    m[..., :3] = rng.uniform(0.2, 0.8, (h, w, 3)); m[..., 3] = rng.uniform(0.6, 1.0, (h, w))
    return m


def params(integrator, W, spp, seed, **kw):
    return oracle.make_params(integrator, W, W, spp, seed, CBOX_CAMERA, (1, 1), nthreads=1, **kw)


@pytest.fixture(scope="module")
def cbox_scene():
    return oracle.OracleScene.from_arrays(geometry.assemble(cbox_models()))


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_legacy_table_is_the_single_material_call_bit_for_bit(integrator, cbox_scene):
    S = cbox_scene
    mat = textured(23, 41, 1)
    W, spp = 32, 4
    p = oracle.make_params(integrator, W, W, spp, 3, CBOX_CAMERA, mat.shape[:2], nthreads=1)
    ref, cref = S.render_forward(p, mat, counters=True)
    cot = _weights(W, W)
    gref, gcref = S.render_backward(p, cot, mat, counters=True)
    S.set_material_slots([0, 0] if integrator == "collocated" else [0, None])
    try:
        img, cnt = S.render_forward_materials(p, [mat], counters=True)
        (g,), gcnt = S.render_backward_materials(p, cot, [mat], counters=True)
    finally:
        S.set_material_slots(None)
    assert ref[..., :3].max() > 0 and np.abs(gref).max() > 0
    assert np.array_equal(img, ref) and cnt == cref
    assert np.array_equal(g, gref) and gcnt == gcref


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_permuting_materials_with_their_slots_permutes_the_gradients(integrator):
    S = oracle.OracleScene.from_arrays(split_box([0, 7, 15, 23, 30]))
    mats = [textured(37, 91, 2), textured(5, 3, 3), textured(1, 1, 4)]
    slots = [2, 0, 1, None]
    W, spp = 32, 4
    p = params(integrator, W, spp, 5)
    cot = _weights(W, W)
    S.set_material_slots(slots + [None])
    img = S.render_forward_materials(p, mats)
    g = S.render_backward_materials(p, cot, mats)
    assert all(np.abs(gk).sum() > 0 for gk in g)                  # every material is seen
    perm = [2, 0, 1]                                              # new list entry j is old material perm[j]
    inv = {old: new for new, old in enumerate(perm)}
    S.set_material_slots([None if k is None else inv[k] for k in slots] + [None])
    img2 = S.render_forward_materials(p, [mats[k] for k in perm])
    g2 = S.render_backward_materials(p, cot, [mats[k] for k in perm])
    assert np.array_equal(img2, img)
    for new, old in enumerate(perm):
        assert np.array_equal(g2[new], g[old])


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_a_split_mesh_shaded_by_one_material_twice_renders_as_it_did_whole(integrator, cbox_scene):
    S = oracle.OracleScene.from_arrays(split_box([0, 15, 30]))
    mat = textured(19, 27, 5)
    W, spp = 32, 8
    p = oracle.make_params(integrator, W, W, spp, 7, CBOX_CAMERA, mat.shape[:2], nthreads=1)
    ref = cbox_scene.render_forward(p, mat)
    cot = _weights(W, W)
    gref = cbox_scene.render_backward(p, cot, mat)
    whole_slots = [0, 0, 0] if integrator == "collocated" else [0, 0, None]
    S.set_material_slots(whole_slots)
    assert np.array_equal(S.render_forward_materials(p, [mat]), ref)
    S.set_material_slots([0, 1, 0 if integrator == "collocated" else None])
    assert np.array_equal(S.render_forward_materials(p, [mat, mat]), ref)
    g0, g1 = S.render_backward_materials(p, cot, [mat, mat])
    assert np.abs(g0).sum() > 0 and np.abs(g1).sum() > 0 and not np.array_equal(g0, g1)
    # each texel's terms are split between the two materials: the float64 sums agree to float32 rounding
    np.testing.assert_allclose(g0.astype(np.float64) + g1, gref, rtol=1e-5, atol=1e-6 * np.abs(gref).max())


def test_slot_semantics_of_an_emitter_with_a_material():
    """The light shaded by a material: path still returns its emission first (prb.py:39-44), direct shades it
    (integrators.h, direct_sample), collocated shades what has a material and leaves the rest black."""
    A = geometry.assemble(cbox_models())
    S = oracle.OracleScene.from_arrays(A)
    light = textured(2, 3, 9)
    mat = textured(8, 8, 8)
    W, spp = 32, 4
    for integrator in INTEGRATORS:
        p = params(integrator, W, spp, 1)
        S.set_material_slots([0, None])
        plain = S.render_forward_materials(p, [mat, light])
        S.set_material_slots([0, 1])
        lit = S.render_forward_materials(p, [mat, light])
        if integrator == "path":
            assert np.array_equal(lit, plain)
        else:
            assert not np.array_equal(lit, plain)
    S.set_material_slots([None, 0])                               # collocated: the box has no material, black
    img = S.render_forward_materials(params("collocated", W, spp, 1), [light])
    full = S.render_forward(oracle.make_params("collocated", W, W, spp, 1, CBOX_CAMERA, light.shape[:2], nthreads=1), light)
    assert 0 < img[..., :3].sum() < 0.5 * full[..., :3].sum()


def test_bad_tables_are_refused():
    S = oracle.OracleScene.from_arrays(split_box([0, 15, 30]))
    p = params("path", 8, 1, 0)
    S.set_material_slots([0, 1, None])
    with pytest.raises(RuntimeError, match="rc=-5"):
        S.render_forward_materials(p, [textured(2, 2, 0)])           # slot 1 of one material
    with pytest.raises(RuntimeError, match="rc=-5"):
        S.render_forward_materials(p, [textured(1, 1, k) for k in range(17)])
    with pytest.raises(RuntimeError, match="rc=-3"):
        S.render_forward_materials(params("uvgrad", 8, 1, 0), [textured(2, 2, 0), textured(2, 2, 1)])


def test_direct_gradient_of_a_second_material_is_exact_for_diffuse():
    """direct is exactly linear in the diffuse texels of every material and its sampling ignores them (as
    tests/test_oracle_render.py, test_direct_gradient_is_exact_for_diffuse): the directional derivative along the diffuse
    texels of the SECOND material, and a central difference at one texel of it (7 x 4, non-square), are exact."""
    S = oracle.OracleScene.from_arrays(split_box([0, 15, 30]))
    S.set_material_slots([0, 1, None])
    a, b = fd_material_np(64, 0), textured(7, 4, 11)
    W, spp = 48, 16
    p = oracle.make_params("direct", W, W, spp, 11, CBOX_CAMERA, (1, 1))
    wimg = _weights(W, W)
    _, gb = S.render_backward_materials(p, wimg, [a, b])
    rng = np.random.default_rng(5)
    delta = np.zeros_like(b); delta[..., :3] = rng.uniform(-1, 1, b.shape[:2] + (3,))
    eps = 1e-2
    def fd(d):
        ip = S.render_forward_materials(p, [a, (b + eps * d).astype(np.float32)]).astype(np.float64)
        im = S.render_forward_materials(p, [a, (b - eps * d).astype(np.float32)]).astype(np.float64)
        return float(((ip - im) * wimg).sum() / (2 * eps))
    ad, f = float((gb.astype(np.float64) * delta).sum()), fd(delta)
    assert abs(f) > 0 and abs(ad - f) / abs(f) < 2e-4, (ad, f)
    # one texel, one channel of the 7 x 4 material: the one with the largest gradient
    y, x, c = np.unravel_index(np.argmax(np.abs(gb[..., :3])), gb[..., :3].shape)
    one = np.zeros_like(b); one[y, x, c] = 1.0
    ad1, f1 = float(gb[y, x, c]), fd(one)
    assert abs(f1) > 0 and abs(ad1 - f1) / abs(f1) < 2e-4, (ad1, f1)
