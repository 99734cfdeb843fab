"""No GPU: the float64 reference of the adjoint of the bounced light (tests/texel_bounce_grad_ref.py) held to account on its own, since the
kernels are held to it.  Its evaluator of the polynomial reproduces the free-running reference's bake; its gradient is the complex-step
derivative of that evaluator, in the materials and in the emissions; the rule is division free (an all-zero material still gets the
gradient of its first vertex, and that is the one-bounce gradient); with one bounce the gradient does not depend on the materials; and
the margins table of the module is the measurement."""
import numpy as np
import pytest

import texel_bounce_cases as BC
import texel_bounce_grad_ref as GR

CASES = list(BC.CASES)
STEP = 1e-20


def _directional(name, rec, mats, emissions, j, flat, ch, g):
    """d/dm of sum(g x bake) in texel ``flat``, channel ``ch`` of material j (j = -1: in row ``flat`` of the emissions), by a complex step"""
    mats = [np.asarray(m, np.float64) for m in mats]
    em = None if emissions is None else np.asarray(emissions, np.float64)
    if j >= 0:
        mats[j] = mats[j].astype(np.complex128)
        mats[j].reshape(-1, 4)[flat, ch] += 1j * STEP
    else:
        em = em.astype(np.complex128)
        em[flat, ch] += 1j * STEP
    out = GR.bake_eval(rec, mats, em)
    return float((out.imag * g).sum() / STEP)


def _masked(name):
    g = GR.cotangent(name).astype(np.float64)[..., :3]
    return np.where(np.isnan(g), 0.0, g)


@pytest.mark.parametrize("name", CASES)
def test_evaluator_reproduces_the_bake(name):
    ref = BC.reference(name)
    out = GR.bake_eval(GR.reference_records(name), BC.materials(name))
    err, top = float(np.abs(out - ref["data"][..., :3]).max()), float(np.abs(ref["data"][..., :3]).max())
    print(f"[texel bounce grad] {name}: evaluator against the reference's bake: {err:.3e} of {top:.3e}")
    assert top > 0 and err <= 1e-12 * top
    # ... and with the emissions spelled out it is the same function
    arrays = BC.CASES[name][0]()
    em = np.asarray(arrays.inst_emission, np.float64).reshape(-1, 3)
    assert np.abs(GR.bake_eval(GR.reference_records(name), BC.materials(name), em) - out).max() <= 1e-14 * top


@pytest.mark.parametrize("name", CASES)
def test_gradient_is_the_complex_step_derivative(name):
    rec, mats, g = GR.reference_records(name), BC.materials(name), _masked(name)
    grad = GR.reference_grad(name)
    rng = np.random.default_rng(5)
    top = max(float(np.abs(d).max()) for d in grad["d_materials"])
    worst = 0.0
    for j, m in enumerate(mats):
        n = m.shape[0] * m.shape[1]
        texels = np.arange(n) if n <= 64 else rng.choice(n, 64, replace=False)
        assert np.abs(grad["d_materials"][j][..., :3]).max() > 0, f"material {j} has no gradient"
        assert (grad["d_materials"][j][..., 3] == 0).all()
        assert (grad["d_materials"][j][~grad["read"][j]] == 0).all()
        for t in texels:
            for ch in range(3):
                worst = max(worst, abs(_directional(name, rec, mats, None, j, int(t), ch, g) - grad["d_materials"][j].reshape(-1, 4)[t, ch]))
    print(f"[texel bounce grad] {name}: d_materials against the complex step: {worst:.3e} of {top:.3e}")
    assert worst <= 1e-9 * top
    arrays = BC.CASES[name][0]()
    em = np.asarray(arrays.inst_emission, np.float64).reshape(-1, 3)
    lights = GR.light_rows(name)
    etop, eworst = float(np.abs(grad["d_emission"]).max()), 0.0
    for i in range(arrays.ninst):
        for ch in range(3):
            d = _directional(name, rec, mats, em, -1, i, ch, g)
            eworst = max(eworst, abs(d - grad["d_emission"][i, ch]))
            if i not in lights:
                assert d == 0.0 and grad["d_emission"][i, ch] == 0.0
    print(f"[texel bounce grad] {name}: d_emission against the complex step: {eworst:.3e} of {etop:.3e}")
    assert eworst <= 1e-9 * max(etop, top)
    assert (etop > 0) == bool(lights)                                 # env_k2 has no mesh light: all zero


def test_zero_albedo_keeps_the_first_vertex():
    name = "cbox_k3"
    rec, g = GR.reference_records(name), _masked(name)
    zero = tuple(np.zeros_like(m) for m in BC.materials(name))
    grad = GR.texel_bounce_grad_ref(rec, zero, GR.cotangent(name))
    top = float(np.abs(grad["d_materials"][0]).max())
    assert top > 0 and np.isfinite(grad["d_materials"][0]).all()
    rng = np.random.default_rng(6)
    for t in rng.choice(zero[0].shape[0] * zero[0].shape[1], 64, replace=False):
        for ch in range(3):
            assert abs(_directional(name, rec, zero, None, 0, int(t), ch, g) - grad["d_materials"][0].reshape(-1, 4)[t, ch]) <= 1e-9 * top
    # the one-bounce gradient of the same case: the first vertex of the same walks
    ref = BC.reference(name)
    hits1 = {k: (ref[k] if k == "nvert" else ref[k][:, :1]) for k in ("nvert", "inst", "prim", "uv", "flags")}
    hits1["nvert"] = np.minimum(ref["nvert"], 1)
    one = GR.texel_bounce_grad_ref(GR.case_records(name, hits1, K=1), BC.materials(name), GR.cotangent(name))
    assert np.abs(one["d_materials"][0] - grad["d_materials"][0]).max() <= 1e-12 * top
    assert (grad["d_emission"] == 0).all()                            # (every beta_k is 0: no light's emission reaches a texel through a black wall)


def test_one_bounce_gradient_ignores_the_material_values():
    name = "cbox_k1"
    rec = GR.reference_records(name)
    a = GR.reference_grad(name)
    rng = np.random.default_rng(8)
    other = tuple(np.concatenate([rng.uniform(0.0, 1.0, m.shape[:2] + (3,)), m[..., 3:]], -1).astype(np.float32) for m in BC.materials(name))
    b = GR.texel_bounce_grad_ref(rec, other, GR.cotangent(name))
    assert all((x == y).all() for x, y in zip(a["d_materials"], b["d_materials"]))
    # (the emission gradient carries beta_1 and does depend on them)
    assert np.abs(a["d_emission"] - b["d_emission"]).max() > 0


@pytest.mark.parametrize("name", CASES)
def test_margins_table_is_the_measurement(name):
    (em, ee), (sm, se) = GR.margin(name)
    print(f"[texel bounce grad] {name}: float32 margin d_materials {em:.3e} (largest entry {sm:.3e}), d_emission {ee:.3e} (largest entry {se:.3e})")
    pm, pe = GR.MARGINS[name]
    assert em <= pm <= 1.02 * em + 1e-12, (em, pm)
    assert ee <= pe <= 1.02 * ee + 1e-12, (ee, pe)
