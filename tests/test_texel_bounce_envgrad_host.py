"""The reference of the bounced light's adjoint in the environment map (tests/texel_bounce_envgrad_ref.py) and its cases
(tests/texel_bounce_env_cases.py), pinned on the CPU: the evaluator with the scene's own map is the forward reference's bake, the gradient
is the evaluator's exact directional derivative (the bake is linear in the map), alpha and unread texels are exactly 0, the cases meet
the conditions the GPU tests rely on — enough accepted environment samples at the first and at later vertices, lanes of one wave that
share a cell, more distinct cells than merge rounds, a footprint clamped at the map's border — the MARGINS table is reproduced, and the
new entry points are declared and bound.  No GPU needed."""
import re

import numpy as np
import pytest

import texel_bounce_env_cases as EC
import texel_bounce_envgrad_ref as ER
from zdr_amd import _native

CASES = list(EC.CASES)


def test_the_entry_points_are_declared_and_bound():
    hdr = open(_native.HERE + "/../include/zdr.h").read()
    for sym in ("zdr_texel_bounce_backward_env_workspace_bytes", "zdr_scene_texel_bounce_backward_env"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in _native.EXPORTS and getattr(_native.lib(), sym).argtypes is not None
    assert "Not differentiated: the environment map" not in hdr
    assert _native.lib().zdr_texel_bounce_backward_env_workspace_bytes(12, 12) == 16 + 4 * 144
    assert _native.lib().zdr_texel_bounce_backward_env_workspace_bytes(0, 12) == 0
    assert _native.ABI_VERSION == 4 and _native.lib().zdr_abi_version() == 4


def test_the_merge_rounds_are_the_headers():
    src = open(_native.HERE + "/csrc/bakegrad.h").read()
    assert re.search(r"#define ZDR_LGRAD_MERGE_ROUNDS %d\b" % EC.MERGE_ROUNDS, src)


@pytest.mark.parametrize("name", CASES)
def test_the_evaluator_with_the_scenes_map_is_the_forward_references_bake(name):
    rec = ER.reference_records(name)
    got = ER.bake_eval(rec, EC.materials(name), EC.env(name)[0])
    want = EC.reference(name)["data"][..., :3]
    off = float(np.abs(got - want).max())
    print(f"[texel bounce envgrad host] {name}: evaluator against the forward reference: {off:.3e} (largest irradiance {float(want.max()):.3e})")
    assert want.max() > 0 and off <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_the_gradient_is_the_evaluators_directional_derivative(name):
    rec, grad = ER.reference_records(name), ER.reference_grad(name)
    g = np.nan_to_num(ER.cotangent(name).astype(np.float64)[..., :3], nan=0.0)
    env = EC.env(name)[0].astype(np.float64)
    base = ER.bake_eval(rec, EC.materials(name), env)
    for seed in range(3):
        delta = np.zeros_like(env)
        delta[..., :3] = np.random.default_rng(40 + seed).uniform(-1.0, 1.0, env.shape[:2] + (3,))
        lhs = float((g * (ER.bake_eval(rec, EC.materials(name), env + delta) - base)).sum())
        rhs = float((grad["d_env"][..., :3] * delta[..., :3]).sum())
        print(f"[texel bounce envgrad host] {name} direction {seed}: <d_out, eval(env + d) - eval(env)> = {lhs:.12e}, <d_env, d> = {rhs:.12e}, differ by {abs(lhs - rhs):.3e}")
        assert abs(lhs - rhs) <= 1e-9
        assert abs(rhs) > 0


@pytest.mark.parametrize("name", CASES)
def test_alpha_and_unread_texels_are_exactly_zero(name):
    grad = ER.reference_grad(name)
    assert (grad["d_env"][..., 3] == 0).all()
    assert (grad["d_env"][~grad["read"]] == 0).all()
    assert grad["read"].any() and (~grad["read"]).any()
    assert np.isfinite(grad["d_env"]).all()


@pytest.mark.parametrize("name", CASES)
def test_condition_1_enough_accepted_environment_samples(name):
    acc = ER.accepted_env(ER.reference_records(name)).sum(0)
    k1 = EC.VERTEX_OF_CONDITION_1.get(name, 0)
    print(f"[texel bounce envgrad host] {name}: accepted environment samples per vertex {[int(v) for v in acc]}")
    assert acc[k1] >= 8
    if EC.case(name)["K"] >= 2:
        assert acc[1:].max() >= 8


def test_the_counts_of_the_shared_cases_are_the_issues():
    rec = ER.reference_records("env_k2")
    assert rec["shaded"].shape[0] == 484 and [int(v) for v in ER.accepted_env(rec).sum(0)] == [80, 30]
    lit = ER.reference_records("env_lit_k2")
    acc = ER.accepted_env(lit)
    assert int(acc[:, 1].sum()) == 26 and int((lit["added"][:, 1] & ~acc[:, 1]).sum()) == 29


@pytest.mark.parametrize("name", ["env_wave", "env_wave_ragged"])
def test_condition_2_lanes_of_one_wave_share_a_cell(name):
    rec = ER.reference_records(name)
    groups = ER.wave_groups(rec, name)
    shared = max(g[2] for g in groups)
    n_env, n_groups = int(ER.accepted_env(rec).sum()), ER.expected_groups(rec, name)
    print(f"[texel bounce envgrad host] {name}: lanes shift {EC.lanes_shift(name)}, at most {shared} lanes of a wave in one cell; {n_env} samples in {n_groups} groups")
    assert shared >= 2 and n_groups < n_env
    assert EC.lanes_shift(name) == (6 if name == "env_wave" else 5)
    if name == "env_wave_ragged":                                     # two texels per wave and an odd number of texels; two trips, the second ragged
        assert len(rec["ys"]) % 2 == 1 and rec["ns"] == 37


def test_condition_3_more_distinct_cells_than_merge_rounds():
    rec = ER.reference_records("env_sky")
    groups = ER.wave_groups(rec, "env_sky")
    most = max(g[1] for g in groups)
    print(f"[texel bounce envgrad host] env_sky: at most {most} distinct cells at one vertex index of one wave (merge rounds: {EC.MERGE_ROUNDS})")
    assert most > EC.MERGE_ROUNDS
    assert EC.lanes_shift("env_sky") == 6                             # a wave is a texel: the count does not depend on the list's order


def test_condition_4_a_footprint_is_clamped_at_a_border():
    found = {}
    for name in CASES:
        rec = ER.reference_records(name)
        _, cx, cy = ER.cells(rec)
        acc = ER.accepted_env(rec)
        ew = rec["env_shape"][1]
        n = int((acc & ((cx == -1) | (cx == ew - 1) | (cy == -1))).sum())
        if n:
            found[name] = n
    print(f"[texel bounce envgrad host] accepted samples with a footprint clamped at the map's border: {found}")
    assert found


def test_the_margins_table_is_reproduced():
    assert sorted(ER.MARGINS) == sorted(CASES)
    for name in CASES:
        e, s = ER.margin(name)
        print(f"[texel bounce envgrad host] {name}: float32 against float64 {e:.3e} (table {ER.MARGINS[name]:.3e}), largest entry {s:.3e}, bar {ER.bar(name):.3e}")
        assert e <= ER.MARGINS[name] <= 1.01 * e + 1e-12, (name, e)


def test_the_profile_holds_the_table():
    text = open(_native.HERE + "/../profiles/texel_bounce_envgrad_margins.txt").read()
    for name in CASES:
        assert re.search(r"^\s+%s\s" % name, text, re.M), name
