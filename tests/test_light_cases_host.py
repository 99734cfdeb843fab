"""CPU: the preconditions of tests/test_gpu_light_cases.py.  The float64 reference of tests/light_cases.py is pinned against the oracle's
copies of the light-side functions (IEEE and FMA build) and against its own float32 transcription, row by row, at the MEASURED margins;
K and KT are held to that measurement; the scene tables the reference reads are the oracle's bit for bit; the rows that the reference
alone leaves open are capped; the families are not hollow; and every deliberate mistake is rejected by the families that exercise it."""
import functools

import numpy as np
import pytest

import light_cases as lc

CASES = [(name, scene) for name, scenes in lc.PLAN for scene in scenes]


@functools.lru_cache(None)
def hits(name, scene):
    return lc.oracle_hits(scene, lc.family(name, scene)[1]) if name == "interact" else None


def open_share(name, scene):
    rows = lc.family(name, scene)[1]
    if name == "interact":                                     # its formulas decide nothing
        return 0.0, {}
    c, _ = lc.reference(name, scene)
    per = {s: int(np.broadcast_to(m, (len(rows),)).sum()) for s, m in c.open.items() if np.any(m)}
    any_open = np.zeros(len(rows), bool)
    for m in c.open.values():
        any_open |= np.broadcast_to(m, any_open.shape)
    return float(any_open.mean()), per


def test_the_margins_are_four_times_the_measured_floor():
    k, kt, lines = lc.measure_k()
    print("\n".join(lines))
    assert (k, kt) == (lc.K_MEASURED, lc.KT_MEASURED)
    assert lc.K == 4 * lc.K_MEASURED and lc.KT == 4 * lc.KT_MEASURED


@pytest.mark.parametrize("scene", ["cbox", "stage", "chandelier", "normals", "terrain"])
def test_the_scene_tables_are_the_oracles_bit_for_bit(scene):
    """world corners through zdro_surface_interact at the three corners of every triangle (w * p is exact for w in {0, 1}), and the
    geometric normal the IEEE build forms with the host's operations"""
    T = lc.tables(scene)
    S = lc.oracle_scene(scene)
    nt = T.P.shape[0]
    prim = np.arange(nt) - T.begin[T.tri_inst]
    for corner, (u, v) in enumerate(((0, 0), (1, 0), (0, 1))):
        q = np.zeros((nt, 16), np.float32)
        q[:, 0], q[:, 1], q[:, 2], q[:, 3] = T.tri_inst.astype(np.int32).view(np.float32), prim.astype(np.int32).view(np.float32), u, v
        o = S.light_rows("interact", q)
        assert np.array_equal(o[:, 0:3].view(np.uint32), T.P[:, corner].view(np.uint32)), corner
        assert np.array_equal(o[:, 3:5], T.UV[:, corner]), corner
        assert np.array_equal(o[:, 8:11].view(np.uint32), T.ng.view(np.uint32))


@pytest.mark.parametrize("name,scene", CASES)
def test_the_reference_agrees_with_the_oracle_and_its_transcription_on_every_row(name, scene):
    hit = hits(name, scene)
    for who in ("ieee", "fma", "f32"):
        got = lc.transcription(name, scene, hit=hit) if who == "f32" else lc.oracle_answers(name, scene, who, hit=hit)
        v = lc.judge(name, scene, got, hit=hit, k=lc.K_MEASURED, kt=lc.KT_MEASURED, computed_tables=who != "f32")
        v.assert_all_inside(f"{name}/{scene} {who}")


@pytest.mark.parametrize("name,scene", CASES)
def test_few_rows_are_open_by_the_reference_alone(name, scene):
    share, per = open_share(name, scene)
    print(f"[light] {name}/{scene}: open by the reference {share:.4f}  {per}")
    assert share <= lc.OPEN_CAP, per


@pytest.mark.parametrize("name,scene", CASES)
def test_only_poles_are_unbounded(name, scene):
    """An infinite bound is a pole of the formula, not a row set aside: the pdf of a mesh sample where cos_light's interval holds 0
    (origins in the light's plane, at its vertex, or at the sampled point: one row in eight by construction), 1 / sin(pi v) at v = 0
    and 1, atan2 on the polar axis, normalize(0).  Every other output of those rows is bounded, and nothing else is unbounded."""
    hit = hits(name, scene)
    v = lc.judge(name, scene, lc.transcription(name, scene, hit=hit), hit=hit)
    allowed = {"sample": {"pdf", "wi", "dist"}, "pdf": {"pdf", "pdf_wide"}, "env": {"duv", "pdf", "lookup", "back", "scale"}, "alias": {"pdf"},
               "misc": {"bh"}, "interact": {"ns"}}[name]
    for out, r in v.res.items():
        print(f"[light] {name}/{scene} {out}: bound infinite on {int(r[3].sum())} of {len(r[3])} rows")
        assert out in allowed or not r[3].any(), out
    cap = 0.25 if scene == "normals" else {"sample": 0.16, "pdf": 0.20}.get(name, 0.02)      # normals: 16 rows, two of them next to the vanishing normal on purpose
    assert v.unbounded.mean() <= cap, v.unbounded.mean()


def test_the_families_are_not_hollow():
    lit = dark = total = 0
    for scene in dict(lc.PLAN)["sample"]:
        c, ref = lc.reference("sample", scene)
        ev = np.stack([x.v for x in ref["eval"]], 1)
        rows = lc.family("sample", scene)[1]
        front_open = np.broadcast_to(c.open.get("front", False), (len(rows),))
        lit += int((ev != 0).any(1).sum()); dark += int(((ev == 0).all(1) & ~front_open).sum()); total += len(rows)
    print(f"[light] sample: eval != 0 on {lit / total:.3f}, eval = 0 by a decided margin on {dark / total:.3f}")
    assert lit >= 0.2 * total and dark >= 0.1 * total
    for scene in dict(lc.PLAN)["env"]:
        rows = lc.family("env", scene)[1]
        assert (rows[:, 0] < 0).mean() >= 0.4 and (rows[:, 0] > 0).mean() >= 0.4
    for name, scene, out in (("sample", "cbox", "eval"), ("sample", "quad_env", "env_uv"), ("sample", "quad_env", "eval"), ("alias", "quad_env", "env_uv"),
                             ("env", "quad_env", "lookup"), ("misc", "quad", "offset"), ("misc", "quad", "tri"), ("misc", "quad", "tent")):
        v = lc.judge(name, scene, lc.transcription(name, scene))
        exact = int(v.res[out][2].sum())
        print(f"[light] {name}/{scene} {out}: {exact} of {len(v.ok)} rows are exact (bit for bit)")
        assert exact >= 16, (name, scene, out)


@pytest.mark.parametrize("mut", sorted(lc.MUTATIONS))
def test_the_judge_rejects_the_wrong_restatement(mut):
    for name in lc.MUTATIONS[mut]:
        worst = 0
        for scene in dict(lc.PLAN)[name]:
            hit = hits(name, scene)
            v = lc.judge(name, scene, lc.transcription(name, scene, hit=hit, mut=mut), hit=hit)
            worst = max(worst, int((~v.ok).sum()))
            print(f"[light] {mut} in {name}/{scene}: {int((~v.ok).sum())} of {len(v.ok)} rows outside")
        assert worst > 0, (mut, name)


def test_less_or_equal_on_the_triangles_diagonal_is_the_same_function():
    """u.x <= u.y in place of u.x < u.y changes nothing: where they differ (u.x = u.y) both branches compute (u / 2, u / 2, 1 - u / 2 - u / 2)
    with the same operations.  So the comparison's strictness is not something a test can hold; the swapped branches are (MUTATIONS)."""
    for name, scene in (("sample", "cbox"), ("sample", "chandelier"), ("misc", "quad")):
        rows = lc.family(name, scene)[1]
        at = (8, 9) if name == "misc" else (5, 6)
        assert (rows[:, at[0]] == rows[:, at[1]]).sum() >= 8
        a, b = lc.transcription(name, scene), lc.transcription(name, scene, mut="tri_le")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
