"""The cases of tests/geometry_cases.py judged without a GPU: the float32 mirror of the plane records against the per-pair bounds of
tests/ray_cases.py on every pair, the mirrors of the two walks (test_bvh_emulation.traverse, test_brute_quads.emulate_quad_walk) against the
decided facts, the stack against what the builder reports, and the share of rays the reference decides by itself — what fails here does
not go to the GPU.  profiles/geometry_cases_margins.txt is the table these tests assert (python tests/geometry_cases.py)."""
import numpy as np
import pytest

import geometry_cases as gc
import ray_cases as rc
import test_brute_quads as bq
import test_bvh_emulation as emu


@pytest.mark.parametrize("name", gc.CASES)
def test_the_mirror_stays_within_its_own_bounds(name):
    """every pair with a finite bound, grazing ones included: |dt| <= Bt, |du| <= Bu, |dv| <= Bv"""
    b = gc.batch(name)
    rt, ru, rv, near = gc.mirror_ratios(b)
    print(f"{b}: worst |dt| / Bt {rt:.3f}, |du| / Bu {ru:.3f}, |dv| / Bv {rv:.3f}; worst barycentric error near a triangle {near:.3e}")
    assert rt <= 1.0 and ru <= 1.0 and rv <= 1.0, (name, rt, ru, rv)
    assert np.isfinite(b.ref.B[:, ~gc.zero_area(b.case)]).mean() > 0.99, name     # the bounds say something: next to no pair of a triangle with an area is without one
    assert max(rt, ru, rv) > 0.05, name                              # ... and are no orders of magnitude above what they bound


@pytest.mark.parametrize("name", gc.CASES)
def test_two_thirds_of_the_rays_are_decided_by_the_reference(name):
    b = gc.batch(name)
    print(f"{b}: decided {b.decided.mean():.3f} (hits {b.ref.decided_hit.mean():.3f}, misses {b.ref.decided_miss.mean():.3f})")
    assert len(b.case.tri) <= 802 and len(b.rays) == gc.N_AIMED + gc.N_RANDOM
    assert b.decided.mean() >= gc.CAP, (name, b.decided.mean())
    assert b.ref.decided_hit.mean() >= 0.3 and b.ref.decided_miss.mean() >= 0.1, name       # both kinds of answer are asked for
    assert b.case.A.ninst >= 2 and (b.case.A.inst_emission[-1] > 0).all() and not (b.case.A.inst_emission[:-1] > 0).any()
    light = np.arange(b.case.A.inst_tri_begin[-2], b.case.A.inst_tri_begin[-1])
    assert len(light) >= 2 and not gc.zero_area(b.case)[light].any()


def test_the_fixed_rule_fails_away_from_the_origin_and_the_per_pair_bound_does_not():
    """on the mirror: what the per-pair bounds are for"""
    for name in ("cbox+1000", "cbox+4096x", "soup+300"):
        old, new = gc.old_rule_ratio(gc.batch(name))
        assert old > 1.5 and new <= 1.0, (name, old, new)


def test_the_degenerate_triangles_are_exactly_degenerate_and_never_hit():
    b = gc.batch("degenerate")
    flat = gc.zero_area(b.case)
    assert flat.sum() == 60 and (b.case.rec_in[flat, 0:3] == 0).all() and (b.case.rec_in[~flat, 0:3] != 0).any(1).all()
    assert (b.ref.state[:, flat] == rc.MISS).all()                   # whoever names one of them is contradicted
    assert not gc.zero_area(gc.case("needles")).any()


def test_the_transformed_case_is_judged_on_world_corners():
    c = gc.case("transformed")
    M = c.A.inst_xform[0].reshape(4, 4).astype(np.float64)
    assert np.linalg.det(M[:3, :3]) < 0 and not np.allclose(M[:3, :3].T @ M[:3, :3], np.eye(3) * (M[:3, :3].T @ M[:3, :3])[0, 0])    # mirrored, not a similarity
    v = c.A.verts[c.A.tris][:, :, :3].astype(np.float64)
    assert np.abs(c.tri - (v @ M[:3, :3].T + M[:3, 3])).max() < 1e-5 and np.abs(c.tri - v).max() > 1.0


def test_the_per_pair_checks_reject_wrong_answers():
    b = gc.batch("soup+300")
    ref = b.ref
    k, t, (_, u, v, _) = rc.closest64(b.case.tri, b.rays)
    rows = np.arange(len(k)); kk = np.maximum(k, 0)
    uv = np.stack([u[rows, kk], v[rows, kk]], 1)
    tt = np.where(k >= 0, t, 0.0)
    assert not ref.check_closest(k, tt, uv) and not ref.check_any(k >= 0)                  # the reference itself is admissible
    hit, miss = np.nonzero(ref.decided_hit)[0], np.nonzero(ref.decided_miss)[0]
    assert len(hit) > 500 and len(miss) > 300
    wrong = k.copy(); wrong[hit] = -1
    assert set(hit) <= {i for i, _, _ in ref.check_closest(wrong, tt, uv)}                # a lost hit
    wrong = k.copy(); wrong[miss] = 5
    assert [i for i, _, _ in ref.check_closest(wrong, np.where(k >= 0, t, 1.0), uv)] == miss.tolist()     # an invented one
    B = ref.B[rows, kk].astype(np.float64)
    answered = np.nonzero((k >= 0) & np.isfinite(B))[0]
    assert set(answered) <= {i for i, _, _ in ref.check_closest(k, tt + 1.5 * B, uv)}     # t beyond its own bound
    off = uv.copy(); off[:, 0] += 1.5 * ref.bu[rows, kk]
    sure = hit[ref.state[hit, kk[hit]] == rc.HIT]
    assert set(sure) <= {i for i, _, _ in ref.check_closest(k, tt, off)}                  # u beyond its own bound
    assert not ref.check_closest(k, tt, off, rotated=True)                                 # ... which a rotated slot's report may use up
    assert [i for i, _, _ in ref.check_any((k >= 0) | np.isin(rows, miss))] == miss.tolist()
    must = np.nonzero((ref.state == rc.HIT).any(1))[0]
    assert [i for i, _, _ in ref.check_any((k >= 0) & ~np.isin(rows, must))] == must.tolist()


@pytest.mark.parametrize("name", ["cbox+1000", "transformed", "soup+300", "ground"])
def test_the_interpolated_hit_point_of_the_mirror_stays_within_its_bound(name):
    """surface_interact's p from the mirror's barycentrics: what tests/test_gpu_geometry_cases.py holds the kernels to"""
    worst, n = gc.mirror_interaction(gc.batch(name))
    print(f"{name}: {n} decided hits, worst |p - p64| / bound {worst:.3f}")
    assert n > 500 and 0.02 < worst <= 1.0, (name, worst)


def walk_subset(b):
    """every 25th ray, and the longest rays of the case (ground: across the plane)"""
    n = len(b.rays)
    with np.errstate(all="ignore"):
        reach = np.where(b.ref.decided_hit, b.ref.dec_t, 0.0)
    return np.unique(np.r_[np.arange(0, n, 25), np.argsort(reach)[-8:]])


@pytest.mark.parametrize("name", gc.CASES)
def test_the_bvh_walks_mirror_contradicts_no_decided_fact(name):
    b = gc.batch(name)
    c = b.case
    nodes, order, isect, stack = c.records
    emu.STACK = stack
    pick = walk_subset(b)
    tri, t, pend = [], [], []
    for r in b.rays[pick]:
        slot, tt, steps, p = emu.traverse(nodes, isect, r[0:3], r[4:7], r[3], r[7], False)     # asserts len(stack) + 4 <= STACK at every push
        assert steps <= 2 * (nodes.shape[0] + isect.shape[0]) + 8
        tri.append(order[slot] if slot >= 0 else -1); t.append(tt); pend.append(p)
    tri, pend = np.array(tri), np.array(pend)
    bad = b.ref.take(pick).check_closest(tri, np.array(t, np.float64))
    assert not bad, (name, len(bad), bad[:3])
    assert not gc.zero_area(c)[tri[tri >= 0]].any()
    occ = np.array([emu.traverse(nodes, isect, r[0:3], r[4:7], r[3], r[7], True)[0] >= 0 for r in b.rays[pick[::3]]])
    bad = b.ref.take(pick[::3]).check_any(occ)
    assert not bad, (name, len(bad), bad[:3])
    assert pend.max() + 4 <= stack or nodes.shape[0] == 0, (name, pend.max(), stack)            # the stack stays within what the builder reports
    print(f"{b}: {len(pick)} rays through the BVH mirror, {nodes.shape[0]} nodes, pending set up to {pend.max()} of {stack} entries, hits {(tri >= 0).mean():.2f}")


@pytest.mark.parametrize("name", [n for n in gc.CASES if "brute" in gc.case(n).accels])
def test_the_quad_walks_mirror_contradicts_no_decided_fact(name):
    b = gc.batch(name)
    nq, order, isect = bq.build(b.case.tri)
    tri, t = bq.emulate_quad_walk(nq, order, isect, b.rays)
    ref = b.ref_brute                                    # a quad's second triangle is tested with the plane of the first: the bounds say so
    bad = ref.check_closest(tri, t.astype(np.float64))
    assert not bad, (name, len(bad), bad[:3])
    assert (ref.decided_hit | ref.decided_miss).mean() >= gc.CAP
    bad = ref.check_any(tri >= 0)                        # the any-hit walk accepts what the closest-hit walk accepts
    assert not bad, (name, len(bad), bad[:3])
    print(f"{b}: {len(b.rays)} rays through the quad walk's mirror, {nq} quads ({bq.NPAR} parallelograms) among {len(order)} triangles, hits {(tri >= 0).mean():.2f}")
