"""The ray families of tests/ray_cases.py judged without a GPU: the float64 reference against the oracle, the conditions that keep
the families from going hollow, the barycentric margin against its measurement, and the CPU mirror of the BVH walk
(tests/test_bvh_emulation.py) on a subset of every family — what fails here does not go to the GPU."""
import numpy as np
import pytest

import ray_cases as rc
import test_bvh_emulation as emu
from zdr_amd.scenes import random_rays


def test_float64_reference_agrees_with_the_oracle(cbox_oracle):
    """2,000 random Cornell box rays: the new reference against the oracle's float32 Moeller-Trumbore, held to the bounds of
    tests/test_gpu_trace.py, check_closest."""
    c = rc.case("cbox")
    rays = random_rays(2000, (-3, 0, -5.5), (2.5, 5.2, 6), seed=21)
    rip, rbt = cbox_oracle.trace_closest(rays)
    k, t, (_, u, v, _) = rc.closest64(c.tri, rays)
    hit_o, hit_r = rip[:, 0] >= 0, k >= 0
    assert (hit_o != hit_r).mean() < 2e-4
    both = hit_o & hit_r
    same = c.tri_of(rip)[both] == k[both]
    assert (~same).mean() < 2e-4
    ok = both.copy(); ok[both] = same
    rows = np.nonzero(ok)[0]
    terr = np.abs(rbt[ok, 2] - t[ok]) / (1e-5 * np.abs(t[ok]) + 5e-6)
    berr = np.maximum(np.abs(rbt[ok, 0] - u[rows, k[ok]]), np.abs(rbt[ok, 1] - v[rows, k[ok]]))
    assert (terr > 1).mean() < 2e-4 and terr.max() < 50, (terr.max(), (terr > 1).mean())
    assert (berr > 1e-4).mean() < 2e-4 and berr.max() < 5e-3, (berr.max(), (berr > 1e-4).mean())
    occ, _ = rc.any64(c.tri, rays)
    assert np.array_equal(occ, hit_r)
    rays[:, 3] = 1e-4; rays[:, 7] = np.random.default_rng(22).uniform(0.1, 6.0, len(rays)).astype(np.float32)
    assert (rc.any64(c.tri, rays)[0] != (cbox_oracle.trace_any(rays) != 0)).mean() < 2e-4


def test_the_families_are_not_hollow():
    stats = rc.family_stats()
    print(stats)
    for family, (n, open_share, hits, misses, dropped) in stats.items():
        assert n >= 150, family
        assert dropped <= 0.1 * n, (family, dropped)                 # the grazing filter takes a few rays out, not a family
        if family != "nonfinite":
            assert hits >= 0.20 and misses >= 0.10, (family, hits, misses)
        if family in ("axis", "tower"):
            assert open_share <= 0.01, (family, open_share)
    for b in rc.batches():
        assert not b.ref.grazing.any(), b                            # every pair that may count is held to the t bound as it stands
        if b.family == "nonfinite":
            assert b.ref.decided_miss.all(), b                       # expected: miss, not occluded
        if b.family == "features":
            exact, near, far, cut = (b.tags == k for k in (0, 3, 2, 4))
            assert exact.sum() >= 100 and near.sum() >= 400 and far.sum() >= 400 and cut.sum() >= 200, b
            assert b.ref.has_open[exact].all(), b                    # the exact rays are open: that is their purpose
            assert b.ref.has_open[near | far].mean() <= 0.01, (b, b.ref.has_open[near | far].mean())
            assert b.ref.has_open[near].mean() <= 0.01, (b, b.ref.has_open[near].mean())   # +-1e-3 of the feature's size still resolves to a side
    # quads: the Cornell box has merged quads, and their diagonals are among the features
    assert sum(kind == "diagonal" for _, _, _, kind in rc.features_of(rc.case("cbox"))) == 3 * 15      # 15 quads (csrc/accel.h)


def test_the_barycentric_margin_is_four_times_the_mirrors_error():
    m = rc.measure_margin()
    near, everywhere = max(v[0] for v in m.values()), max(v[1] for v in m.values())
    print(f"mirror32 against float64: {near:.3e} on pairs with |u|, |v| <= {rc.NEAR:g}, {everywhere:.3e} on all; margin {rc.BARY_MARGIN:.3e}")
    assert 4 * near <= rc.BARY_MARGIN <= 5 * near
    assert everywhere < 1e-3                                         # a pair beyond NEAR is outside by 1/2: no error of this size changes that
    assert rc.BARY_MARGIN < 0.1 * 1e-3 * np.sin(0.37)                # the +-1e-3 companions sit at least ten margins off their feature


def test_the_checks_reject_wrong_answers():
    """check_closest / check_any on answers made wrong on purpose: a test that accepts everything proves nothing."""
    b = next(b for b in rc.batches() if b.family == "intervals" and b.scene == "cbox")
    ref = b.ref
    k, t, (_, u, v, _) = rc.closest64(b.case.tri, b.rays)
    rows = np.arange(len(k)); kk = np.maximum(k, 0)
    uv = np.stack([u[rows, kk], v[rows, kk]], 1)
    assert not ref.check_closest(k, np.where(k >= 0, t, 0.0), uv) and not ref.check_any(k >= 0)       # the reference itself is admissible
    hit = np.nonzero(ref.decided_hit)[0]; miss = np.nonzero(ref.decided_miss)[0]
    assert len(hit) > 100 and len(miss) > 100
    wrong = k.copy(); wrong[hit] = -1
    assert [i for i, _, _ in ref.check_closest(wrong, t, uv)] == hit.tolist()                          # a lost hit
    wrong = k.copy(); wrong[miss] = 5
    assert [i for i, _, _ in ref.check_closest(wrong, np.where(k >= 0, t, 1.0), uv)] == miss.tolist()  # an invented hit
    off = np.where(k >= 0, t + 3e-5 * np.abs(t) + 1e-5, 0.0)
    assert [i for i, _, _ in ref.check_closest(k, off, uv)] == np.nonzero(k >= 0)[0].tolist()          # t beyond its bound
    assert [i for i, _, _ in ref.check_closest(k, np.where(k >= 0, t, 0.0), uv + 3e-5)] == hit.tolist()   # barycentrics beyond the margin
    behind = np.where(np.isin(rows, hit), np.where(ref.state == rc.HIT, ref.t, -np.inf).argmax(1), k)   # the FARTHEST decided hit instead of the nearest
    moved = hit[behind[hit] != k[hit]]
    assert len(moved) > 20 and set(moved) <= {i for i, _, _ in ref.check_closest(behind, ref.t[rows, np.maximum(behind, 0)])}
    truth = k >= 0
    assert [i for i, _, _ in ref.check_any(truth | np.isin(rows, miss))] == miss.tolist()                # an invented occluder
    assert [i for i, _, _ in ref.check_any(truth & ~np.isin(rows, hit))] == hit.tolist()                 # a lost one


def emulate(c, rays, any_hit=False):
    nodes, order, isect, stack = c.records
    emu.STACK = stack
    tri, t, pend = [], [], []
    for r in rays:
        slot, tt, steps, p = emu.traverse(nodes, isect, r[0:3], r[4:7], r[3], r[7], any_hit)     # raises when the trip budget fires or a child word leaves the allocation
        assert steps <= 2 * (nodes.shape[0] + isect.shape[0]) + 8
        tri.append(order[slot] if slot >= 0 else -1); t.append(tt); pend.append(p)
    return np.array(tri), np.array(t, np.float64), np.array(pend)


@pytest.mark.parametrize("i", range(len(rc.PLAN)))
def test_the_walks_mirror_gives_admissible_answers(i):
    family = rc.PLAN[i][0]
    for b in [b for b in rc.batches() if b.family == family]:
        n = len(b.rays)
        if family == "nonfinite":
            pick = np.arange(n)
        elif family == "tower":        # the long rays, then the rays at (0.9, 0.9) and at (0.2, 0.2) from every origin, every other tilt
            pick = np.r_[0, 1, 2:52:2, 402:452:2]
        else:
            pick = np.unique(np.linspace(0, n - 1, 40).astype(int))
        ref = b.ref.take(pick)
        tri, t, pend = emulate(b.case, b.rays[pick])
        bad = ref.check_closest(tri, t)
        assert not bad, (b, len(bad), bad[:3])
        occ, _, _ = emulate(b.case, b.rays[pick[::4]], any_hit=True)
        bad = b.ref.take(pick[::4]).check_any(occ >= 0)
        assert not bad, (b, len(bad), bad[:3])
        print(f"{b}: {len(pick)} rays through the mirror, pending set up to {pend.max()}")
        if b.scene == "tower" and family == "tower":
            assert pend[:2].min() > 12 and pend.max() > 12, pend.max()          # beyond the LDS part of either layout (12 and 10)
        if b.scene == "tower64":
            assert pend.max() <= 10, pend.max()                                 # the control stays inside it
