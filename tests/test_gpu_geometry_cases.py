"""-m gpu: the ray queries on geometry like a mesh a user might bring — the cases of tests/geometry_cases.py (away from the origin, of mixed
scale, needles, duplicates, a shared centroid, an exactly flat grid, zero-area triangles, a mirrored non-uniformly scaled instance) through
zdr_trace_closest / zdr_trace_any, zdr_trace_fused in both LDS layouts, and surface_interact behind zdr_light_dump.  Every ray is judged by
the float64 reference under the PER-PAIR bounds of tests/ray_cases.py (operation counts, checked on the CPU mirrors by
tests/test_geometry_cases_host.py): no share of the rays is set aside, and no constant here comes from what a GPU returned."""
import functools

import numpy as np
import pytest
import torch

import geometry_cases as gc
import ray_cases as rc
from gpu_util import make_scene
from test_gpu_ray_cases import closest, fused_against_plain, none_bad, occluded

pytestmark = pytest.mark.gpu
PAIRS = [(name, accel) for name in gc.CASES for accel in gc.case(name).accels]
BVH_CASES = [name for name in gc.CASES if "bvh" in gc.case(name).accels]


@functools.lru_cache(None)
def scene_of(name, accel):
    s = make_scene("path", arrays=gc.case(name).A, accel=accel)
    assert s.info()["accel"] == accel
    return s


# ------------------------------------------------------------------------------ a. walk<> against float64
@pytest.mark.parametrize("name,accel", PAIRS)
def test_every_ray_of_the_case_is_admissible(name, accel):
    b = gc.batch(name)
    c, ref = b.case, b.ref_of(accel)
    scene = scene_of(name, accel)
    if accel == "bvh" and len(c.tri) > 4:
        assert scene.info()["bvh_stack_entries"] == c.records[3]         # the tree the host tests walked
    ip, bt = closest(scene, b.rays)
    tri = c.tri_of(ip)
    none_bad(ref.check_closest(tri, bt[:, 2], bt[:, :2], rotated=accel == "brute"), f"{b} {accel} closest")
    miss = ip[:, 0] < 0
    assert np.array_equal(bt[miss], np.stack([np.zeros(miss.sum(), np.float32)] * 2 + [b.rays[miss, 7]], 1)), (b, accel)   # a miss reports (0, 0, tmax)
    assert not gc.zero_area(c)[tri[~miss]].any(), (b, accel)             # no answer names a triangle without area
    assert (~miss)[ref.decided_hit].all() and miss[ref.decided_miss].all()
    none_bad(ref.check_any(occluded(scene, b.rays)), f"{b} {accel} any")
    rows, k = np.nonzero(~miss)[0], tri[~miss]           # for the record (-s): how much of its bounds the kernel uses; asserted above
    with np.errstate(all="ignore"):
        rt = np.abs(bt[rows, 2] - ref.t[rows, k]) / ref.B[rows, k]
        sure = ref.state[rows, k] == rc.HIT
        ru = np.maximum(np.abs(bt[rows, 0] - ref.u[rows, k]) / ref.bu[rows, k], np.abs(bt[rows, 1] - ref.v[rows, k]) / ref.bv[rows, k])[sure]
    print(f"[geometry] {b} {accel}: hits {(~miss).mean():.3f}, decided by the reference {(ref.decided_hit | ref.decided_miss).mean():.3f}, every ray admissible; "
          f"worst |dt| / Bt {np.nanmax(rt):.3f}, worst |du|, |dv| / Bu, Bv {np.nanmax(ru):.3f}{' (unrotated bounds)' if accel == 'brute' else ''}")


def test_brute_force_and_bvh_agree_bit_for_bit_without_quads_away_from_the_origin(monkeypatch):
    """One primitive per triangle (ZDR_NO_QUADS=1): the same records through the same fmaf order — at (1000, 1000, 1000) as at the origin
    (tests/test_gpu_ray_cases.py)."""
    b = gc.batch("cbox+1000")
    monkeypatch.setenv("ZDR_NO_QUADS", "1")
    brute = make_scene("path", arrays=b.case.A, accel="brute")
    monkeypatch.delenv("ZDR_NO_QUADS")
    ipa, bta = closest(brute, b.rays)
    ipb, btb = closest(scene_of("cbox+1000", "bvh"), b.rays)
    none_bad(b.ref.check_closest(b.case.tri_of(ipa), bta[:, 2], bta[:, :2]), f"{b} brute without quads")     # no quad, no rotation: the BVH's bounds
    same = (ipa == ipb).all(1)
    assert np.array_equal(bta[same].view(np.uint32), btb[same].view(np.uint32)), b
    assert same[~b.ref.has_open].all(), b                # another primitive only where the reference leaves the answer open
    print(f"[geometry] {b}: same primitive on {same.mean():.4f}, t and barycentrics equal bit for bit there")


# -------------------------------------------------------------------- b. walk_steal against walk<> and float64
def waves_of(name, seed=11):
    """(shadow, next, need) of 16 whole waves of the case's own rays: 256 distinct ray pairs, 64 of them per wave in a seeded order with
    seeded need bits.  ground: two more waves in which eight lanes own rays that cross the 2e4-wide plane and the others short ones — the
    short lanes finish and steal."""
    b = gc.batch(name)
    rng = np.random.default_rng(seed)
    pool = b.rays
    ps, pn = pool[rng.choice(len(pool), 256, replace=False)], pool[rng.choice(len(pool), 256, replace=False)]
    s, n, need = [], [], []
    for w in range(16):
        pick = rng.choice(256, 64, replace=False)
        s.append(ps[pick]); n.append(pn[pick]); need.append(rng.integers(0, 4, 64))
    if name == "ground":
        reach = np.where(b.ref.decided_hit & (b.rays[:, 7] > 1e29), b.ref.dec_t, np.nan)
        long_rays, short_rays = b.rays[reach > 3000.0], b.rays[reach < 100.0]          # (the nearest origin is 1e-3 diagonals = 28 units away)
        assert len(long_rays) >= 16 and len(short_rays) >= 100
        for w in range(2):
            ws, wn = short_rays[rng.choice(len(short_rays), 64)], short_rays[rng.choice(len(short_rays), 64)]
            for l in (3, 11, 20, 29, 37, 44, 54, 62):
                ws[l], wn[l] = long_rays[rng.integers(len(long_rays))], long_rays[rng.integers(len(long_rays))]
            s.append(ws); n.append(wn); need.append(np.full(64, 3))
    need = np.concatenate(need).astype(np.int32)
    assert all((need == k).sum() > 150 for k in range(4))
    return np.concatenate(s), np.concatenate(n), need


@pytest.mark.parametrize("backward", [False, True], ids=["forward-layout", "backward-layout"])
@pytest.mark.parametrize("name", BVH_CASES)
def test_the_fused_walk_answers_as_the_plain_walk(name, backward):
    c = gc.case(name)
    shadow, nxt, need = waves_of(name)
    what = f"{name} ({'backward' if backward else 'forward'} layout)"
    occ, ip, bt, differ = fused_against_plain(scene_of(name, "bvh"), c, shadow, nxt, need, backward, what)
    tri = c.tri_of(ip)
    assert not gc.zero_area(c)[tri[tri >= 0]].any(), what
    print(f"[geometry fused] {what}: {len(need)} lanes in {len(need) // 64} waves, {differ} continuation rays on another primitive at a bit-equal t, "
          f"every lane equal to the plain walk and admissible")


# ----------------------------------------------------------------------------------- c. surface interaction
@pytest.mark.parametrize("name,accel", [(n, a) for n in ("cbox+1000", "transformed") for a in ("brute", "bvh")])
def test_surface_interaction_reports_the_world_point_and_normal(name, accel):
    """ZDR_LIGHT_INTERACT: the hit as zdr_trace_closest reports it, p within the bound of geometry_cases.interaction_facts of the float64 hit
    point, ng the float64 normal of the WORLD triangle with the sign of the world corners' winding — through a mirrored instance too."""
    b = gc.batch(name)
    c, ref = b.case, b.ref_of(accel)
    scene = scene_of(name, accel)
    rows = np.zeros((len(b.rays), 16), np.float32)
    rows[:, 0:3] = b.rays[:, 0:3]; rows[:, 3:6] = b.rays[:, 4:7]; rows[:, 6] = b.rays[:, 3]; rows[:, 7] = b.rays[:, 7]
    o = scene.light_dump("interact", torch.from_numpy(rows))
    scene.check()
    o = o.cpu().numpy()
    ip = np.stack([o[:, 0].view(np.int32), o[:, 1].view(np.int32)], 1)
    pip, pbt = closest(scene, b.rays)
    assert np.array_equal(ip, pip) and np.array_equal(o[:, 4].view(np.uint32), pbt[:, 2].view(np.uint32))      # the walk of zdr_trace_closest (its barycentrics are judged below)
    tri = c.tri_of(ip)
    none_bad(ref.check_closest(tri, o[:, 4], o[:, 2:4], rotated=accel == "brute"), f"{b} {accel} interact")
    sure = np.nonzero((tri >= 0) & (ref.state[np.arange(len(tri)), np.maximum(tri, 0)] == rc.HIT))[0]
    assert len(sure) > 1000
    p64, pb, n64, nb = gc.interaction_facts(ref, sure, tri[sure], rotated=accel == "brute")
    rp = gc.ratio(np.abs(o[sure, 5:8].astype(np.float64) - p64), pb)
    rn = np.abs(o[sure, 13:16].astype(np.float64) - n64) / nb[:, None]
    print(f"[geometry interact] {b} {accel}: {len(sure)} decided hits, worst |p - p64| / bound {rp.max():.3f}, worst |ng - n64| / bound {rn.max():.3f}")
    assert rp.max() <= 1.0, (name, accel, rp.max(), sure[rp.max(1).argmax()])
    assert rn.max() <= 1.0, (name, accel, rn.max(), sure[rn.max(1).argmax()])
    if name == "transformed":                            # the object-space winding is the opposite one: a normal from object space would fail above
        v = c.A.verts[c.A.tris][:, :, :3].astype(np.float64)
        M = c.A.inst_xform[0].reshape(4, 4).astype(np.float64)[:3, :3]
        n_obj = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) @ np.linalg.inv(M)          # inverse-transpose applied to the object-space normal
        n_obj /= np.linalg.norm(n_obj, axis=1, keepdims=True)
        assert ((n_obj[tri[sure]] * n64).sum(1) < -0.999).all()
