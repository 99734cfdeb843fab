"""-m gpu: the BVH walks ray by ray.  The families of tests/ray_cases.py — zero direction components, origins on box planes, rays inside a
triangle's plane, through corners, edges and quad diagonals, intervals closing around the hit, the tower whose rays outgrow the LDS
part of the traversal stack, NaNs and infinities — through zdr_trace_closest / zdr_trace_any (walk<>) and through zdr_trace_fused
(shadow_and_closest -> walk_steal, in waves composed so that lanes steal from each other), every ray judged by the float64 reference:
no share of the rays is set aside."""
import functools

import numpy as np
import pytest
import torch

import ray_cases as rc
from gpu_util import make_scene
from zdr_amd import _native

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def scene_of(name, accel):
    s = make_scene("path", arrays=rc.case(name).A, accel=accel)
    assert s.info()["accel"] == accel
    return s


def closest(scene, rays):
    ip, bt = scene.trace_closest(torch.from_numpy(np.ascontiguousarray(rays)))
    scene.check()                                        # no watchdog fired: the walk ended by itself
    return ip.cpu().numpy(), bt.cpu().numpy()


def occluded(scene, rays):
    occ = scene.trace_any(torch.from_numpy(np.ascontiguousarray(rays)))
    scene.check()
    return occ.cpu().numpy()


def none_bad(bad, what):
    assert not bad, (what, f"{len(bad)} answers contradict the float64 reference", bad[:4])


# ------------------------------------------------------------------------------ a. walk<> against float64
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_every_ray_of_the_family_is_admissible(family):
    for b in [b for b in rc.batches() if b.family == family]:
        for accel in b.case.accels:
            scene = scene_of(b.scene, accel)
            ip, bt = closest(scene, b.rays)
            none_bad(b.ref.check_closest(b.case.tri_of(ip), bt[:, 2], bt[:, :2]), f"{b} {accel} closest")
            miss = ip[:, 0] < 0
            assert np.array_equal(bt[miss], np.stack([np.zeros(miss.sum(), np.float32)] * 2 + [b.rays[miss, 7]], 1)), (b, accel)   # a miss reports (0, 0, tmax)
            none_bad(b.ref.check_any(occluded(scene, b.rays)), f"{b} {accel} any")
            print(f"[rays] {b} {accel}: hits {(~miss).mean():.3f}, every ray admissible")


def test_brute_force_and_bvh_agree_bit_for_bit_without_quads(monkeypatch):
    """One primitive per triangle (ZDR_NO_QUADS=1): the same records through the same fmaf order, only the culling differs — on the
    rays that random draws never produce as well (tests/test_gpu_trace.py, test_bvh_equals_brute_on_the_gpu, states it for random rays)."""
    monkeypatch.setenv("ZDR_NO_QUADS", "1")
    brute = make_scene("path", arrays=rc.case("cbox").A, accel="brute")
    monkeypatch.delenv("ZDR_NO_QUADS")
    bvh = scene_of("cbox", "bvh")
    for b in [b for b in rc.batches() if b.scene == "cbox"]:
        ipa, bta = closest(brute, b.rays)
        ipb, btb = closest(bvh, b.rays)
        none_bad(b.ref.check_closest(b.case.tri_of(ipa), bta[:, 2], bta[:, :2]), f"{b} brute without quads")
        same = (ipa == ipb).all(1)
        assert np.array_equal(bta[same].view(np.uint32), btb[same].view(np.uint32)), b
        assert same[~b.ref.has_open].all(), b            # another primitive only where the reference leaves the answer open
        print(f"[rays] {b}: same primitive on {same.mean():.4f}, t and barycentrics equal bit for bit there")


# -------------------------------------------------------------------- b. walk_steal against walk<> and float64
def fused_against_plain(scene, c, shadow, nxt, need, backward, what):
    """One zdr_trace_fused call against zdr_trace_any / zdr_trace_closest of the same rays, lane by lane, and against float64."""
    shadow, nxt, need = np.ascontiguousarray(shadow, np.float32), np.ascontiguousarray(nxt, np.float32).copy(), np.ascontiguousarray(need, np.int32)
    occ, ip, bt = scene.trace_fused(torch.from_numpy(shadow), torch.from_numpy(nxt), torch.from_numpy(need), backward_layout=backward)
    scene.check()
    occ, ip, bt = occ.cpu().numpy(), ip.cpu().numpy(), bt.cpu().numpy()
    nxt[:, 3] = 0.0; nxt[:, 7] = 1e30                    # as the path kernels pass them
    a, b = (need & 1) != 0, (need & 2) != 0
    pocc = occluded(scene, shadow)
    pip, pbt = closest(scene, nxt)
    lanes = lambda m: (what, "lanes", np.nonzero(m)[0][:8].tolist())
    assert not (occ[~a] != 0).any(), lanes(occ != 0)
    assert np.array_equal(occ[a] != 0, pocc[a] != 0), lanes(a & ((occ != 0) != (pocc != 0)))
    assert (ip[~b] == -1).all() and np.array_equal(bt[~b], np.tile(np.float32([0, 0, 1e30]), ((~b).sum(), 1))), what
    tbits = bt[:, 2].view(np.uint32) != pbt[:, 2].view(np.uint32)
    assert not (b & tbits).any(), (lanes(b & tbits), bt[b & tbits][:4], pbt[b & tbits][:4])
    differ = b & ((ip != pip).any(1) | (bt.view(np.uint32) != pbt.view(np.uint32)).any(1))
    assert not (differ & (ip == pip).all(1)).any(), lanes(differ)         # same primitive: same barycentrics, bit for bit
    # ... another primitive at the very same t (min over {t, record} against first found): both must be admissible — as every answer must
    rs, rows_s = rc.ref_of_distinct(c, shadow[a])
    none_bad(rs.check_any(occ[a], rows_s), f"{what}: fused shadow rays")
    rn, rows_n = rc.ref_of_distinct(c, nxt[b])
    none_bad(rn.check_closest(c.tri_of(ip[b]), bt[b, 2], bt[b, :2], rows_n), f"{what}: fused continuation rays")
    none_bad(rn.check_closest(c.tri_of(pip[b]), pbt[b, 2], pbt[b, :2], rows_n), f"{what}: plain walk of the continuation rays")
    return occ, ip, bt, int(differ.sum())


def finite_pool(scene_name):
    return np.concatenate([b.rays for b in rc.batches() if b.scene == scene_name and b.family != "nonfinite"])


def waves_of(scene_name, seed=7):
    """The wave compositions: [(name, shadow (64 k, 8), next (64 k, 8), need (64 k))], k whole waves each."""
    c = rc.case(scene_name)
    rng = np.random.default_rng(seed)
    tower = scene_name.startswith("tower")
    pool = finite_pool(scene_name)
    filler = pool[0]
    out = []
    def wave(name, lanes):                               # lanes: {lane: (shadow or None, next or None)}; the others have need = 0
        s, n, need = np.tile(filler, (64, 1)), np.tile(filler, (64, 1)), np.zeros(64, np.int32)
        for l, (a, b) in lanes.items():
            if a is not None: s[l] = a; need[l] |= 1
            if b is not None: n[l] = b; need[l] |= 2
        out.append((name, s, n, need))
    if tower:
        up, down = rc.tower_long_ray(c), rc.tower_long_ray(c, True)          # into the cap at the far end / through the whole tower, hitting nothing
        for l in (0, 31, 63):                            # 63 thieves from the first steal trip on; a thief finds the hit
            wave(f"one owner in lane {l}", {l: (None, up)})
        short = up.copy(); short[7] = 42.5               # the cap is at t = 43
        wave("shadow ray only, blocked by the cap", {0: (up, None)})
        wave("shadow ray only, ending short of the cap", {0: (short, None)})
        wave("both rays in one lane: miss, then cap", {5: (down, up)})
        wave("both rays in one lane: cap, then miss", {5: (up, down)})
        fam = next(b.rays for b in rc.batches() if b.scene == scene_name and b.family == "tower")
        long_rays = fam[(fam[:, 7] > 1e29) & (fam[:, 0] + fam[:, 1] > 1.0) & ((fam[:, 2] == -1.0) | (fam[:, 2] == 41.5))]    # beside the triangles, from either end: all the way
        short_rays = fam[(fam[:, 0] + fam[:, 1] < 1.0) | (fam[:, 7] < 1e29)]
        owners = (3, 11, 20, 29, 37, 44, 54, 62)
        lanes = {l: (short_rays[rng.integers(len(short_rays))], short_rays[rng.integers(len(short_rays))]) for l in range(64)}
        for l in owners:
            lanes[l] = (long_rays[rng.integers(len(long_rays))], long_rays[rng.integers(len(long_rays))])
        wave("eight owners of long rays among short ones", lanes)
        wave("every lane has two long rays", {l: (long_rays[rng.integers(len(long_rays))], long_rays[rng.integers(len(long_rays))]) for l in range(64)})
        nf = next(b.rays for b in rc.batches() if b.scene == "tower" and b.family == "nonfinite")
        lanes = {l: (fam[rng.integers(len(fam))], fam[rng.integers(len(fam))]) for l in range(64)}
        for l, k in ((5, 0), (17, 7), (40, 13), (63, 19)):
            lanes[l] = (nf[k], nf[(k + 9) % len(nf)])
        if scene_name == "tower":
            wave("four non-finite ray pairs among finite ones", lanes)
    # mixed: 64 distinct ray pairs of all finite families, seeded need bits (0 among them), 32 waves
    ps, pn = pool[rng.choice(len(pool), 64, replace=False)], pool[rng.choice(len(pool), 64, replace=False)]
    s, n, need = [], [], []
    for w in range(32):
        perm = rng.permutation(64)
        s.append(ps[perm]); n.append(pn[perm]); need.append(rng.integers(0, 4, 64))
    need = np.concatenate(need).astype(np.int32)
    assert all((need == k).sum() > 300 for k in range(4))
    out.append(("mixed, 32 waves", np.concatenate(s), np.concatenate(n), need))
    return out


@pytest.mark.parametrize("backward", [False, True], ids=["forward-layout", "backward-layout"])
@pytest.mark.parametrize("scene_name", ["tower", "tower64", "cbox", "terrain"])
def test_the_fused_walk_answers_as_the_plain_walk(scene_name, backward):
    """tower: pending sets of up to 18 entries against 12 / 10 in LDS — the scratch half of the stack, the one-at-a-time push and the
    patched pop; tower64: the control that stays in LDS; cbox, terrain: the other families in mixed waves."""
    c = rc.case(scene_name)
    scene = scene_of(scene_name, "bvh")
    if scene_name == "tower":
        assert scene.info()["bvh_stack_entries"] > 12                        # the builder's bound leaves room beyond the LDS part (12 / 10 entries)
    comps = waves_of(scene_name)
    shadow, nxt, need = (np.concatenate([x[k] for x in comps]) for k in (1, 2, 3))
    occ, ip, bt, differ = fused_against_plain(scene, c, shadow, nxt, need, backward, f"{scene_name} ({'backward' if backward else 'forward'} layout)")
    at = 0
    for name, s, n, nd in comps:                         # what the compositions are about, stated on the answers
        o, i = occ[at:at + len(nd)], c.tri_of(ip[at:at + len(nd)])
        cap = len(c.tri) - 2                             # the cap's triangle over (0.9, 0.9)
        if name.startswith("one owner"):
            l = int(name.split()[-1])
            assert i[l] == cap, (name, i[l], bt[at + l])
        if name == "shadow ray only, blocked by the cap": assert o[0] == 1
        if name == "shadow ray only, ending short of the cap": assert o[0] == 0
        if name == "both rays in one lane: miss, then cap": assert o[5] == 0 and i[5] == cap
        if name == "both rays in one lane: cap, then miss": assert o[5] == 1 and i[5] == -1
        if name.startswith("four non-finite"):
            for l in (5, 17, 40, 63):
                assert o[l] == 0 and i[l] == -1, (name, l)
        at += len(nd)
    print(f"[fused] {scene_name}, {'backward' if backward else 'forward'} layout: {len(need)} lanes in {len(need) // 64} waves, "
          f"{differ} continuation rays on another primitive at a bit-equal t, every lane equal to the plain walk and admissible")


@pytest.mark.parametrize("backward", [False, True], ids=["forward-layout", "backward-layout"])
def test_partial_waves_of_the_fused_walk(backward):
    """n = 1 and n = 65: the lanes beyond n take part without a ray (as thieves); n = 0 does nothing."""
    c = rc.case("tower")
    scene = scene_of("tower", "bvh")
    up, down = rc.tower_long_ray(c), rc.tower_long_ray(c, True)
    occ, ip, bt, _ = fused_against_plain(scene, c, down[None], up[None], np.array([3]), backward, "n = 1")
    assert occ[0] == 0 and c.tri_of(ip)[0] == len(c.tri) - 2
    fam = next(b.rays for b in rc.batches() if b.scene == "tower" and b.family == "tower")
    s, n = np.concatenate([fam[:64], up[None]]), np.concatenate([fam[64:128], down[None]])
    occ, ip, bt, _ = fused_against_plain(scene, c, s, n, np.full(65, 3), backward, "n = 65")
    assert occ[64] == 1 and ip[64, 0] == -1
    e = torch.empty((0, 8))
    occ, ip, bt = scene.trace_fused(e, e, torch.empty((0,), dtype=torch.int32), backward_layout=backward)
    scene.check()
    assert occ.shape == (0,) and ip.shape == (0, 2) and bt.shape == (0, 3)


# ----------------------------------------------------------------------------------------------- c. arguments
def test_fused_walk_arguments():
    L = _native.lib()
    bvh, brute = scene_of("cbox", "bvh"), scene_of("cbox", "brute")
    r = torch.zeros((64, 8), device=bvh.device); need = torch.zeros(64, dtype=torch.int32, device=bvh.device)
    occ = torch.zeros(64, dtype=torch.int32, device=bvh.device); ip = torch.zeros((64, 2), dtype=torch.int32, device=bvh.device); bt = torch.zeros((64, 3), device=bvh.device)
    good = [bvh._handle, r.data_ptr(), r.data_ptr(), need.data_ptr(), 64, 0, occ.data_ptr(), ip.data_ptr(), bt.data_ptr(), None]
    assert L.zdr_trace_fused(*good) == 0
    torch.cuda.synchronize()
    for k in (0, 1, 2, 3, 6, 7, 8):
        args = list(good); args[k] = None
        assert L.zdr_trace_fused(*args) == -1 and b"null" in L.zdr_last_error(), k          # ZDR_E_INVALID
    args = list(good); args[0] = brute._handle
    assert L.zdr_trace_fused(*args) == -3 and b"BVH" in L.zdr_last_error()                  # ZDR_E_UNSUPPORTED
    args[4] = 0
    assert L.zdr_trace_fused(*args) == -3
    args = list(good); args[4] = 0
    assert L.zdr_trace_fused(*args) == 0
    with pytest.raises(_native.ZdrError, match="BVH"):
        brute.trace_fused(r, r, need)
