"""-m gpu: the bounced light (Scene.texel_bounce; include/zdr.h, zdr_scene_texel_bounce) against the float64 reference of
tests/texel_bounce_ref.py on the cases of tests/texel_bounce_cases.py, for both accelerators.

1. Estimator: the reference shades the dump's OWN hits, so the comparison is of the shading alone; every vertex's beta and add within
   max(4 x MARGINS, 4 float32 ulps of the case's largest add) where the flags agree and no decision is near; at most 1 % of the samples
   set aside for differing flags.
2. Walk: against the free-running reference, nvert and the triangle at every vertex agree for at least 99 % of the samples (the host test
   bounds the reference's own fragility at 0.25 %); the largest |u, v| differences per vertex index are printed, and
   tools/texel_bounce_margins.py writes the same lines into profiles/texel_bounce_margins.txt.
3. The buffer of texel_bounce_forward is, bit for bit, the sum of the dumped adds in the order the header defines, times 1 / spp.
4. Properties: the same bits from run to run and from workspace to workspace, a zero material, sample ranges, the prefix property, the
   statement about the Cornell box's ceiling, BVH against brute force.
5. and 6.: the high-level call on a list, and the argument checks.
Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

import texel_bounce_cases as BC
import texel_bounce_ref as BR
import texel_lighting_cases as LC
from texel_bounce_gpu import ACCELS, case_args, case_kw, case_scene, run_dump, run_forward, walk_differences
from zdr_amd import TexelBounce
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

def sum_of_dump(name, q, dump, samples=None, vertices=None):
    """The texel buffer from the dumped adds, in float32 and in the order of include/zdr.h: lane j of 2^shift takes the samples begin + j,
    begin + j + lanes, ... and adds the accepted adds of each, vertices ascending; the lanes' sums are added in lane order, times 1 / spp."""
    H, W = BC.case(name)[2]
    spp = BC.case(name)[4]
    begin, end = samples if samples is not None else (BC.RANGES.get(name) or (0, spp))
    shift = N.lib().zdr_texel_bounce_lanes_shift(H, W, begin, end)
    assert shift >= 0
    lanes, ns = 1 << shift, end - begin
    T = q.shape[0] // ns
    assert T * ns == q.shape[0] and (q[:, 2].reshape(T, ns) == np.arange(begin, end)).all()
    K = dump["add"].shape[1] if vertices is None else vertices
    add = dump["add"].astype(np.float32).reshape(T, ns, -1, 3)
    added = ((dump["flags"] & BR.F_ADDED) != 0).reshape(T, ns, -1)
    E = np.zeros((T, lanes, 3), np.float32)
    for si in range(ns):
        for k in range(K):
            m = added[:, si, k]
            E[m, si % lanes] = E[m, si % lanes] + add[m, si, k]
    Es = E[:, 0].copy()
    for j in range(1, lanes):
        Es = Es + E[:, j]
    out = np.zeros((H, W, 4), np.float32)
    xs, ys = q[::ns, 0], q[::ns, 1]
    out[ys, xs, :3] = Es * (np.float32(1.0) / np.float32(spp))
    out[ys, xs, 3] = dump["surface"].reshape(T, ns).sum(1).astype(np.float32) / np.float32(spp)
    return out, lanes


# ---------------------------------------------------------------------------------------- 1. estimator
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_shading_of_the_dumps_own_hits(name, accel):
    q, dump = run_dump(name, accel)
    K = BC.bounces(name)
    ref = BC.run_reference(name, hits=dump)
    same = (ref["flags"] == dump["flags"]).all(1) & (ref["nvert"] == dump["nvert"])
    have = (np.arange(K)[None, :] < dump["nvert"][:, None]) & same[:, None] & ~ref["near"]
    eb = np.abs(dump["beta"].astype(np.float64) - ref["beta"]).max(-1)
    ea = np.abs(dump["add"].astype(np.float64) - ref["add"]).max(-1)
    bar = BC.bar(name)
    print(f"[texel bounce estimator] {name} {accel}: samples {same.size}, flags differ on {int((~same).sum())}, vertices compared {int(have.sum())} "
          f"(near: {int((ref['near'] & (np.arange(K)[None, :] < dump['nvert'][:, None])).sum())}); kernel vs float64: beta {eb[have].max():.3e}, add {ea[have].max():.3e}; "
          f"float32 reference {BC.MARGINS[name]:.3e}; bar {bar:.3e}; largest add {BC.scale(name):.4e}; accepted {int(((dump['flags'] & BR.F_ADDED) != 0).sum())}")
    assert have.sum() > 0 and ((dump["flags"] & BR.F_ADDED) != 0).any()
    assert (~same).sum() <= BC.MAX_SET_ASIDE * same.size
    assert eb[have].max() <= bar and ea[have].max() <= bar


# --------------------------------------------------------------------------------------------- 2. walk
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_walk_against_the_free_running_reference(name, accel):
    q, dump = run_dump(name, accel)
    ref = BC.reference(name)
    agree, line = walk_differences(name, accel)
    print(line)
    assert agree.sum() >= BC.MIN_WALK_AGREEMENT * agree.size
    assert np.array_equal(dump["surface"][agree], ref["surface"][agree])


# ------------------------------------------------------------------------ 3. product is the sum of dump
@pytest.mark.parametrize("accel", ACCELS)
@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_buffer_is_the_sum_of_the_dump_bit_for_bit(name, accel):
    q, dump = run_dump(name, accel)
    want, lanes = sum_of_dump(name, q, dump)
    got = run_forward(name, accel)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())
    print(f"[texel bounce product] {name} {accel}: {lanes} lanes per texel, texels whose bits differ from the sum of the dump: {diff} of {got.shape[0] * got.shape[1]}; "
          f"largest irradiance {got[..., :3].max():.4e}")
    assert (got[~BC.reached(name)] == 0).all()
    assert got[..., :3].max() > 0
    assert diff == 0
    if name == "multi_k3":
        assert lanes == 8                                             # 9 samples: two trips, and lanes 1..7 have none in the second


# -------------------------------------------------------------------------------------- 4. properties
@pytest.mark.parametrize("accel", ACCELS)
def test_two_runs_and_two_workspaces_give_the_same_bits(accel):
    name = "multi_k3"
    scene = case_scene(name, accel)
    pts, m = case_args(name)
    need = N.lib().zdr_texel_bounce_workspace_bytes(24, 24)
    a = scene.texel_bounce_forward(pts, m, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"), **case_kw(name)).clone()
    b = scene.texel_bounce_forward(pts, m, workspace=torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda"), **case_kw(name)).clone()
    c = scene.texel_bounce_forward(pts, m, **case_kw(name))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    scene.check()


@pytest.mark.parametrize("accel", ACCELS)
def test_a_zero_material_gives_exact_zeros_and_the_same_surface(accel):
    name = "multi_k3"
    got = run_forward(name, accel)
    zero = run_forward(name, accel, mats=tuple(np.zeros_like(m) for m in BC.materials(name)))
    assert (zero[..., :3] == 0).all() and (got[..., :3] > 0).any()
    assert np.array_equal(zero[..., 3], got[..., 3]) and (got[..., 3] > 0).any()


@pytest.mark.parametrize("accel", ACCELS)
def test_disjoint_sample_ranges_add_up_to_the_whole(accel):
    name = "cbox_k3"
    whole = run_forward(name, accel).astype(np.float64)
    parts = run_forward(name, accel, samples=(0, 2)).astype(np.float64) + run_forward(name, accel, samples=(2, 4)).astype(np.float64)
    ulp = float(np.spacing(np.float32(whole[..., :3].max())))
    off = np.abs(whole - parts)[..., :3].max() / ulp
    print(f"[texel bounce ranges] {accel}: [0, 2) + [2, 4) against [0, 4): largest difference {off:.2f} ulps of the largest irradiance {whole[..., :3].max():.4e}")
    assert off <= 4.0
    assert np.array_equal(whole[..., 3], parts[..., 3])               # counts over spp: quarters are exact


@pytest.mark.parametrize("accel", ACCELS)
def test_one_bounce_is_the_first_vertex_of_a_walk_of_three(accel):
    q, dump = run_dump("cbox_k3", accel)
    want, _ = sum_of_dump("cbox_k3", q, dump, vertices=1)
    got = run_forward("cbox_k1", accel)
    assert got[..., :3].max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("accel", ACCELS)
def test_the_ceiling_of_the_cornell_box_has_no_direct_light_and_mostly_bounced_light(accel):
    name = "cbox_k3"
    pts, _ = case_args(name)
    direct = case_scene(name, accel).texel_lighting_forward(pts, spp=BC.CASES[name][4], seed=BC.SEED).cpu().numpy()
    n, dark, lit = BC.ceiling_statement(direct, run_forward(name, accel), BC.points(name))
    rn, rdark, rlit = BC.ceiling_statement(LC.reference("cbox_16x16")["data"], BC.reference(name)["data"], BC.points(name))
    print(f"[texel bounce ceiling] {accel}: ceiling texels {n}, direct irradiance exactly 0 on {dark}, bounced light on {lit} (reference: {rn}, {rdark}, {rlit})")
    assert n == rn > 0 and dark == n
    assert lit > n // 2 and abs(lit - rlit) <= max(1, rn // 20)


def test_bvh_and_brute_force_agree():
    name = "multi_k3"
    (q, a), (_, b) = run_dump(name, "brute"), run_dump(name, "bvh")
    same = BR.signature_equal(a, b)
    fa, fb = run_forward(name, "brute"), run_forward(name, "bvh")
    err = np.abs(fa[..., :3].astype(np.float64) - fb[..., :3]).max()
    print(f"[texel bounce accelerators] {name}: signatures agree on {int(same.sum())} of {same.size} samples; irradiance differs by at most {err:.3e} "
          f"over all texels (the estimator's bar: {BC.bar(name):.3e})")
    assert np.array_equal(fa[..., 3], fb[..., 3])
    assert err <= BC.bar(name)


# --------------------------------------------------------------------- 5. the high-level call on a list
def test_texel_bounce_of_a_list_bakes_the_second_materials_texture_at_its_own_size():
    name = "multi_k3"
    scene = case_scene(name, "bvh")
    _, m = case_args(name)
    old = scene.material_slots
    scene.material_slots = BC.MULTI_SLOTS
    try:
        tb = scene.texel_bounce(m, index=1, spp=4, bounces=2, seed=BC.SEED)
        assert isinstance(tb, TexelBounce) and tuple(tb.data.shape) == (5, 7, 4) and not tb.data.requires_grad
        texels = scene.texel_aovs(m, 1)
        low = scene.texel_bounce_forward(texels.data, m, spp=4, bounces=2, seed=BC.SEED)
        torch.cuda.synchronize()
        assert torch.equal(tb.data, low)
        assert (tb.irradiance > 0).any() and (tb.surface > 0).any() and (tb.surface <= 1).all()
        first = scene.texel_bounce(m, spp=4, bounces=2, seed=BC.SEED)
        assert tuple(first.data.shape) == (24, 24, 4)
        with pytest.raises(ValueError):
            scene.texel_bounce(m, index=2)
    finally:
        scene.material_slots = old


# --------------------------------------------------------------------------------- 6. argument checks
def test_bad_arguments_raise():
    name = "cbox_k1"
    scene = case_scene(name, "brute")
    pts, m = case_args(name)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            scene.texel_bounce_forward(pts, m, spp=4, bounces=bad)
    for samples in ((2, 2), (3, 1), (0, 5)):
        with pytest.raises(ValueError):
            scene.texel_bounce_forward(pts, m, spp=4, samples=samples)
    with pytest.raises(ValueError):
        scene.texel_bounce_forward(pts[..., :8].contiguous(), m, spp=4)
    with pytest.raises(ValueError):
        scene.texel_bounce_forward(pts.reshape(-1, 16), m, spp=4)
    with pytest.raises(ValueError):
        scene.texel_bounce_dump(pts, m, torch.zeros((1, 3), dtype=torch.int32), spp=4, bounces=9)
    p = N.TexelBounceParams()
    p.struct_size = 4
    out = torch.zeros((16, 16, 4), device="cuda")
    ws = torch.zeros(2048, dtype=torch.uint8, device="cuda")
    dims = np.array([[16, 16]], np.int32)
    assert N.lib().zdr_scene_texel_bounce(scene._handle, C.byref(p), pts.data_ptr(), m[0].data_ptr(), dims.ctypes.data, 1, out.data_ptr(), ws.data_ptr(), None) == -1   # ZDR_E_INVALID
