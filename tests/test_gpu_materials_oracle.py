"""-m gpu: per-model materials (Scene.material_slots, zdr_render_*_materials) against the CPU oracle's material table
(zdro_render_*_materials, pinned by tests/test_oracle_materials.py): materials of different, odd, non-square sizes and contents,
permuted slots, quads of the brute-force walk cut between instances, 16 materials, the environment gradient beside 15, every
cell mode of the staging array, the full-size configuration and tile shards.  Forward image and each material's gradient.

Flips (tests/gpu_util.py) needs a per-path dump that the material kernels do not have, so the materials are rough: resampled from
the cbox texture (roughness 1), which fits the base bars without it (tests/test_gpu_fullsize.py), or, for the few-texel cases,
roughness 0.6 - 1 as tests/test_gpu_render.py, test_few_texels_gradient_matches_oracle."""
import time

import numpy as np
import pytest
import torch

import oracle
from conftest import cbox_material_np
from gpu_util import assert_grad_parity, assert_image_parity, make_scene, oracle_params
from test_oracle_materials import split_box, textured

pytestmark = pytest.mark.gpu

SIZES = [(37, 91), (128, 64), (5, 3), (1, 1)]
FIVE = [0, 4, 6, 10, 16, 30]                    # back wall + ceiling, floor, side walls, short box, tall box: four reached by direct light
CUT = [0, 3, 13, 24, 30]                        # boundaries between the two triangles of merged quads (2|3, 11|16 12|17 10|15, 20|25 ...)
SIXTEEN = [0, 1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 20, 22, 24, 26, 28, 30]
SLOTS16 = [(7 * i + 11) % 16 for i in range(16)]   # a permutation; instance 12 (triangles 22, 23: the tall box's back faces) has slot 15


@pytest.fixture(scope="module")
def cbox_a():
    return cbox_material_np()


def rough(a, h, w, k):
    """An (h, w) material resampled from the cbox texture (roughness 1) with offsets and a tint of its own."""
    ys = (np.arange(h) * 1024 // h + 97 * k) % 1024
    xs = (np.arange(w) * 1024 // w + 331 * k) % 1024
    m = a[ys][:, xs].copy()
    m[..., :3] *= np.float32(0.55 + 0.45 * ((0.37 * k) % 1.0))
    return np.ascontiguousarray(m)


_KEEP = []


def cot_image(W, H, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, (H, W, 4)).astype(np.float32)


def render_both(arrays, integrator, accel, slots, mats, res, spp, seed, cot, sampler=None):
    """(image, gradients) of the HIP kernels and of the oracle for one scene, slot table and material list."""
    W, H = res
    scene = make_scene(integrator, accel=accel, arrays=arrays)
    okw = {}
    if sampler is not None:
        scene.sampler = "pmj02bn"
        scene.set_pmj02bn_tables(*sampler)
        _KEEP.append(sampler)                   # the oracle borrows the tables' memory
        oracle.lib().zdro_set_pmj02bn_tables(sampler[0].ctypes.data_as(oracle.C.POINTER(oracle.C.c_uint32)), *sampler[0].shape[:2],
                                             sampler[1].ctypes.data_as(oracle.C.POINTER(oracle.C.c_uint16)), *sampler[1].shape[:2])
        okw["sampler"] = oracle.SAMPLER_PMJ02BN
    scene.material_slots = slots
    mt = [torch.from_numpy(m).cuda() for m in mats]
    img = scene.render_forward_materials(mt, res, spp, seed).cpu().numpy()
    g = [torch.zeros_like(m) for m in mt]
    scene.render_backward_materials(torch.from_numpy(cot).cuda(), g, mt, res, spp, seed)
    scene.check()
    S = oracle.OracleScene.from_arrays(arrays)
    S.set_material_slots(slots)
    ref = S.render_forward_materials(oracle_params(scene, W, H, spp, seed, (1, 1), **okw), mats)
    gref = S.render_backward_materials(oracle_params(scene, W, H, spp, seed + 1, (1, 1), **okw), cot, mats)
    return scene, img, [x.cpu().numpy() for x in g], ref, gref


def check_all(what, img, g, ref, gref, mats):
    assert (ref[..., :3].max(-1) > 0).mean() > 0.5
    assert_image_parity(img[..., :3], ref[..., :3], f"{what} forward")
    assert (img[..., 3] == 1.0).all()
    for k, (gk, rk) in enumerate(zip(g, gref)):
        h, w = mats[k].shape[:2]
        assert np.abs(rk).sum() > 0, (what, k, "material receives no gradient")
        assert_grad_parity(gk, rk, f"{what} material {k} ({h} x {w})")
        assert abs(gk.sum() - rk.sum()) <= 3e-4 * np.abs(rk).sum(), (what, k, gk.sum(), rk.sum())


CASES = [(i, a, "cmj") for i in ("path", "direct", "collocated") for a in ("brute", "bvh")] + [("path", "brute", "pmj02bn")]


@pytest.mark.parametrize("integrator,accel,sampler", CASES)
def test_materials_of_odd_sizes_in_permuted_slots_match_oracle(integrator, accel, sampler, cbox_a):
    """Four materials of different, odd, non-square sizes on four of five pieces of the box, in permuted slots; the fifth piece
    (the tall box) has none: path stops there, direct returns its (zero) emission, collocated is black."""
    mats = [rough(cbox_a, h, w, k) for k, (h, w) in enumerate(SIZES)]
    slots = [2, 0, 3, 1, None, None]
    tables = None
    if sampler == "pmj02bn":
        from zdr_amd import pmj02bn_tables as T
        tables = (T.pmj02_sets(n_sets=5, n_samples=256, seed=2), T.blue_noise_textures(n_tex=4, res=32, seed=2))
    W, spp, seed = 64, 16, 3
    _, img, g, ref, gref = render_both(split_box(FIVE), integrator, accel, slots, mats, (W, W), spp, seed, cot_image(W, W, 1), tables)
    check_all(f"{integrator} {accel} {sampler}", img, g, ref, gref, mats)


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_quads_cut_between_instances_match_oracle(integrator, cbox_a):
    """The brute-force walk tests merged pairs of triangles as one quad (zdr_api.cpp, find_quads) also across instances: here
    every piece boundary but one falls between the two triangles of a quad, each side with a material of its own.  The oracle
    loops over plain triangles."""
    mats = [rough(cbox_a, h, w, k + 4) for k, (h, w) in enumerate([(16, 9), (3, 7), (24, 40), (2, 2)])]
    slots = [1, 3, 0, 2, None]
    W, spp, seed = 64, 16, 8
    _, img, g, ref, gref = render_both(split_box(CUT), integrator, "brute", slots, mats, (W, W), spp, seed, cot_image(W, W, 2))
    check_all(f"cut quads {integrator}", img, g, ref, gref, mats)


def sixteen(cbox_a):
    sizes = [(37, 91), (128, 64), (5, 3), (1, 1), (3, 5), (2, 2), (64, 32), (9, 17), (7, 1), (1, 6), (33, 20), (4, 4), (11, 13), (2, 9), (16, 3), (3, 5)]
    return [rough(cbox_a, h, w, k) for k, (h, w) in enumerate(sizes)]


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_sixteen_materials_match_oracle(accel, cbox_a):
    """16 pieces, 16 materials in permuted slots.  Slot 15 shades the tall box's two back faces, which the camera does not see:
    its gradient comes from vertices at depth >= 1 only, through the material byte of the backward record's link word."""
    mats = sixteen(cbox_a)
    W, spp, seed = 64, 32, 12
    _, img, g, ref, gref = render_both(split_box(SIXTEEN), "path", accel, SLOTS16 + [None], mats, (W, W), spp, seed, cot_image(W, W, 3))
    check_all(f"16 materials {accel}", img, g, ref, gref, mats)


def test_fifteen_materials_beside_the_environment_gradient(cbox_a):
    """15 materials and d_env in one call (zdr_render_backward_materials_env): the map is entry 15 of the table, material 14
    the last one beside it.  Image under the map and material gradients against the oracle; d_env still the exact adjoint."""
    from test_gpu_envmap_grad import Case, adjoint_identity, direction, rel, sky
    from zdr_amd import envmap
    mats = sixteen(cbox_a)[:15]
    slots = [None if k == 15 else k for k in SLOTS16] + [None]
    arrays = split_box(SIXTEEN)
    scene = make_scene("path", arrays=arrays)
    scene.add_envmap(sky())
    scene.material_slots = slots
    I = envmap.prepare_image(sky())
    S = oracle.OracleScene.from_arrays(arrays)
    S.set_envmap(I, *envmap.build_tables(I))
    S.set_material_slots(slots)
    W, spp, seed = 64, 16, 4
    mt = [torch.from_numpy(m).cuda() for m in mats]
    cot = cot_image(W, W, 4)
    img = scene.render_forward_materials(mt, (W, W), spp, seed).cpu().numpy()
    g = [torch.zeros_like(m) for m in mt]
    d_env = torch.zeros(I.shape, device="cuda")
    scene.render_backward_materials(torch.from_numpy(cot).cuda(), g, mt, (W, W), spp, seed, d_env=d_env)
    scene.check()
    ref = S.render_forward_materials(oracle_params(scene, W, W, spp, seed, (1, 1)), mats)
    gref = S.render_backward_materials(oracle_params(scene, W, W, spp, seed + 1, (1, 1)), cot, mats)
    check_all("15 materials + d_env", img, [x.cpu().numpy() for x in g], ref, gref, mats)
    assert float(d_env.abs().sum()) > 0
    E = torch.from_numpy(np.ascontiguousarray(I, np.float32)).cuda()
    lhs, rhs, _ = adjoint_identity(Case(scene, mt, slots), E, direction(E))
    scene.check()
    assert abs(lhs) > 1e-3 and rel(lhs, rhs) <= 1e-4, (lhs, rhs)


CELL_MODES = {
    "lds": [(1, 1), (2, 2), (1, 3)],             # 4 + 9 + 8 = 21 cells: the whole array in LDS (<= 28)
    "copies": [(37, 91), (5, 3), (1, 1)],        # 3,524 cells: replicated staging arrays (< 2^16)
    "one_copy": [(256, 256), (1, 1), (2, 2)],    # 66,049 + 4 + 9 cells: one copy of the concatenated array (>= 2^16)
}


@pytest.mark.parametrize("mode", list(CELL_MODES))
@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_every_cell_mode_matches_oracle_texel_by_texel(integrator, mode, cbox_a):
    """Three materials in each mode of the staging array (scene.h): small materials texel by texel at the bar of
    test_few_texels_gradient_matches_oracle, larger ones through assert_grad_parity, every sum to 3e-4."""
    dims = CELL_MODES[mode]
    mats = [textured(h, w, 20 + k) if h * w <= 64 else rough(cbox_a, h, w, k) for k, (h, w) in enumerate(dims)]
    W, spp, seed = 96, 16, 4
    _, img, g, ref, gref = render_both(split_box([0, 10, 20, 30]), integrator, "brute", [0, 1, 2, None], mats, (W, W), spp, seed,
                                       cot_image(W, W, 5))
    assert_image_parity(img[..., :3], ref[..., :3], f"cells {mode} {integrator} forward")
    for k, (got, r) in enumerate(zip(g, gref)):
        h, w = dims[k]
        assert np.abs(r).sum() > 0
        if h * w <= 64:
            bad = np.abs(got - r) > 2e-3 * np.abs(r) + 2e-4 * np.abs(r).max()
            print(f"[cells] {mode} {integrator} material {k} ({h} x {w}): max rel {float((np.abs(got - r) / np.abs(r).max()).max()):.2e}")
            assert bad.sum() == 0, (mode, k, int(bad.sum()), np.abs(got - r).max())
        else:
            assert_grad_parity(got, r, f"cells {mode} {integrator} material {k} ({h} x {w})")
        assert abs(got.sum() - r.sum()) <= 3e-4 * abs(r.sum()), (mode, k, got.sum(), r.sum())


def test_full_size_constant_material_beside_the_cbox_texture(cbox_a):
    """BASELINE configs[2]'s size (path, 512^2, spp 256) on the box in two pieces: the walls with the 1024^2 cbox material, the two
    boxes with a 1 x 1 constant.  Every gradient term of the constant lands on its 4 staging cells: the reference's few-texel
    hotspot (README.md:21 of the reference; DESIGN.md: one float32 accumulator of 1e8 terms was 40 % off)."""
    const = np.array([0.6, 0.35, 0.25, 1.0], np.float32).reshape(1, 1, 4)
    mats = [cbox_a, const]
    arrays = split_box([0, 15, 30])
    scene = make_scene("path", arrays=arrays)
    scene.material_slots = [0, 1, None]
    W, spp, seed = 512, 256, 7
    cot = cot_image(W, W, 1)
    mt = [torch.from_numpy(m).cuda() for m in mats]
    img = scene.render_forward_materials(mt, (W, W), spp, seed).cpu().numpy()
    ct = torch.from_numpy(cot).cuda()
    g = [torch.zeros_like(m) for m in mt]
    scene.render_backward_materials(ct, g, mt, (W, W), spp, seed)   # warm-up: buffers, code objects
    torch.cuda.synchronize()
    g = [torch.zeros_like(m) for m in mt]
    t0 = time.perf_counter()
    scene.render_backward_materials(ct, g, mt, (W, W), spp, seed)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    scene.check()
    S = oracle.OracleScene.from_arrays(arrays)
    S.set_material_slots([0, 1, None])
    ref = S.render_forward_materials(oracle_params(scene, W, W, spp, seed, (1, 1)), mats)
    gref = S.render_backward_materials(oracle_params(scene, W, W, spp, seed + 1, (1, 1)), cot, mats)
    g0, g1 = [x.cpu().numpy() for x in g]
    err = np.abs(g1 - gref[1]) / np.abs(gref[1])
    print(f"[full size] backward {ms:.1f} ms; 1 x 1 material: got {g1.ravel()} oracle {gref[1].ravel()} max rel err {err.max():.2e}")
    assert_image_parity(img[..., :3], ref[..., :3], "full size two materials forward")
    assert_grad_parity(g0, gref[0], "full size two materials: cbox texture")
    assert (np.abs(gref[1]) > 0).all() and err.max() <= 3e-4, (g1.ravel(), gref[1].ravel())


def test_tile_shards_union_to_the_oracle_image(cbox_a):
    """The union of render_forward_materials(..., tile_shard=(r, 8)) over r is the oracle's unsharded image."""
    mats = [rough(cbox_a, h, w, k) for k, (h, w) in enumerate(SIZES)]
    slots = [2, 0, 3, 1, None, None]
    arrays = split_box(FIVE)
    scene = make_scene("path", arrays=arrays)
    scene.material_slots = slots
    mt = [torch.from_numpy(m).cuda() for m in mats]
    W, H, spp, seed = 77, 52, 16, 6
    parts = torch.full((H, W, 4), -1.0, device="cuda")
    owner = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    for r in range(8):
        one = scene.render_forward_materials(mt, (W, H), spp, seed, tile_shard=(r, 8), out=torch.full((H, W, 4), -1.0, device="cuda"))
        mine = one[..., 3] >= 0
        owner += mine.int()
        parts = torch.where(mine[..., None], one, parts)
    scene.check()
    assert (owner == 1).all()
    S = oracle.OracleScene.from_arrays(arrays)
    S.set_material_slots(slots)
    ref = S.render_forward_materials(oracle_params(scene, W, H, spp, seed, (1, 1)), mats)
    assert_image_parity(parts.cpu().numpy()[..., :3], ref[..., :3], "8 tile shards, union")
    assert (parts[..., 3] == 1.0).all()
