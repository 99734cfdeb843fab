"""-m gpu: the item banks of the persistent path kernels (ItemBanks, zdr_kernels.hip) with several items per wave.

A wave keeps the items it draws in two banks, item n in bank n & 1, and starts the next item while the last paths of the one
before are still running.  The bookkeeping (which item a bank holds, how many of its paths are parked or running, when it
retires) can only go wrong when a wave draws several items and the banks are reused: the small images of the other tests give
every resident wave one item at the most.  Here the persistent grid is cut to one wave per CU with the knob the library reads
per call, ZDR_PERSISTENT_WAVES_PER_CU = 1 (256 waves on an MI355X):

  many-items        128 x 128, spp 64: 256 tiles x 8 chunks of 8 samples (spp / ZDR_MIN_CHUNK's default 8) = 2,048 items, eight per
                    wave, each bank reused four times.
  partial-tiles     100 x 76, spp 24, ZDR_MIN_CHUNK = 16: 13 x 10 tiles, the last column and the last row partly outside the image.
                    (24 / 16 allows ONE chunk per tile, so this grid has 130 items of 24 samples and no short chunk: the case is
                    kept as it was asked for, and the next one adds what it was meant to reach.)
  short-last-chunk  the same image with ZDR_MIN_CHUNK = 4 and ZDR_TARGET_WAVES = 650: 650 / 130 tiles = 5 chunks per tile of
                    ceil(24 / 5) = 5 samples, the last one of 4 (and every chunk shorter than a refill batch of 8): 650 items,
                    two or three per wave.

Each render is held to the CPU oracle with the bars of tests/gpu_util.py and to the same render with the default grid (one item
per wave at these sizes): the same paths, so only the order of the float additions may differ (the bars of
tests/test_gpu_render.py, test_work_item_granularity_only_reassociates).  scene.check() raises on ZDR_DEVERR_STALL and
ZDR_DEVERR_POOL.  The material is the cbox texture (roughness 1), which fits the base bars without a noise floor."""
import numpy as np
import pytest
import torch

from conftest import cbox_material_np
from gpu_util import assert_grad_parity, assert_image_parity, make_scene, oracle_params

pytestmark = pytest.mark.gpu

KNOBS = ("ZDR_PERSISTENT_WAVES_PER_CU", "ZDR_MIN_CHUNK", "ZDR_TARGET_WAVES")
CASES = {
    "many-items": ((128, 128), 64, {"ZDR_PERSISTENT_WAVES_PER_CU": "1"}),
    "partial-tiles": ((100, 76), 24, {"ZDR_PERSISTENT_WAVES_PER_CU": "1", "ZDR_MIN_CHUNK": "16"}),
    "short-last-chunk": ((100, 76), 24, {"ZDR_PERSISTENT_WAVES_PER_CU": "1", "ZDR_MIN_CHUNK": "4", "ZDR_TARGET_WAVES": "650"}),
}
SEED = 7


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def cotangent(W, H):
    return np.random.default_rng(11).uniform(0.5, 1.5, (H, W, 4)).astype(np.float32)


@pytest.fixture(scope="module")
def mat():
    return cbox_material_np()


_REFERENCE = {}


def reference(cbox_oracle, mat, res, spp):
    """(image, gradient) of the oracle, computed once per size: the accelerators and the grids render the same scene"""
    key = (res, spp)
    if key not in _REFERENCE:
        W, H = res
        scene = make_scene("path")
        img = cbox_oracle.render_forward(oracle_params(scene, W, H, spp, SEED, mat.shape[:2]), mat)
        grad = cbox_oracle.render_backward(oracle_params(scene, W, H, spp, SEED + 1, mat.shape[:2]), cotangent(W, H), mat)   # backward renders with seed + 1
        for a in (img, grad):
            a.setflags(write=False)
        _REFERENCE[key] = (img, grad)
    return _REFERENCE[key]


def render(scene, m, cot, res, spp):
    img = scene.render_forward(m, res, spp, SEED)
    scene.check()
    g = torch.zeros_like(m)
    scene.render_backward(cot, g, m, res, spp, SEED)
    scene.check()
    return img, g


def assert_reassociated_only(img, g, img0, g0):
    torch.testing.assert_close(img, img0, rtol=2e-5, atol=1e-6)
    torch.testing.assert_close(g, g0, rtol=1e-4, atol=1e-6 * float(g0.abs().max()))


@pytest.mark.parametrize("accel", ["brute", "bvh"])
@pytest.mark.parametrize("case", list(CASES))
def test_waves_that_draw_several_items_match_oracle_and_default_grid(case, accel, cbox_oracle, mat, monkeypatch):
    res, spp, env = CASES[case]
    W, H = res
    ref, gref = reference(cbox_oracle, mat, res, spp)
    scene = make_scene("path", accel=accel)
    assert scene.info()["accel"] == accel
    m = torch.from_numpy(mat).cuda()
    cot = torch.from_numpy(cotangent(W, H)).cuda()
    set_knobs(monkeypatch, env)
    img, g = render(scene, m, cot, res, spp)
    set_knobs(monkeypatch, {})
    img0, g0 = render(scene, m, cot, res, spp)
    what = f"item banks {case} {accel}"
    assert (img[..., 3] == 1.0).all()
    assert_image_parity(img.cpu().numpy()[..., :3], ref[..., :3], what + " forward")
    assert_grad_parity(g.cpu().numpy(), gref, what + " backward")
    assert_reassociated_only(img, g, img0, g0)


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_material_table_backward_with_several_items_per_wave(accel, mat, monkeypatch):
    """The material-table form of the loop (k_path<..., MT>, k_path_bwd<..., MT>): four materials of odd sizes in permuted slots
    (tests/test_gpu_materials_oracle.py), the short-last-chunk grid, against the oracle's material table and the default grid."""
    from test_gpu_materials_oracle import FIVE, SIZES, check_all, cot_image, render_both, rough
    from test_oracle_materials import split_box
    res, spp, env = CASES["short-last-chunk"]
    W, H = res
    mats = [rough(mat, h, w, k) for k, (h, w) in enumerate(SIZES)]
    cot = cot_image(W, H, 4)
    set_knobs(monkeypatch, env)
    scene, img, g, ref, gref = render_both(split_box(FIVE), "path", accel, [2, 0, 3, 1, None, None], mats, res, spp, SEED, cot)   # (calls scene.check())
    check_all(f"item banks material table {accel}", img, g, ref, gref, mats)
    set_knobs(monkeypatch, {})
    mt = [torch.from_numpy(x).cuda() for x in mats]
    img0 = scene.render_forward_materials(mt, res, spp, SEED)
    g0 = [torch.zeros_like(x) for x in mt]
    scene.render_backward_materials(torch.from_numpy(cot).cuda(), g0, mt, res, spp, SEED)
    scene.check()
    torch.testing.assert_close(torch.from_numpy(img).cuda(), img0, rtol=2e-5, atol=1e-6)
    for a, b in zip(g, g0):
        torch.testing.assert_close(torch.from_numpy(a).cuda(), b, rtol=1e-4, atol=1e-6 * float(b.abs().max()))


@pytest.mark.parametrize("accel", ["brute", "bvh"])
def test_emission_gradient_backward_with_several_items_per_wave(accel, monkeypatch):
    """The emission-gradient form (k_path_bwd<..., LG>) on the three-light scene, the short-last-chunk grid: for one seed the image
    is linear in the emissions, so <g, I(e)> = <d_e, e> without Monte Carlo noise (the bar of tests/test_gpu_emission_grad.py), and
    the default grid returns the same d_e up to the order of its additions."""
    from test_gpu_emission_grad import Case, build, emissions_of, euler, rel
    res, spp, env = CASES["short-last-chunk"]
    s = build("lights3", "path", accel)
    case = Case(s, w=res[0], h=res[1], spp=spp, seed=SEED)
    e = emissions_of(s)
    set_knobs(monkeypatch, env)
    lhs, rhs, d_e = euler(case, e)
    s.check()
    set_knobs(monkeypatch, {})
    _, _, d_e0 = euler(case, e)
    s.check()
    print(f"[item banks] emission gradient {accel}: <g, I> = {lhs!r}, <d_e, e> = {rhs!r}, rel {rel(lhs, rhs):.3e}")
    assert abs(lhs) > 1e-3, lhs
    assert rel(lhs, rhs) <= 1e-4, (lhs, rhs)
    torch.testing.assert_close(d_e, d_e0, rtol=1e-4, atol=1e-6 * float(d_e0.abs().max()))
