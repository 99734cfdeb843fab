"""-m gpu: the texture-space feature buffers (Scene.texel_aovs; include/zdr.h, zdr_scene_texel_aovs) against the float64 reference of
tests/texel_ref.py on the cases of tests/texel_cases.py, and the properties the header states: watertight coverage on shared edges,
degenerate triangles, the slot table, determinism, agreement with what the renderer reads and writes, the denoiser on these guides, and
the argument checks of the C entry points.

Discrete channels are exact outside a case's uncertain texels (tests/texel_cases.py); position, normal and texel_size are held to
4 x the float32 reference's own error with a floor of 4 float32 ulps of the channel's scale (texel_cases.bars).  Every figure is printed
before it is asserted."""
import os

import numpy as np
import pytest
import torch

import texel_cases as TC
import texel_ref as R
from conftest import ASSETS
from denoise_ref import denoise_ref
from gpu_util import make_scene, panel_mesh, terrain_arrays
from test_gpu_denoise import within_bound
from zdr_amd import Scene, TexelAovs, denoise, geometry
from zdr_amd import _native as N

pytestmark = pytest.mark.gpu

_scenes = {}


def case_scene(name, accel="auto"):
    make = TC.CASES[name][0]
    key = (make, accel)
    if key not in _scenes:
        _scenes[key] = Scene(make(), integrator="direct", accel=accel)
    return _scenes[key]


def run_case(name, accel="auto"):
    _, slots, material, hw = TC.CASES[name]
    out = case_scene(name, accel).texel_aovs_forward(material, hw, slots=slots)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name", list(TC.CASES))
def test_parity_with_the_float64_reference(name):
    got = run_case(name).cpu().numpy()
    ref = TC.reference(name)
    keep = TC.compared(name)
    d = ref["data"]
    print(f"[texel parity] {name}: {int((~keep).sum())} of {keep.size} texels uncertain; covered {int(d[..., 11].sum())}, reached {int(d[..., 12].sum())}; "
          f"coverage differs on {int((got[..., 11] != d[..., 11])[keep].sum())}, reach on {int((got[..., 12] != d[..., 12])[keep].sum())}, "
          f"instance on {int((got[..., 14] != d[..., 14])[keep].sum())}")
    for ch in (11, 12, 14, 15):
        assert np.array_equal(got[..., ch][keep], d[..., ch][keep]), (name, ch)
    assert (got[..., 0:4] == 0).all() and (got[..., 13] == 0).all()
    empty = got[..., 12] == 0
    assert (got[empty][:, :14] == 0).all() and (got[empty][:, 14:] == -1).all()
    e, bars, m = TC.errors(name, got), TC.bars(name), TC.MARGINS[name]
    print(f"[texel parity] {name}: kernel vs float64 position {e[0]:.3e} normal {e[1]:.3e} texel_size {e[2]:.3e};  float32 reference {m[0]:.3e} {m[1]:.3e} {m[2]:.3e};  "
          f"bars {bars[0]:.3e} {bars[1]:.3e} {bars[2]:.3e}")
    for got_e, bar in zip(e, bars):
        assert got_e <= bar, (name, e, bars)


def test_where_several_triangles_cover_a_texel_the_lowest_g_wins():
    """the soup: the winner's position and normal are those of the reference's winner, which the parity test holds; here the winner is
    identified by the texel_size channel, which differs from triangle to triangle"""
    got = run_case("soup_130").cpu().numpy()
    ref = TC.reference("soup_130")
    A = TC.soup_arrays()
    H, W = TC.SOUP_HW
    _, _, UV, area, _ = R.world_triangles(A, np.float64)
    Q = R.pixel_space(UV, H, W, np.float64)
    size = np.array([np.sqrt(area[g] / (0.5 * abs(R.Setup(Q[g], np.float64).area2))) for g in range(130)])
    keep = TC.compared("soup_130") & (ref["cov_g"] >= 0)
    want = size[ref["cov_g"][keep]]
    assert np.abs(got[..., 7][keep] - want).max() <= 1e-5 * want.max()
    won = np.unique(ref["cov_g"][keep])
    assert (won < 2).sum() == 2 and (won >= 102).any() and (ref["cov_g"][keep] >= 2).sum() > 20      # the large ones, and others beside them


# ------------------------------------------------------------------------------------ watertightness
def atlas_scene(kind, n):
    key = ("atlas", kind, n)
    if key not in _scenes:
        arrays = terrain_arrays(n) if kind == "terrain" else geometry.from_arrays(*panel_mesh(n, n))
        _scenes[key] = Scene(arrays, integrator="direct")
    return _scenes[key]


@pytest.mark.parametrize("kind", ["terrain", "panel"])
@pytest.mark.parametrize("n,hw", [(8, (8, 8)), (8, (9, 9)), (8, (5, 7)), (16, (33, 33)), (64, (16, 16))])
def test_a_unit_square_atlas_is_covered_without_a_gap(kind, n, hw):
    """exact, no tolerance: every lattice point of the texture lies in the closed unit square, many of them on shared edges or on
    vertices (9 x 9 over an 8 x 8 grid: all of them), and at least one triangle must claim each"""
    scene = atlas_scene(kind, n)
    slots = (0, None) if kind == "terrain" else (0,)
    got = scene.texel_aovs_forward(0, hw, slots=slots).cpu().numpy()
    print(f"[texel watertight] {kind} n={n} {hw}: uncovered {int((got[..., 11] != 1).sum())}, unreached {int((got[..., 12] != 1).sum())}")
    assert (got[..., 11] == 1).all() and (got[..., 12] == 1).all() and (got[..., 14] == 0).all() and (got[..., 15] == 0).all()
    assert np.isfinite(got).all()


# ---------------------------------------------------------------------------------- degenerate input
def test_triangles_without_area_reach_by_their_box_and_cover_nothing():
    scene = Scene([(os.path.join(ASSETS, "quad.obj"), None, 0.0)], integrator="direct")
    for H, W in ((6, 5), (8, 8)):
        got = scene.texel_aovs_forward(0, (H, W), slots=(0,)).cpu().numpy()
        ys, xs = np.mgrid[0:H, 0:W]
        assert (got[..., 11] == 0).all()
        assert np.array_equal(got[..., 12] == 1, (xs <= 1) & (ys >= H - 2))
        assert (got[..., 7] == 0).all() and np.isfinite(got).all()
        assert (got[..., 14][got[..., 12] == 1] == 0).all()
    got = scene.texel_aovs_forward(0, (1, 1), slots=(0,)).cpu().numpy()
    assert got[0, 0, 11] == 0 and got[0, 0, 12] == 1
    scene.check()


def test_a_triangle_with_a_nan_uv_is_skipped():
    v, t = panel_mesh(1, 1)
    v = np.concatenate([v, v[[0, 2, 1]]])
    v[:4, 3:5] = np.array([0.23, 0.19], np.float32) + np.array([0.51, 0.47], np.float32) * v[:4, 3:5]   # (no lattice point of 16 x 16 on an edge)
    v[4:, 3:5] = np.array([[0.8, 0.8], [0.95, 0.8], [0.8, 0.95]], np.float32)   # a third triangle away from the first two ...
    v[5, 3] = np.nan                                                 # ... with a NaN u at one corner
    t = np.concatenate([t, [[4, 5, 6]]]).astype(np.int32)
    A = geometry.from_arrays(v, t)
    scene = Scene(A, integrator="direct")
    got = scene.texel_aovs_forward(0, (16, 16), slots=(0,)).cpu().numpy()
    good = geometry.from_arrays(v[:4], t[:2])
    r = R.texel_aovs_ref(good, (0,), 0, (16, 16))
    ref = r["data"]
    assert not r["uncertain"].any()
    assert np.array_equal(got[..., 11], ref[..., 11]) and np.array_equal(got[..., 12], ref[..., 12])
    assert got[..., 12].sum() > 0 and np.isfinite(got).all()
    scene.check()                                                    # the device error word stays clear


# --------------------------------------------------------------------------------------------- slots
def two_panels():
    if "two_panels" not in _scenes:
        v, t = panel_mesh(2, 2)
        v = v.copy(); v[:, 3:5] = 0.1 + 0.8 * v[:, 3:5]
        lift = np.eye(4, dtype=np.float32); lift[1, 3] = 1.0
        A = geometry.from_arrays(np.concatenate([v, v]), np.concatenate([t, t + v.shape[0]]), [0, t.shape[0], 2 * t.shape[0]],
                                 np.stack([np.eye(4, dtype=np.float32).reshape(16), lift.reshape(16)]))
        _scenes["two_panels"] = Scene(A, integrator="direct")
    return _scenes["two_panels"]


def test_the_slot_table_decides_whose_triangles_are_rasterised():
    scene = two_panels()
    hw = (12, 12)
    both = scene.texel_aovs_forward(0, hw, slots=(0, 0)).cpu().numpy()
    cov = both[..., 11] == 1
    assert cov.sum() > 50 and (both[..., 14][cov] == 0).all() and (both[..., 9][cov] == 0).all()        # the lower g: model 0, at y = 0
    second = scene.texel_aovs_forward(0, hw, slots=(None, 0)).cpu().numpy()
    assert np.array_equal(second[..., 11], both[..., 11]) and (second[..., 14][cov] == 1).all() and np.abs(second[..., 9][cov] - 1).max() < 1e-6
    for k in (0, 1):
        own = scene.texel_aovs_forward(k, hw, slots=(0, 1)).cpu().numpy()
        assert np.array_equal(own[..., 11], both[..., 11]) and (own[..., 14][cov] == k).all() and (own[..., 15][cov] == k).all()
    none = scene.texel_aovs_forward(5, hw, slots=(0, 1)).cpu().numpy()
    assert (none[..., :14] == 0).all() and (none[..., 14:] == -1).all()


def test_the_emitter_of_the_cornell_box_never_appears_and_the_views_are_views():
    scene = make_scene("path")
    mat = torch.rand(16, 24, 4, device="cuda")
    f = scene.texel_aovs(mat)
    assert isinstance(f, TexelAovs) and tuple(f.data.shape) == (16, 24, 16) and not f.data.requires_grad
    inst = f.instance.cpu().numpy()
    assert set(np.unique(inst)) <= {-1.0, 0.0} and (inst == 0).sum() > 0
    assert torch.equal(f.coverage, f.data[..., 11]) and torch.equal(f.reach, f.data[..., 12]) and torch.equal(f.position, f.data[..., 8:11])
    assert torch.equal(f.normal, f.data[..., 4:7]) and torch.equal(f.texel_size, f.data[..., 7]) and torch.equal(f.slot, f.data[..., 15])
    g = f.as_guides()
    assert torch.equal(g[..., 11], f.reach) and torch.equal(g[..., :11], f.data[..., :11]) and torch.equal(g[..., 12:], f.data[..., 12:])
    assert torch.equal(f.as_guides(reached=False), f.data) and g.data_ptr() != f.data.data_ptr()
    assert float((f.reach - f.coverage).min()) >= 0 and float((f.reach - f.coverage).sum()) > 0
    assert torch.equal(scene.texel_aovs([mat]).data, f.data)                              # a list of one: the default slots give the same table
    with pytest.raises(ValueError):
        scene.texel_aovs(mat, index=1)


# --------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["cbox_64x64", "soup_130"])
def test_two_calls_and_both_accelerators_give_the_same_bits(name):
    a, b = run_case(name, "brute"), run_case(name, "brute")
    c = run_case(name, "bvh")
    assert case_scene(name, "brute").info()["accel"] == "brute" and case_scene(name, "bvh").info()["accel"] == "bvh"
    assert torch.equal(a, b) and torch.equal(a, c)
    assert float(a[..., 11].sum()) > 0


# ---------------------------------------------------------------------------------- against the renderer
@pytest.mark.parametrize("tex", [16, 64])
def test_gradients_of_the_screen_side_buffers_land_only_on_reached_texels(tex):
    scene = make_scene("path")
    gen = torch.Generator().manual_seed(11 + tex)
    mat = torch.rand(tex, tex, 4, generator=gen).cuda()
    cot = torch.zeros(64, 64, 16)
    cot[..., 0:4] = torch.rand(64, 64, 4, generator=gen) + 0.1
    d = torch.zeros_like(mat)
    scene.render_aovs_backward(cot.cuda(), d, mat, (64, 64), 4, 5)
    reach = scene.texel_aovs(mat).reach
    torch.cuda.synchronize()
    nz = (d != 0).any(-1)
    print(f"[texel support] {tex}^2: texels with gradient {int(nz.sum())}, reached {int((reach == 1).sum())}, gradient outside reach {int((nz & (reach != 1)).sum())}")
    assert int(nz.sum()) > 0.3 * int((reach == 1).sum())
    assert not bool((nz & (reach != 1)).any())


def test_texel_positions_looked_up_at_a_pixels_uv_give_the_pixels_position():
    """position is affine within a triangle: where a pixel's four footprint texels are covered and won by one triangle, the bilinear
    lookup of the texel positions at the pixel's uv IS the point the pixel sees"""
    name = "cbox_64x64"
    scene = make_scene("path")
    H = W = 64
    tex = run_case(name).cpu().numpy().astype(np.float64)
    ref = TC.reference(name)
    f = scene.render_aovs(torch.rand(H, W, 4, device="cuda"), res=(32, 32), spp=1, seed=3)
    a = f.data.detach().cpu().numpy()
    hit = (a[..., 14] == 0) & (a[..., 11] == 1)
    uv = a[..., 12:14][hit]
    px, py = uv[:, 0] * np.float32(W - 1), (np.float32(1.0) - uv[:, 1]) * np.float32(H - 1)
    ix, iy = px.astype(np.int32), py.astype(np.int32)
    ox, oy = (px - ix).astype(np.float64), (py - iy).astype(np.float64)
    x0, x1, y0, y1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    g = [ref["cov_g"][y, x] for y, x in ((y0, x0), (y1, x0), (y0, x1), (y1, x1))]
    ok = (g[0] >= 0) & (g[0] == g[1]) & (g[0] == g[2]) & (g[0] == g[3])
    for y, x in ((y0, x0), (y1, x0), (y0, x1), (y1, x1)):
        ok &= ~ref["uncertain"][y, x] & (tex[y, x, 11] == 1)
    P = lambda y, x: tex[y, x, 8:11]                                                       # noqa: E731
    looked = (P(y0, x0) * (1 - oy)[:, None] + P(y1, x0) * oy[:, None]) * (1 - ox)[:, None] + (P(y0, x1) * (1 - oy)[:, None] + P(y1, x1) * oy[:, None]) * ox[:, None]
    err = np.abs(looked - a[..., 8:11][hit].astype(np.float64))[ok]
    bar = TC.bars(name)[0]
    print(f"[texel lookup] {int(ok.sum())} of {int(hit.sum())} pixels qualify; largest |lookup - position| = {err.max():.3e}, bar {bar:.3e}")
    assert ok.sum() >= 100
    assert err.max() <= bar


# ------------------------------------------------------------------------------------ with the denoiser
@pytest.mark.parametrize("reached", [False, True])
def test_the_denoiser_takes_the_buffers_as_guides(reached):
    scene = make_scene("path")
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(40, 48, 4, generator=gen)
    f = scene.texel_aovs(x.cuda())
    guides = f.as_guides() if reached else f.data
    out = denoise(x.cuda(), guides, demodulate=False, sigma_depth=0, sigma_albedo=0)
    torch.cuda.synchronize()
    gc = guides.cpu()
    within_bound(out, denoise_ref(x, gc, 4, 0.25, 0.0, 0.0), denoise_ref(x, gc, 4, 0.25, 0.0, 0.0, dtype=torch.float32), float(x.abs().max()),
                 f"texel guides, reached={reached}")


# -------------------------------------------------------------------------------------------- C-ABI
def test_the_entry_points_refuse_what_the_header_says_they_refuse():
    scene = make_scene("path")
    L = N.lib()
    INVALID, UNSUPPORTED = -1, -3
    buf = torch.zeros(8 * 8 * 16 + 8 * 8 * 2 + 64, dtype=torch.float32, device="cuda")
    aovs, ws = buf.data_ptr(), buf.data_ptr() + 4 * 8 * 8 * 16
    st = scene._stream()
    call = lambda h, m, th, tw, a, w: L.zdr_scene_texel_aovs(h, m, th, tw, a, w, st)       # noqa: E731
    assert call(scene._handle, 0, 8, 8, aovs, ws) == 0
    assert call(None, 0, 8, 8, aovs, ws) == INVALID
    assert call(scene._handle, 0, 8, 8, None, ws) == INVALID and call(scene._handle, 0, 8, 8, aovs, None) == INVALID
    assert call(scene._handle, 0, 8, 8, aovs + 4, ws) == INVALID and call(scene._handle, 0, 8, 8, aovs, ws + 8) == INVALID
    for th, tw in ((0, 8), (8, 0), (-1, 8), (8, -3)):
        assert call(scene._handle, 0, th, tw, aovs, ws) == INVALID
        assert L.zdr_texel_aovs_workspace_bytes(th, tw) == 0
    assert call(scene._handle, -1, 8, 8, aovs, ws) == INVALID and call(scene._handle, N.MAX_MATERIALS, 8, 8, aovs, ws) == INVALID
    assert call(scene._handle, N.MAX_MATERIALS - 1, 8, 8, aovs, ws) == 0
    assert call(scene._handle, 0, 8, 8, aovs, aovs + 16) == INVALID                          # the output overlaps the workspace
    assert call(scene._handle, 0, 8, 8, aovs + 256, aovs) == INVALID
    assert call(scene._handle, 0, 8193, 8192, aovs, ws) == UNSUPPORTED and L.zdr_texel_aovs_workspace_bytes(8193, 8192) == 0
    assert b"2^26" in L.zdr_last_error()
    assert L.zdr_texel_aovs_workspace_bytes(8192, 8192) == 8 * 8192 * 8192 and L.zdr_texel_aovs_workspace_bytes(5, 7) == 8 * 35
    torch.cuda.synchronize()
    scene.check()


# ------------------------------------------------------------------------------------------ example
def test_the_example_takes_the_texel_prior_and_masks_the_unreached_texels(tmp_path):
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("optimize_texture_texel", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "optimize_texture.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    plain = ex.run(iters=2, res=32, spp=2, tex=32, verbose=False)
    prior = ex.run(iters=2, res=32, spp=2, tex=32, out=str(tmp_path), verbose=False, texel_prior=0.5, mask_unreached=True)
    assert prior[0] > plain[0] and np.isfinite(prior).all()                                # the prior of a random texture is not 0
    png = np.asarray(Image.open(os.path.join(str(tmp_path), "texture_diffuse.png")))
    scene = make_scene("path")
    reach = scene.texel_aovs(torch.zeros(32, 32, 4, device="cuda")).reach.cpu().numpy()
    assert (reach == 0).sum() > 0 and (png[reach == 0] == 0).all() and (png[reach == 1] > 0).any()
