"""The reference of the texture-space feature buffers (tests/texel_ref.py) on the host, and the cases the GPU test compares with it
(tests/texel_cases.py): the reference against itself (what bilinear lookups touch lies inside reach), the float32 reference against the
float64 one (the margins of profiles/texel_aovs_margins.txt), and the bound on each case's uncertain texels.  Also: the bindings of
zdr_scene_texel_aovs exist.  No GPU."""
import os

import numpy as np
import pytest

import texel_cases as TC
import texel_ref as R
from conftest import ASSETS, ROOT
from zdr_amd import _native, geometry


@pytest.mark.parametrize("name", list(TC.CASES))
def test_what_bilinear_lookups_touch_lies_inside_reach_and_coverage_does_too(name):
    make, slots, material, hw = TC.CASES[name]
    ref = TC.reference(name)
    cov, reach = ref["data"][..., 11] == 1, ref["data"][..., 12] == 1
    touched = R.bilinear_touched(make(), slots, material, hw, 4000 if name.startswith("cbox") else 400, seed=3)
    extra = int((reach & ~touched).sum())
    print(f"[texel ref] {name}: reach {int(reach.sum())}, touched by sampled lookups {int(touched.sum())}, reach beyond them {extra}")
    assert not (touched & ~reach).any()
    assert not (cov & ~reach).any()
    assert touched.sum() > 0 and ((ref["cov_g"] >= 0) == cov).all() and ((ref["reach_g"] >= 0) == reach).all()
    assert (ref["reach_g"][cov] <= ref["cov_g"][cov]).all()               # the reach winner is the lowest g of a larger set
    if name == "cbox_64x64":
        assert extra <= 4                                                # the mask is tight: the rim of measure zero, and what 4,000 samples miss


@pytest.mark.parametrize("name", list(TC.CASES))
def test_at_most_one_percent_of_a_case_is_uncertain(name):
    unc = TC.reference(name)["uncertain"]
    print(f"[texel ref] {name}: {int(unc.sum())} of {unc.size} texels uncertain")
    assert unc.sum() <= TC.MAX_UNCERTAIN * unc.size


@pytest.mark.parametrize("name", list(TC.CASES))
def test_the_float32_reference_agrees_with_float64_within_the_stated_margins(name):
    r64, r32 = TC.reference(name), TC.reference(name, "float32")
    keep = TC.compared(name)
    for key in ("cov_g", "reach_g"):
        assert np.array_equal(r64[key][keep], r32[key][keep]), key
    for ch in (11, 12, 14, 15):
        assert np.array_equal(r64["data"][..., ch][keep], r32["data"][..., ch][keep]), ch
    e = TC.errors(name, r32["data"])
    print(f"[texel ref] {name}: float32 vs float64 position {e[0]:.3e} normal {e[1]:.3e} texel_size {e[2]:.3e}; margins {TC.MARGINS[name]}; bars {TC.bars(name)}")
    for got, m in zip(e, TC.MARGINS[name]):
        assert got <= m and m <= 1.02 * got + 1e-12                       # the constant IS the measurement, rounded up


def test_the_margins_file_states_the_constants():
    txt = open(os.path.join(ROOT, "profiles", "texel_aovs_margins.txt")).read()
    for name in TC.CASES:
        line = [ln for ln in txt.splitlines() if ln.strip().startswith(name + " ")]
        assert line, name
        r64, r32 = TC.reference(name), TC.reference(name, "float32")
        for v in TC.errors(name, r32["data"]):
            assert f"{v:.3e}" in line[0], (name, v, line[0])


def test_the_soup_is_what_it_is_meant_to_be():
    """two waves of slots with the second partial, the large triangles on the cooperative route, slivers that mostly hold no lattice
    point, and texels that several triangles cover: the winner there is the lowest g"""
    A = TC.soup_arrays()
    H, W = TC.SOUP_HW
    assert A.tris.shape[0] == 130
    Q = R.pixel_space(R.world_triangles(A, np.float64)[2], H, W, np.float64)
    covers = np.zeros((130, H, W), bool)
    ys, xs = np.mgrid[0:H, 0:W]
    for g in range(130):
        S = R.Setup(Q[g], np.float64)
        covers[g] = R.classify_points(S, xs.astype(np.float64), ys.astype(np.float64), np.float64)[0]
    assert covers[0].sum() > 64 and covers[1].sum() > 64
    assert (covers[2:102].sum((1, 2)) == 0).sum() > 50 and (covers[2:102].sum((1, 2)) > 0).sum() >= 1
    many = covers.sum(0) >= 2
    assert many.sum() > 100
    ref = TC.reference("soup_130")
    assert np.array_equal(ref["cov_g"][many], covers.argmax(0)[many])
    won = np.unique(ref["cov_g"][ref["cov_g"] >= 0])
    assert (won >= 102).any() and (won < 2).any()                        # the mid-sized triangles win somewhere: the band and the rim
    area2 = np.array([R.Setup(Q[g], np.float64).area2 for g in range(102, 130)])
    assert (area2 > 0).any() and (area2 < 0).any()                       # both windings


def test_degenerate_triangles_reach_by_their_box_alone_and_cover_nothing():
    A = geometry.assemble([(os.path.join(ASSETS, "quad.obj"), None, 0.0)])
    for H, W in ((6, 5), (8, 8)):
        d = R.texel_aovs_ref(A, (0,), 0, (H, W))["data"]
        ys, xs = np.mgrid[0:H, 0:W]
        assert (d[..., 11] == 0).all() and np.array_equal(d[..., 12] == 1, (xs <= 1) & (ys >= H - 2))
        assert (d[..., 7] == 0).all()
    d = R.texel_aovs_ref(A, (0,), 0, (1, 1))["data"]
    assert d[0, 0, 11] == 0 and d[0, 0, 12] == 1
    d = R.texel_aovs_ref(A, (None,), 0, (4, 4))["data"]
    assert (d[..., 12] == 0).all() and (d[..., 14:16] == -1).all() and (d[..., :14] == 0).all()


def test_the_bindings_exist():
    assert "zdr_texel_aovs_workspace_bytes" in _native.EXPORTS and "zdr_scene_texel_aovs" in _native.EXPORTS
    import zdr_amd
    assert hasattr(zdr_amd, "TexelAovs") and hasattr(zdr_amd.Scene, "texel_aovs") and hasattr(zdr_amd.Scene, "texel_aovs_forward")
    assert set(zdr_amd.TexelAovs.CHANNELS) == {"normal", "texel_size", "position", "coverage", "reach", "instance", "slot"}
    header = open(os.path.join(ROOT, "include", "zdr.h")).read()
    assert "zdr_scene_texel_aovs" in header and "#define ZDR_ABI_VERSION 4" in header
