"""The NumPy reference of the prefiltered gather (tests/texel_mip_ref.py) pinned on the host: level sizes, both adjoints as exact
transposes in float64, the properties include/zdr.h states for the gather in float32 bit for bit, and the checkerboard that the
bilinear gather aliases on.  No GPU."""
import numpy as np
import pytest

import texel_mip_ref as MR
import texel_project_ref as PR

SIZES = [(7, 5), (1, 9), (24, 16), (33, 17), (2, 1), (1, 1)]           # (width, height)
WANT = {
    (7, 5): [(7, 5), (4, 3), (2, 2), (1, 1)],
    (1, 9): [(1, 9), (1, 5), (1, 3), (1, 2), (1, 1)],
    (24, 16): [(24, 16), (12, 8), (6, 4), (3, 2), (2, 1), (1, 1)],
    (33, 17): [(33, 17), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1)],
    (2, 1): [(2, 1), (1, 1)],
    (1, 1): [(1, 1)],
}


def synthetic(rng, n, res, share=0.8, scale=(0.25, 40.0)):
    """as ``synthetic`` of tests/test_gpu_texel_project.py, with a scale (float 6) drawn log-uniformly"""
    v = np.zeros((n, 1, 8), np.float32)
    v[:, 0, 0] = rng.uniform(0, 1, n) < share
    v[:, 0, 2] = rng.uniform(0, res[0], n); v[:, 0, 3] = rng.uniform(0, res[1], n)
    v[:, 0, 6] = np.exp(rng.uniform(np.log(scale[0]), np.log(scale[1]), n))
    return v


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("res", SIZES)
def test_level_sizes_and_offsets(res):
    lay = MR.layout(res)
    assert [(w, h) for w, h, _ in lay] == WANT[res]
    off = 0
    for w, h, o in lay[1:]:
        assert o == off
        off += w * h
    for levels in (1, 2, 3):
        assert [(w, h) for w, h, _ in MR.layout(res, levels)] == WANT[res][:levels + 1]
    pyr = MR.pyramid_ref(np.ones((res[1], res[0], 4)), 0)
    assert [(v.shape[1], v.shape[0]) for v in pyr] == WANT[res]
    assert MR.pack(pyr).shape == (max(off, 1), 4)


def test_a_level_is_the_box_filter_of_the_border_continued_finer_level():
    x = np.arange(7 * 5 * 4, dtype=np.float64).reshape(5, 7, 4)
    l1 = MR.pyramid_ref(x, 1)[1]
    assert np.array_equal(l1[0, 0], (x[0, 0] + x[0, 1] + x[1, 0] + x[1, 1]) / 4)
    assert np.array_equal(l1[0, 3], (2 * x[0, 6] + 2 * x[1, 6]) / 4)              # the last column counts twice
    assert np.array_equal(l1[2, 3], x[4, 6])                                      # the corner counts four times
    c = np.full((5, 7, 4), np.float32(0.3), np.float32)
    for v in MR.pyramid_ref(c, 0, np.float32):
        assert (bits(v) == bits(np.float32(0.3))).all()


@pytest.mark.parametrize("res", SIZES)
def test_the_pyramid_adjoint_is_the_exact_transpose_in_float64(res):
    rng = np.random.default_rng(5)
    for levels in (0, 1, 2, 3):
        x = rng.normal(size=(res[1], res[0], 4))
        pyr = MR.pyramid_ref(x, levels)
        G = [None] + [rng.normal(size=v.shape) for v in pyr[1:]]
        lhs = sum(float((v * g).sum()) for v, g in zip(pyr[1:], G[1:]))
        rhs = float((x * MR.pyramid_adjoint_ref(G, res, levels)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1e-300), (res, levels, lhs, rhs)


@pytest.mark.parametrize("res", SIZES)
@pytest.mark.parametrize("footprint", [1.0, 3.0, 0.5])
def test_the_gather_adjoint_is_the_exact_transpose_in_float64(res, footprint):
    rng = np.random.default_rng(6)
    view = synthetic(rng, 300, res)
    x, y = rng.normal(size=(res[1], res[0], 4)), rng.normal(size=(300, 1, 4))
    lhs = float((MR.gather_mip_ref(x, view, footprint) * y).sum())
    rhs = float((x * MR.gather_mip_adjoint_ref(y, view, res, footprint)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_the_level_split():
    L = 5
    l0, f = MR.level_split(np.array([np.nan, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 31.9, 32.0, 1e9, np.inf], np.float32), 1.0, L, np.float32)
    assert l0.tolist() == [0, 0, 0, 0, 0, 1, 1, 4, 5, 5, 5]
    assert f[[0, 1, 2, 3, 5, 8, 9, 10]].tolist() == [0.0] * 8 and f.dtype == np.float32
    assert f[4] == np.float32(np.log2(np.float32(1.5))) and 0 < f[7] <= 1
    assert MR.level_split(np.float32(4.0), 0.5, L)[0] == 1 and MR.level_split(np.float32(4.0), 3.0, L)[0] == 3
    assert MR.level_split(np.float32(7.0), 1.0, 0) == (0, 0.0)


@pytest.mark.parametrize("res", SIZES)
def test_the_four_properties_in_float32_bit_for_bit(res):
    rng = np.random.default_rng(7)
    image = rng.normal(size=(res[1], res[0], 4)).astype(np.float32)
    pyr = MR.pyramid_ref(image, 0, np.float32)
    L = len(pyr) - 1
    # 1. wherever s <= 1 the result is the bilinear gather's
    view = synthetic(rng, 300, res, scale=(0.01, 1.0))
    view[:3, 0, 6] = (0.0, 1.0, np.nan)
    assert (bits(MR.gather_mip_ref(image, view, 1.0, 0, np.float32)) == bits(PR.gather_ref(image, view, np.float32))).all()
    # 2. scale = 2^k, footprint 1: the bilinear gather of level k with X, Y scaled by 2^-k
    for k in range(L + 1):
        view = synthetic(rng, 300, res)
        view[:, 0, 6] = 2.0 ** k
        scaled = view.copy()
        scaled[:, 0, 2:4] = view[:, 0, 2:4] * np.float32(2.0 ** -k)
        assert (bits(MR.gather_mip_ref(image, view, 1.0, 0, np.float32)) == bits(PR.gather_ref(pyr[k], scaled, np.float32))).all(), k
    # 3. a constant image comes out as visible x that constant, for any scale
    view = synthetic(rng, 300, res)
    view[:, 0, 0] *= rng.uniform(0.2, 1.0, 300).astype(np.float32)
    const = np.full((res[1], res[0], 4), np.float32(0.3), np.float32)
    got = MR.gather_mip_ref(const, view, 1.0, 0, np.float32)
    assert (bits(got) == bits((view[:, :, 0:1] * np.float32(0.3)).astype(np.float32) * np.ones((1, 1, 4), np.float32))).all()
    # 4. what lies behind an invisible texel never reaches the result
    view = synthetic(rng, 300, res)
    clean = MR.gather_mip_ref(image, view, 1.0, 0, np.float32)
    off = view[:, 0, 0] == 0
    assert off.sum() > 20
    view[off, 0, 2] = np.nan; view[off, 0, 3] = 1e30; view[off, 0, 6] = np.nan
    got = MR.gather_mip_ref(image, view, 1.0, 0, np.float32)
    assert (bits(got) == bits(clean)).all() and (got[off] == 0).all() and not np.isnan(got).any()
    poisoned = [np.full_like(v, np.nan) for v in pyr]
    view[:, 0, 0] = 0
    assert (MR.gather_mip_ref(image, view, 1.0, 0, np.float32, pyramid=poisoned) == 0).all()


def test_a_checkerboard_gathers_to_one_half_where_the_bilinear_gather_aliases():
    rng = np.random.default_rng(8)
    ys, xs = np.mgrid[0:64, 0:64]
    board = np.repeat(((xs + ys) % 2).astype(np.float32)[..., None], 4, -1)
    view = synthetic(rng, 400, (64, 64))
    view[:, 0, 6] = rng.uniform(2.0, 40.0, 400)
    on = view[:, 0, 0] == 1
    got = MR.gather_mip_ref(board, view, 1.0, 0, np.float32)
    assert (got[on] == 0.5).all() and (got[~on] == 0).all()
    plain = PR.gather_ref(board, view, np.float32)[on]
    print(f"[texel mip checkerboard] bilinear standard deviation {plain.std():.3f}")
    assert plain.std() > 0.1
