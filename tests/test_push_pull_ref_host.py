"""The push-pull reference of tests/push_pull_ref.py against itself, in float64 and without a GPU: the forward's dense matrix is the
transpose of the adjoint's, its rows sum to 1, and the properties include/zdr.h (zdr_push_pull) states hold."""
import pytest
import torch

from push_pull_ref import WEIGHT_KINDS, dense, level_sizes, make_weight, push_pull_ref, push_pull_ref_transpose

SIZES = [(1, 1), (7, 1), (1, 7), (2, 2), (5, 3), (16, 16), (37, 29)]      # (W, H)


def texture(H, W, seed=0):
    return torch.rand(H, W, 4, generator=torch.Generator().manual_seed(31 * H + W + seed), dtype=torch.float64) + 0.25


@pytest.mark.parametrize("W,H", [(5, 3), (4, 4)])
@pytest.mark.parametrize("kind", ["binary", "fractional", "charts", "corner", "ones"])
@pytest.mark.parametrize("levels", [None, 1])
def test_the_dense_forward_is_the_transpose_of_the_dense_adjoint_and_its_rows_sum_to_one(W, H, kind, levels):
    w = make_weight(kind, H, W)
    if kind == "binary":
        w[0, 0] = 1.0                                              # (never all zero at these sizes)
    K = dense(lambda x: push_pull_ref(x, w, levels), H, W)
    Kt = dense(lambda g: push_pull_ref_transpose(g, w, levels), H, W)
    assert float((K - Kt.T).abs().max()) <= 1e-15
    rows = K.sum(1)
    if levels is None:
        assert float((rows - 1).abs().max()) <= 1e-14               # every texel is reached by the full pyramid
    else:
        assert float(rows.max()) <= 1 + 1e-14                       # cut short, U also mixes in top texels that nothing reached: 0
    assert float(K.min()) >= 0


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", WEIGHT_KINDS)
def test_the_properties_of_the_definition(W, H, kind):
    w, x, g = make_weight(kind, H, W), texture(H, W), texture(H, W, 1)
    y, dx = push_pull_ref(x, w), push_pull_ref_transpose(g, w)
    lhs, rhs = float((g * y).sum()), float((dx * x).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)            # <g, K x> = <K^T g, x>
    assert torch.equal(dx[w == 0], torch.zeros_like(dx[w == 0]))
    if not bool((w > 0).any()):                                    # "zeros", and a sparse weight on a tiny texture
        assert torch.equal(y, torch.zeros_like(y)) and torch.equal(dx, torch.zeros_like(dx))
        return
    if kind == "ones":
        assert torch.equal(y, x) and torch.equal(dx, g)
    assert torch.equal(y[w == 1], x[w == 1])
    known = x[w > 0]
    lo, hi = known.min(0).values, known.max(0).values              # convexity, per channel
    assert bool((y >= lo - 1e-12).all()) and bool((y <= hi + 1e-12).all())
    c = torch.tensor([0.5, 2.0, -3.0, 1.0], dtype=torch.float64)
    const = torch.where((w > 0)[..., None], c.expand(H, W, 4), texture(H, W, 2))
    assert float((push_pull_ref(const, w) - c).abs().max()) <= 1e-12


@pytest.mark.parametrize("W,H", SIZES)
def test_a_single_texel_in_the_far_corner_fills_the_whole_texture(W, H):
    x = texture(H, W)
    y = push_pull_ref(x, make_weight("corner", H, W))
    assert float((y - x[H - 1, W - 1]).abs().max()) <= 1e-12


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("kind", ["binary", "fractional", "charts", "corner"])
def test_what_sits_behind_weight_zero_changes_nothing(W, H, kind):
    w, x = make_weight(kind, H, W), texture(H, W)
    bad = x.clone()
    hole = (w == 0)
    bad[hole] = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e300], dtype=torch.float64)
    assert torch.equal(push_pull_ref(bad, w), push_pull_ref(torch.where(hole[..., None], torch.zeros_like(x), x), w))
    assert torch.equal(push_pull_ref(bad, w, dtype=torch.float32), push_pull_ref(x, w, dtype=torch.float32))
    wn = w.clone()
    wn[hole] = float("nan")                                        # a NaN weight is weight 0
    assert torch.equal(push_pull_ref(x, wn), push_pull_ref(x, w))


def test_levels_stop_where_they_should():
    assert level_sizes(29, 37) == [(29, 37), (15, 19), (8, 10), (4, 5), (2, 3), (1, 2), (1, 1)]
    assert level_sizes(29, 37, 1) == [(29, 37), (15, 19)] and level_sizes(29, 37, 2) == [(29, 37), (15, 19), (8, 10)]
    assert level_sizes(1, 1, 3) == [(1, 1)] and level_sizes(29, 37, 50) == level_sizes(29, 37)
    H, W = 29, 37
    x = texture(H, W)
    w = torch.zeros(H, W)
    w[0, 0] = 1.0
    for levels, reach in ((1, 4), (2, 8)):
        # the top level holds one known texel; pulling down, the bilinear taps carry it two texels further per level
        y = push_pull_ref(x, w, levels)
        filled = (y != 0).any(-1)
        assert bool(filled[:reach // 2, :reach // 2].all()) and not bool(filled[reach:, :].any()) and not bool(filled[:, reach:].any())
        assert float((y[filled] - x[0, 0]).abs().max()) > 0         # cut short, a hole's weights no longer sum to 1 everywhere
    full = push_pull_ref(x, w)
    assert float((full - x[0, 0]).abs().max()) <= 1e-12
