"""Pins the torch reference of the denoiser (tests/denoise_ref.py) in float64, so that the GPU tests compare the kernels with something
that has itself been checked: fixed points, the adjoint identity, the explicit transpose against autograd, the B3 blur it degenerates
to, and the instance barrier.  No GPU needed."""
import pytest
import torch

from denoise_ref import B3, denoise_ref, denoise_ref_transpose, guides, level_forward, level_weights, synthetic_aovs

SIGMAS = (0.25, 0.1, 0.1)
H, W = 29, 37


@pytest.fixture(scope="module")
def aovs():
    return synthetic_aovs(H, W, 1)


def rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_synthetic_guides_have_every_kind_of_pixel(aovs):
    c, ident = aovs[..., 11], aovs[..., 14]
    assert set(ident.unique().tolist()) == {-1.0, 0.0, 1.0, 2.0}
    assert ((c == 0) & (ident >= 0)).any() and ((c > 0) & (c < 1)).any() and (c == 1).any()
    n, z, a, _ = guides(aovs, torch.float64)
    assert torch.isfinite(n).all() and torch.isfinite(z).all() and torch.isfinite(a).all()
    assert (n[c == 0] == 0).all() and (z[c == 0] == 0).all()


@pytest.mark.parametrize("levels", [1, 3, 6])
def test_a_constant_image_is_a_fixed_point(aovs, levels):
    x = torch.full((H, W, 4), 0.75, dtype=torch.float64)
    x[..., 3] = 1.0
    out = denoise_ref(x, aovs, levels, *SIGMAS)
    assert (out - x).abs().max() <= 1e-14


@pytest.mark.parametrize("levels", [1, 3, 6])
def test_adjoint_identity(aovs, levels):
    x, g = rand((H, W, 4), 2), rand((H, W, 4), 3)
    lhs = (g * denoise_ref(x, aovs, levels, *SIGMAS)).sum()
    rhs = (denoise_ref_transpose(g, aovs, levels, *SIGMAS) * x).sum()
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * abs(lhs), (float(lhs), float(rhs))


@pytest.mark.parametrize("levels", [1, 4])
def test_explicit_transpose_is_what_autograd_gives(aovs, levels):
    x, g = rand((H, W, 4), 4).requires_grad_(), rand((H, W, 4), 5)
    auto, = torch.autograd.grad(denoise_ref(x, aovs, levels, *SIGMAS), x, g)
    mine = denoise_ref_transpose(g, aovs, levels, *SIGMAS)
    assert (auto - mine).abs().max() <= 1e-13 * auto.abs().max()


def test_one_level_without_edge_stopping_is_the_b3_blur_with_renormalised_borders():
    A = torch.zeros(H, W, 16, dtype=torch.float64)
    A[..., 11] = 1.0
    x = rand((H, W, 4), 6)
    b = torch.tensor(B3, dtype=torch.float64)
    for s in (1, 4):
        got = level_forward(x, level_weights(guides(A, torch.float64), s, 0.0, 0.0, 0.0))

        def blur(t, dim):                                         # 1-D, taps outside dropped
            out = torch.zeros_like(t)
            n = t.shape[dim]
            for k in range(-2, 3):
                lo, hi = max(0, -s * k), min(n, n - s * k)
                if lo < hi:
                    out.narrow(dim, lo, hi - lo).add_(b[k + 2] * t.narrow(dim, lo + s * k, hi - lo))
            return out
        num = blur(blur(x, 0), 1)
        den = blur(blur(torch.ones_like(x), 0), 1)
        assert (got - num / den).abs().max() <= 1e-14


@pytest.mark.parametrize("levels", [1, 5])
def test_pixels_of_different_instances_never_mix(aovs, levels):
    ident = aovs[..., 14]
    for k in (-1.0, 1.0):
        x = (ident == k).to(torch.float64)[..., None].expand(H, W, 4).contiguous()
        out = denoise_ref(x, aovs, levels, *SIGMAS)
        assert (out - x).abs().max() <= 1e-14


def test_a_switched_off_sigma_drops_its_term(aovs):
    x = rand((H, W, 4), 7)
    all_on = denoise_ref(x, aovs, 2, *SIGMAS)
    for k in range(3):
        s = list(SIGMAS)
        s[k] = 0.0
        assert (denoise_ref(x, aovs, 2, *s) - all_on).abs().max() > 1e-6
        s[k] = -1.0
        assert torch.equal(denoise_ref(x, aovs, 2, *s), denoise_ref(x, aovs, 2, *[0.0 if i == k else v for i, v in enumerate(SIGMAS)]))
