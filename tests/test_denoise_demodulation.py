"""The albedo ``zdr_amd.denoise(demodulate=True)`` divides by, on hand-made feature rows — torch code, no GPU needed: which channels it
reads, where it is 1, and the floor.  The expected values are written out by hand from the rule (m = max(albedo / coverage, floor)
where coverage > 0 and slot >= 0, else 1), so that neither the product's code nor the reference's decides what is right."""
import pytest
import torch

from denoise_ref import demodulation_ref
from zdr_amd.denoiser import demodulation_albedo


def row(albedo, coverage, instance, slot):
    r = torch.full((16,), 7.0)                       # every channel the rule does not name holds a value that would show if read
    r[0:3] = torch.tensor(albedo)
    r[11], r[14], r[15] = coverage, instance, slot
    return r


ROWS = [  # (feature row, expected m)
    (row([0.4, 0.2, 0.1], 1.0, 0, 0), [0.4, 0.2, 0.1]),              # a plain hit
    (row([0.2, 0.1, 0.05], 0.5, 0, 0), [0.4, 0.2, 0.1]),             # premultiplied by a fractional coverage
    (row([0.4, 0.004, 0.0], 1.0, 0, 2), [0.4, 0.01, 0.01]),          # below the floor, and exactly 0
    (row([0.001, 0.001, 0.001], 0.25, 3, 1), [0.01, 0.01, 0.01]),    # 0.004 after the division: still below
    (row([0.0, 0.0, 0.0], 0.0, -1, -1), [1.0, 1.0, 1.0]),            # nothing hit
    (row([0.3, 0.3, 0.3], 0.0, 0, 0), [1.0, 1.0, 1.0]),              # coverage 0 with a slot: no division by 0
    (row([0.0, 0.0, 0.0], 1.0, 1, -1), [1.0, 1.0, 1.0]),             # a hit without a material (a light): slot -1, instance >= 0
    (row([0.5, 0.5, 0.5], 1.0, -1, 0), [0.5, 0.5, 0.5]),             # the slot decides, not the instance
]


def test_m_on_hand_made_rows():
    data = torch.stack([r for r, _ in ROWS]).reshape(2, 4, 16)
    want = torch.tensor([m for _, m in ROWS]).reshape(2, 4, 3)
    got = demodulation_albedo(data, 1e-2)
    assert got.shape == (2, 4, 3) and torch.isfinite(got).all()
    assert torch.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    assert torch.allclose(demodulation_ref(data, 1e-2), want, rtol=1e-6, atol=0)
    assert torch.allclose(demodulation_albedo(data, 0.3)[0, 0], torch.tensor([0.4, 0.3, 0.3]))


def test_m_carries_gradient_to_albedo_and_coverage_only_and_never_a_nan():
    data = torch.stack([r for r, _ in ROWS]).reshape(2, 4, 16).double().requires_grad_()
    g, = torch.autograd.grad(demodulation_albedo(data, 1e-2).sum(), data)
    assert torch.isfinite(g).all()
    others = [c for c in range(16) if c not in (0, 1, 2, 11)]
    assert (g[..., others] == 0).all()
    assert float(g[0, 0, 0]) == pytest.approx(1.0) and float(g[0, 1, 0]) == pytest.approx(2.0)          # d(a / c) / da = 1 / c
    assert float(g[0, 1, 11]) == pytest.approx(-(0.2 + 0.1 + 0.05) / 0.25, rel=1e-6)                    # d(a / c) / dc = -a / c^2, three channels
    assert (g[0, 2, 1:3] == 0).all() and (g[1, 0:3] == 0).all()                                             # clamped, or m = 1: no gradient
