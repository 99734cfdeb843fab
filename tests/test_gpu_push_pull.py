"""-m gpu: the push-pull kernels (zdr_push_pull, zdr_push_pull_backward) against the torch reference of tests/push_pull_ref.py on synthetic
weights — no scene — and, with the Cornell box, the Python layer around them.

The bar of every parity check is the project's measured one (tests/test_gpu_denoise.py): the reference runs in float64 and in float32,
and the kernels' result must satisfy  max|hip - ref64| <= 8 max(max|ref32 - ref64|, 2^-20 max|input|).  Both sides are printed.
What the definition makes exact — known texels, an all-zero weight, what sits behind weight 0, repeatability — is compared as bits."""
import pytest
import torch

from push_pull_ref import WEIGHT_KINDS, make_weight, push_pull_ref, push_pull_ref_transpose
from test_gpu_denoise import within_bound
from zdr_amd import push_pull
from zdr_amd.pushpull import push_pull_backward, push_pull_forward, workspace_bytes

pytestmark = pytest.mark.gpu

# (W, H): one texel; a single row and a single column, where the clamp of U acts on every tap; one push; odd sizes inside the fused tail
# (one workgroup, at most 32 x 32 texels at its base); one level launched above the tail; odd at nearly every level, with four levels
# launched above the tail (257 x 131 -> 129 x 66 -> 65 x 33 -> 33 x 17 -> 17 x 9, the first that fits it)
SIZES = [(1, 1), (7, 1), (1, 7), (2, 2), (5, 3), (37, 29), (257, 131)]
CASES = [(w, h, k) for (w, h) in SIZES for k in WEIGHT_KINDS]

_inputs, _refs = {}, {}


def inputs(W, H, kind):
    """weight, texture and cotangent of one case (float32, CPU), made once; x and g positive, so that nothing cancels"""
    if (W, H, kind) not in _inputs:
        gen = torch.Generator().manual_seed(100 * W + H)
        x = torch.rand(H, W, 4, generator=gen) * torch.tensor([2.0, 1.0, 0.5, 1.0]) + 0.125
        g = torch.rand(H, W, 4, generator=gen) + 0.5
        _inputs[(W, H, kind)] = (make_weight(kind, H, W), x, g)
    return _inputs[(W, H, kind)]


def refs(W, H, kind, levels=None):
    """(forward64, forward32, adjoint64, adjoint32) of one case, computed once and shared"""
    key = (W, H, kind, levels)
    if key not in _refs:
        w, x, g = inputs(W, H, kind)
        _refs[key] = (push_pull_ref(x, w, levels), push_pull_ref(x, w, levels, dtype=torch.float32),
                      push_pull_ref_transpose(g, w, levels), push_pull_ref_transpose(g, w, levels, dtype=torch.float32))
    return _refs[key]


def parity(W, H, kind, levels=None):
    w, x, g = inputs(W, H, kind)
    y = push_pull_forward(x.cuda(), w.cuda(), levels=levels)
    dx = push_pull_backward(g.cuda(), w.cuda(), levels=levels)
    torch.cuda.synchronize()
    f64, f32, a64, a32 = refs(W, H, kind, levels)
    what = f"{W}x{H} {kind} levels={levels}"
    _, bound = within_bound(y, f64, f32, float(x.abs().max()), what + " forward")
    within_bound(dx, a64, a32, float(g.abs().max()), what + " adjoint")
    return y.cpu(), dx.cpu(), bound


@pytest.mark.parametrize("W,H,kind", CASES)
def test_forward_and_adjoint_match_the_reference(W, H, kind):
    parity(W, H, kind)


@pytest.mark.parametrize("W,H,kind", CASES)
def test_adjoint_identity(W, H, kind):
    """<g, K x> = <K^T g, x>, the dot products accumulated in float64 on the host"""
    w, x, g = inputs(W, H, kind)
    Kx = push_pull_forward(x.cuda(), w.cuda()).cpu().double()
    Ktg = push_pull_backward(g.cuda(), w.cuda()).cpu().double()
    lhs, rhs = float((g.double() * Kx).sum()), float((Ktg * x.double()).sum())
    print(f"[push-pull adjoint] {W}x{H} {kind}: <g, Kx> = {lhs:.9g}  <K^T g, x> = {rhs:.9g}  rel = {abs(lhs - rhs) / max(abs(lhs), 1e-30):.3e}")
    assert abs(lhs - rhs) <= 1e-4 * abs(lhs)
    assert (lhs > 1e-3) == bool((w > 0).any())                     # nothing known: K = 0


@pytest.mark.parametrize("W,H,kind", CASES)
def test_what_the_definition_makes_exact_holds_bit_for_bit(W, H, kind):
    w, x, g = (t.cuda() for t in inputs(W, H, kind))
    y, dx = push_pull_forward(x, w), push_pull_backward(g, w)
    assert torch.equal(y[w == 1], x[w == 1])                         # known texels: the same bits
    assert torch.equal(dx[w == 0], torch.zeros_like(dx[w == 0]))     # no gradient lands on a hole
    if kind == "ones":
        assert torch.equal(y, x) and torch.equal(dx, g)
    if not bool((w > 0).any()):
        assert torch.equal(y, torch.zeros_like(y)) and torch.equal(dx, torch.zeros_like(dx))
    # what sits behind weight 0 is never read into the result
    hole = (w == 0)[..., None]
    bad = torch.where(hole, torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38], device="cuda").expand_as(x), x)
    assert torch.equal(push_pull_forward(bad, w), push_pull_forward(torch.where(hole, torch.zeros_like(x), x), w))
    assert torch.equal(push_pull_forward(bad, w), y)
    # two calls give the same bits, also with one workspace shared by forward and adjoint and filled with NaN bytes before
    assert torch.equal(push_pull_forward(x, w), y) and torch.equal(push_pull_backward(g, w), dx)
    ws = torch.full((workspace_bytes((W, H)),), 0xFF, dtype=torch.uint8, device="cuda")
    assert torch.equal(push_pull_backward(g, w, workspace=ws), dx)
    assert torch.equal(push_pull_forward(x, w, workspace=ws), y)
    assert torch.equal(push_pull_backward(g, w, workspace=ws), dx)
    assert torch.equal(push_pull_forward(x, w, workspace=ws), y)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert torch.equal(push_pull_forward(x, w > 0), push_pull_forward(x, (w > 0).float()))      # a bool weight is converted


@pytest.mark.parametrize("W,H,kind", [c for c in CASES if c[2] != "zeros"])
def test_every_output_texel_lies_within_the_known_inputs(W, H, kind):
    """convexity, per channel, widened by the parity bar of the case; a texture that is constant where w > 0 comes out constant"""
    w, x, _ = inputs(W, H, kind)
    if not bool((w > 0).any()):
        return                                                     # (a sparse weight on a tiny texture: covered by the exact test)
    y, _, bound = parity(W, H, kind)
    known = x[w > 0]
    lo, hi = known.min(0).values, known.max(0).values
    print(f"[push-pull convexity] {W}x{H} {kind}: below by {float((lo - y).max()):.3e}, above by {float((y - hi).max()):.3e}, allowed {bound:.3e}")
    assert bool((y >= lo - bound).all()) and bool((y <= hi + bound).all())
    c = torch.tensor([0.5, 2.0, 0.25, 1.0])
    const = torch.where((w > 0)[..., None], c.expand(H, W, 4), torch.full((H, W, 4), float("nan")))
    out = push_pull_forward(const.cuda(), w.cuda()).cpu()
    assert float((out - c).abs().max()) <= 8 * 2.0 ** -20 * 2.0


@pytest.mark.parametrize("kind", WEIGHT_KINDS)
@pytest.mark.parametrize("W,H,levels", [(37, 29, 1), (37, 29, 2), (257, 131, 1), (257, 131, 3)])
def test_a_pyramid_cut_short_matches_the_reference_and_leaves_unreachable_holes_zero(W, H, levels, kind):
    """37 x 29: the cut-off top is inside the fused tail; 257 x 131: it lies below it (levels=1: its own launch) or at its base"""
    y, dx, _ = parity(W, H, kind, levels)
    f64, _, a64, _ = refs(W, H, kind, levels)
    assert torch.equal(y[f64 == 0], torch.zeros_like(y[f64 == 0])) and torch.equal(dx[a64 == 0], torch.zeros_like(dx[a64 == 0]))
    if kind == "corner":
        assert int((f64 == 0).all(-1).sum()) > H * W // 2            # most of the texture is out of the single texel's reach


def test_arguments_are_checked():
    w, x, _ = (t.cuda() for t in inputs(37, 29, "binary"))
    with pytest.raises(ValueError, match="workspace"):
        push_pull_forward(x, w, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="out"):
        push_pull_forward(x, w, out=torch.empty(29, 37, 3, device="cuda"))
    with pytest.raises(ValueError, match="weight"):
        push_pull(x, w[:-1])
    with pytest.raises(ValueError, match="GPU"):
        push_pull(x, w.cpu())


# ----------------------------------------------------------------------------------------------------------------- with a scene
def test_the_cornell_box_through_a_filled_material():
    """material = push_pull(theta, coverage) as a reparameterisation: the gradient of a render lands on covered texels only, and is the
    adjoint kernel applied to the gradient of the filled material, bit for bit"""
    from conftest import fd_material_np
    from gpu_util import make_scene
    scene = make_scene("path")
    theta = torch.from_numpy(fd_material_np(64, 0)).cuda().requires_grad_()
    f = scene.texel_aovs(theta)
    cov = f.coverage
    assert 0 < int((cov == 0).sum()) < 64 * 64 and not cov.is_contiguous()      # a view into the (H, W, 16) tensor, with holes
    m = push_pull(theta, cov)
    m.retain_grad()
    scene.render(m, res=(32, 32), spp=1, seed=3).sum().backward()
    torch.cuda.synchronize()
    assert float(m.grad.abs().sum()) > 0 and bool(torch.isfinite(theta.grad).all())
    assert torch.equal(theta.grad[cov == 0], torch.zeros_like(theta.grad[cov == 0]))
    assert torch.equal(theta.grad, push_pull_backward(m.grad, cov))
    spilled = float(m.grad[cov == 0].abs().sum())
    print(f"[push-pull cbox] texels without coverage: {int((cov == 0).sum())}; |gradient| that landed on them and was carried back: {spilled:.4g} "
          f"of {float(m.grad.abs().sum()):.4g}")
    assert torch.equal(m.detach()[cov == 1], theta.detach()[cov == 1])
    assert torch.equal(f.fill(theta), m) and torch.equal(f.fill(theta.detach(), by="reach"), push_pull(theta.detach(), f.reach))
    w = cov.cpu()
    within_bound(m.detach(), push_pull_ref(theta.detach().cpu(), w), push_pull_ref(theta.detach().cpu(), w, dtype=torch.float32),
                 float(theta.detach().abs().max()), "cbox 64x64 coverage forward")
    scene.check()
