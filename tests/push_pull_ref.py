"""Reference of zdr_push_pull and its adjoint (include/zdr.h), in torch, written from the definition there with explicit loops over the
levels; ``dtype`` selects float64 (the truth of the parity tests) or float32 (the yardstick: what another correct float32 evaluation
differs from the truth by).  Everything stays on the device the inputs are on: the tests run it on the CPU, tools/push_pull_cost.py
times it on the GPU.  The upsampling U is a gather here and its transpose a scatter (index_add_), where the kernels gather both ways:
tests/test_push_pull_ref_host.py checks the two against each other through their dense matrices."""
import torch

WEIGHT_KINDS = ("binary", "fractional", "charts", "corner", "zeros", "ones")


def level_sizes(H, W, levels=None):
    """[(H_0, W_0), ..., (H_L, W_L)]: halved and rounded up until 1 x 1, or ``levels`` times if that comes first."""
    sizes = [(H, W)]
    while sizes[-1] != (1, 1) and (levels is None or len(sizes) - 1 < levels):
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def _quads(t):
    """the four children (2i + {0, 1}, 2j + {0, 1}) of every coarse texel; children outside the level are 0"""
    h, w = t.shape[:2]
    full = torch.zeros((h + h % 2, w + w % 2) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
    full[:h, :w] = t
    return full[0::2, 0::2], full[0::2, 1::2], full[1::2, 0::2], full[1::2, 1::2]


def push_weights(a):
    a00, a01, a10, a11 = _quads(a)
    S = (a00 + a01) + (a10 + a11)
    a1 = S.clamp(max=1.0)
    r = torch.where(S > 0, a1 / torch.where(S > 0, S, torch.ones_like(S)), torch.zeros_like(S))
    return a1, r


def taps(nf, nc, device=None):
    """the two taps of U for every fine index of an axis: c = i >> 1 and nb = c + 1 (i odd) or c - 1 (i even), clamped"""
    i = torch.arange(nf, device=device)
    c = i >> 1
    return c, torch.where(i % 2 == 1, c + 1, c - 1).clamp(0, nc - 1)


def upsample(v, hf, wf):
    """U: (hc, wc, C) -> (hf, wf, C), along the rows first, then across them"""
    cx, nx = taps(wf, v.shape[1], v.device)
    cy, ny = taps(hf, v.shape[0], v.device)
    t = 0.75 * v[:, cx] + 0.25 * v[:, nx]
    return 0.75 * t[cy] + 0.25 * t[ny]


def upsample_t(h, hc, wc):
    """U^T: (hf, wf, C) -> (hc, wc, C), every fine texel scattered to its taps"""
    cx, nx = taps(h.shape[1], wc, h.device)
    cy, ny = taps(h.shape[0], hc, h.device)
    t = torch.zeros((hc,) + tuple(h.shape[1:]), dtype=h.dtype, device=h.device)
    t.index_add_(0, cy, 0.75 * h)
    t.index_add_(0, ny, 0.25 * h)
    out = torch.zeros((hc, wc) + tuple(h.shape[2:]), dtype=h.dtype, device=h.device)
    out.index_add_(1, cx, 0.75 * t)
    out.index_add_(1, nx, 0.25 * t)
    return out


def _a0(w, dtype):
    return torch.nan_to_num(w.to(dtype), nan=0.0).clamp(0.0, 1.0)


def _over(v, a):
    """v / a where a > 0, else 0"""
    pos = (a > 0)[..., None]
    return torch.where(pos, v / torch.where(a > 0, a, torch.ones_like(a))[..., None], torch.zeros_like(v))


def push_pull_ref(x, w, levels=None, dtype=torch.float64):
    """y = K x of include/zdr.h (zdr_push_pull); x (H, W, 4), w (H, W)"""
    x = x.to(dtype)
    sizes = level_sizes(x.shape[0], x.shape[1], levels)
    L = len(sizes) - 1
    a = [_a0(w, dtype)]
    p = [torch.where(a[0][..., None] > 0, a[0][..., None] * x, torch.zeros_like(x))]
    for l in range(L):                                             # push
        a1, r = push_weights(a[l])
        p00, p01, p10, p11 = _quads(p[l])
        a.append(a1)
        p.append(((p00 + p01) + (p10 + p11)) * r[..., None])
    y = _over(p[L], a[L])                                          # top
    for l in range(L - 1, -1, -1):                                 # pull
        y = p[l] + (1.0 - a[l])[..., None] * upsample(y, *sizes[l])
    return torch.where(a[0][..., None] == 1, x, y)


def push_pull_ref_transpose(g, w, levels=None, dtype=torch.float64):
    """d_x = K^T g of include/zdr.h (zdr_push_pull_backward); g (H, W, 4), w (H, W)"""
    g = g.to(dtype)
    sizes = level_sizes(g.shape[0], g.shape[1], levels)
    L = len(sizes) - 1
    a, r, G = [_a0(w, dtype)], [None], [g]
    for l in range(L):
        a1, r1 = push_weights(a[l])
        a.append(a1)
        r.append(r1)
        G.append(upsample_t((1.0 - a[l])[..., None] * G[l], *sizes[l + 1]))
    q = _over(G[L], a[L])
    for l in range(L - 1, -1, -1):
        py, px = torch.arange(sizes[l][0], device=g.device) >> 1, torch.arange(sizes[l][1], device=g.device) >> 1
        q = G[l] + (r[l + 1][..., None] * q)[py][:, px]
    return torch.where(a[0][..., None] > 0, a[0][..., None] * q, torch.zeros_like(q))


def dense(fn, H, W):
    """the (4 H W) x (4 H W) float64 matrix of a linear map of (H, W, 4) textures, column by column"""
    n = H * W * 4
    M = torch.zeros(n, n, dtype=torch.float64)
    for k in range(n):
        e = torch.zeros(n, dtype=torch.float64)
        e[k] = 1.0
        M[:, k] = fn(e.reshape(H, W, 4)).reshape(-1)
    return M


def make_weight(kind, H, W, seed=0):
    """the weights of the tests, float32 (H, W)"""
    gen = torch.Generator().manual_seed(1000 * H + W + 7 * seed)
    if kind == "binary":                                           # density 0.3
        return (torch.rand(H, W, generator=gen) < 0.3).float()
    if kind == "fractional":                                       # half the texels 0, the others in (0, 1]
        u, keep = torch.rand(H, W, generator=gen), torch.rand(H, W, generator=gen) < 0.5
        return torch.where(keep, u.clamp_min(1.0 / 64), torch.zeros_like(u))
    if kind == "charts":                                           # two rectangles with a gap between them, like charts
        w = torch.zeros(H, W)
        w[H // 8: max(H // 8 + 1, H // 2 - H // 16), W // 8: max(W // 8 + 1, (3 * W) // 4)] = 1.0
        w[H // 2 + H // 16 + (H > 2): max(H // 2 + H // 16 + (H > 2), H - H // 8), W // 4: max(W // 4 + 1, W - W // 8)] = 1.0
        return w
    if kind == "corner":                                           # one texel of weight 0.25 in the far corner
        w = torch.zeros(H, W)
        w[H - 1, W - 1] = 0.25
        return w
    if kind == "zeros":
        return torch.zeros(H, W)
    if kind == "ones":
        return torch.ones(H, W)
    raise KeyError(kind)
