"""Reference of the à-trous denoiser (include/zdr.h, zdr_denoise) in plain torch, for any float dtype and device: the forward, and
its transpose WRITTEN OUT as a scatter (each tap's w(p, q) g(p) / D(p) is added at q), not obtained from autograd and not relying on
the symmetry of the weights.  A helper, not a test; tests/test_denoise_ref.py pins it in float64."""
import torch

B3 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def guides(aovs, dtype):
    """(n, z, a, id) of the (H, W, 16) feature buffers: divided by coverage where it is positive, 0 elsewhere; id = channel 14."""
    A = aovs.to(dtype)
    c = A[..., 11:12]
    hit = c > 0
    safe = torch.where(hit, c, torch.ones_like(c))
    zero = torch.zeros_like(c)
    n = torch.where(hit, A[..., 4:7] / safe, zero)
    z = torch.where(hit, A[..., 7:8] / safe, zero)[..., 0]
    a = torch.where(hit, A[..., 0:3] / safe, zero)
    return n, z, a, A[..., 14]


def _windows(H, W, s, i, j):
    """Slices (of p, of q = p + s (i, j)) over the pixels p whose tap lies inside the image; None when there are none."""
    dy, dx = s * j, s * i
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def level_weights(g, s, sigma_normal, sigma_depth, sigma_albedo):
    """[(slices of p, slices of q, w(p, q))] for the taps of step s that exist."""
    n, z, a, ident = g
    H, W = z.shape
    taps = []
    for j in range(-2, 3):
        for i in range(-2, 3):
            win = _windows(H, W, s, i, j)
            if win is None:
                continue
            P, Q = win
            T = torch.zeros_like(z[P])
            if sigma_normal > 0:
                T = T + ((n[P] - n[Q]) ** 2).sum(-1) / sigma_normal ** 2
            if sigma_depth > 0:
                T = T + (z[P] - z[Q]) ** 2 / ((sigma_depth * 0.5 * (z[P] + z[Q])) ** 2 + 1e-20)
            if sigma_albedo > 0:
                T = T + ((a[P] - a[Q]) ** 2).sum(-1) / sigma_albedo ** 2
            w = B3[i + 2] * B3[j + 2] * (ident[P] == ident[Q]).to(z.dtype) * torch.exp(-T)
            taps.append((P, Q, w))
    return taps


def _normaliser(taps, like):
    D = torch.zeros_like(like)
    for P, _, w in taps:
        D[P] += w
    return D


def level_forward(x, taps):
    acc = torch.zeros_like(x)
    for P, Q, w in taps:
        acc[P] = acc[P] + w[..., None] * x[Q]
    return acc / _normaliser(taps, x[..., 0])[..., None]


def level_transpose(g, taps):
    h = g / _normaliser(taps, g[..., 0])[..., None]
    out = torch.zeros_like(g)
    for P, Q, w in taps:
        out[Q] = out[Q] + w[..., None] * h[P]
    return out


def denoise_ref(image, aovs, levels, sigma_normal, sigma_depth, sigma_albedo, dtype=torch.float64):
    """out = K_{L-1} ... K_0 image, computed in ``dtype``."""
    g = guides(aovs, dtype)
    x = image.to(dtype)
    for lvl in range(levels):
        x = level_forward(x, level_weights(g, 1 << lvl, sigma_normal, sigma_depth, sigma_albedo))
    return x


def denoise_ref_transpose(d_out, aovs, levels, sigma_normal, sigma_depth, sigma_albedo, dtype=torch.float64):
    """d_image = K_0^T ... K_{L-1}^T d_out, computed in ``dtype``."""
    g = guides(aovs, dtype)
    x = d_out.to(dtype)
    for lvl in reversed(range(levels)):
        x = level_transpose(x, level_weights(g, 1 << lvl, sigma_normal, sigma_depth, sigma_albedo))
    return x


def synthetic_aovs(H, W, seed, dtype=torch.float32):
    """(H, W, 16) feature buffers that exercise every branch of the guides: instance ids -1, 0, 1, 2 in blocks whose edges are not
    multiples of any tile size, pixels of coverage 0 (with and without an id) and of fractional coverage, smooth normals and depth
    with a step across them, albedo premultiplied by coverage like the rest."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    A = torch.zeros(H, W, 16, dtype=torch.float64)
    ident = ((xx + 3) // 11 + 2 * ((yy + 5) // 13)) % 4 - 1            # blocks of 11 x 13, offset by (3, 5)
    cov = torch.ones(H, W, dtype=torch.float64)
    r = torch.rand(H, W, generator=gen, dtype=torch.float64)
    cov = torch.where(r < 0.15, torch.zeros_like(cov), cov)            # nothing hit, id kept or not (below)
    cov = torch.where((r >= 0.15) & (r < 0.4), 0.25 + 0.5 * torch.rand(H, W, generator=gen, dtype=torch.float64), cov)
    cov = torch.where(ident < 0, torch.zeros_like(cov), cov)
    ident = torch.where((cov == 0) & (r < 0.08), -torch.ones_like(ident), ident)
    n = torch.stack([torch.sin(0.2 * xx), torch.cos(0.3 * yy), torch.ones_like(xx)], -1) + 0.1 * torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    n = n / n.norm(dim=-1, keepdim=True)
    z = 3.0 + 0.05 * xx + 0.02 * yy + 2.0 * (xx > 0.6 * W) + 0.05 * torch.randn(H, W, generator=gen, dtype=torch.float64)
    alb = 0.5 + 0.3 * torch.sin(0.5 * xx[..., None] + torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)) + 0.05 * torch.randn(H, W, 3, generator=gen, dtype=torch.float64)
    A[..., 0:3] = alb * cov[..., None]
    A[..., 3] = 0.5 * cov
    A[..., 4:7] = n * cov[..., None]
    A[..., 7] = z * cov
    A[..., 11] = cov
    A[..., 14] = ident
    A[..., 15] = torch.where(ident >= 0, torch.zeros_like(ident), -torch.ones_like(ident))
    return A.to(dtype)


def denoise_full_ref(image, aovs, levels, sigma_normal, sigma_depth, sigma_albedo, demodulate, albedo_floor, dtype=torch.float64):
    """zdr_amd.denoise in ``dtype`` on top of denoise_ref: the demodulation around the linear core, the core's weights taken from the
    DETACHED feature buffers (no gradient through them), so that autograd of this function is the derivative the product defines."""
    image, aovs = image.to(dtype), aovs.to(dtype)
    core = lambda x: denoise_ref(x, aovs.detach(), levels, sigma_normal, sigma_depth, sigma_albedo, dtype)   # noqa: E731
    if not demodulate:
        return core(image)
    m = demodulation_ref(aovs, albedo_floor)
    filtered = core(torch.cat([image[..., :3] / m, image[..., 3:]], -1))
    return torch.cat([filtered[..., :3] * m, filtered[..., 3:]], -1)


def demodulation_ref(aovs, albedo_floor):
    """m of the issue, written from its sentence and not from the product's code: 1 everywhere, and where coverage (channel 11) is
    positive and the slot (channel 15) is not negative, albedo (channels 0..2) / coverage, raised to the floor where it is below."""
    H, W = aovs.shape[:2]
    m = torch.ones(H, W, 3, dtype=aovs.dtype)
    rows = ((aovs[..., 11] > 0) & (aovs[..., 15] >= 0)).nonzero(as_tuple=True)
    mean_albedo = aovs[rows][:, 0:3] / aovs[rows][:, 11:12]
    m[rows] = torch.maximum(mean_albedo, torch.full_like(mean_albedo, albedo_floor))
    return m
