"""Inputs, fp64 references and error bounds for the region encoder's backward tests (test_region_train_gpu.py).

Sampling positions are BUILT off pixel borders, not filtered: pixel position = integer cell in [-2, size + 1] + fraction in
[0.02, 0.98], coordinate = (position + 0.5) / size, stored as fp32.  grad_in is continuous across a border, but a position that fp32
floors into one cell and fp64 into the next touches a different set of pixels, and the bounds below count hits per pixel.  Points
outside the map and corners half outside are covered by the cell range."""
import torch

from oracle import region as O

EPS = 2.0 ** -24          # half an ulp of fp32, relative


def make_coords(N, P, H, W, gen):
    cell = torch.stack([torch.randint(-2, W + 2, (N, P), generator=gen), torch.randint(-2, H + 2, (N, P), generator=gen)], -1)
    frac = 0.02 + 0.96 * torch.rand(N, P, 2, generator=gen, dtype=torch.float64)
    size = torch.tensor([W, H], dtype=torch.float64)
    return ((cell.double() + frac + 0.5) / size).to(torch.float32)


def make_case(N, C, H, W, P, seed, unfused=False):
    gen = torch.Generator().manual_seed(seed)
    c = make_coords(N, P, H, W, gen)
    v = torch.rand(N, P, generator=gen) > 0.3
    v[N - 1] = False                                           # the last region: no valid point
    g = torch.randn((N, C, P) if unfused else (N, C), generator=gen)
    return c, v, g


def corners(c, H, W):
    """fp64 corner geometry of fp32 coordinates ``c`` [N, P, 2] -> (pixel index [N, P, 4], in-bounds [N, P, 4]); the pixel position is
    ATen's ((2c - 1 + 1) * size - 1) / 2."""
    c = c.double()
    ix, iy = ((2 * c[..., 0] - 1 + 1) * W - 1) / 2, ((2 * c[..., 1] - 1 + 1) * H - 1) / 2
    x0, y0 = ix.floor().long(), iy.floor().long()
    xs = torch.stack([x0, x0 + 1, x0, x0 + 1], -1)
    ys = torch.stack([y0, y0, y0 + 1, y0 + 1], -1)
    inb = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    return (ys.clamp(0, H - 1) * W + xs.clamp(0, W - 1)), inb


def scatter_per_pixel(values, c, H, W, select=None):
    """sum over the (point, in-bounds corner) pairs of ``values`` [N, K, P] into [N, K, H * W]; ``select`` [N, P] drops points."""
    N, K, P = values.shape
    pix, inb = corners(c, H, W)
    if select is not None:
        inb = inb & select[..., None]
    out = torch.zeros(N, K, H * W, dtype=torch.float64)
    for n in range(N):
        for k in range(4):
            m = inb[n, :, k]
            out[n].index_add_(1, pix[n, m, k], values[n][:, m].double())
    return out


def weight_error(H, W):
    """One corner weight against fp64 on the same fp32 coordinates: the kernel computes the pixel position in fp32 (four roundings on
    values up to 2.4 * size: <= 4.3 * size * 2^-24), a weight is a product of two such factors."""
    return 10 * (max(H, W) + 2) * EPS


def mean_reference(c, v, g, C, H, W):
    """fp64 autograd of masked_mean(point_sample(x, c), v) (it does not depend on x: the expression is linear)."""
    N = c.shape[0]
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    out = O.masked_mean(O.point_sample(x, c.double()), v)
    return torch.autograd.grad(out, x, g.double())[0]


def mean_bound(ref, c, v, g, H, W):
    """|err| <= 4 * 2^-24 |ref| + (d + 2^-40) (hits[n, pix] / cnt_n) |grad_out[n, c]|: A[n, pix] sums hits[n, pix] weights exactly
    (integers, each truncated by < 2^-40), then three roundings (A to float, / cnt, * g)."""
    N, P = v.shape
    hits = scatter_per_pixel(torch.ones(N, 1, P), c, H, W, select=v)[:, 0]            # [N, HW]
    cnt = v.sum(1).clamp(min=1).double()
    per_pix = (weight_error(H, W) + 2.0 ** -40) * hits / cnt[:, None]
    return 4 * EPS * ref.abs() + (per_pix[:, None, :] * g.abs().double()[:, :, None]).reshape(ref.shape)


def unfused_reference(c, g, H, W):
    N, C, P = g.shape
    x = torch.zeros(N, C, H, W, dtype=torch.float64, requires_grad=True)
    out = O.point_sample(x, c.double())
    return torch.autograd.grad(out, x, g.double())[0]


def unfused_bound(c, g, H, W):
    """Pixel pix of channel c sums k = hits[n, pix] terms in fp32, each weight off by at most d:
    |err| <= (k + 4) 2^-24 S + d S',  S = sum_p w |grad_out| (the fp64 backward run on |grad_out|), S' = sum of |grad_out[n, c, p]|
    over the points with a corner on pix."""
    N, C, P = g.shape
    S = unfused_reference(c, g.abs(), H, W).reshape(N, C, H * W)
    hits = scatter_per_pixel(torch.ones(N, 1, P), c, H, W)
    S1 = scatter_per_pixel(g.abs(), c, H, W)
    return ((hits + 4) * EPS * S + weight_error(H, W) * S1).reshape(N, C, H, W)
