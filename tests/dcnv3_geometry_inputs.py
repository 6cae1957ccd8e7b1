"""Case table, inputs and the independent fp64 reference shared by test_dcnv3_geometry_cpu.py / test_dcnv3_geometry_gpu.py: the DCNv3
operator with kernel, stride, pad and dilation that DIFFER between h and w.  Nothing here touches torch.cuda or the oracle.

A geometry is (kh, kw, sh, sw, ph, pw, dh, dw).  Ten entries change one pair at a time, so a failure names the pair; `all` / `all_T`
change every pair at once, each being the other with h and w exchanged.  kh * kw is 5, 6 or 9: the windowed backward's 4-point
pseudo-levels end ragged, and both tiled forwards (<= 9 points) accept every entry."""
import zlib

import numpy as np
import torch

GEOMETRIES = {
    #          kh kw sh sw ph pw dh dw
    "k3x2":   (3, 2, 1, 1, 1, 1, 1, 1),
    "k2x3":   (2, 3, 1, 1, 1, 1, 1, 1),
    "k5x1":   (5, 1, 1, 1, 2, 0, 1, 1),
    "k1x5":   (1, 5, 1, 1, 0, 2, 1, 1),
    "s1x2":   (3, 3, 1, 2, 1, 1, 1, 1),
    "s2x1":   (3, 3, 2, 1, 1, 1, 1, 1),
    "p0x2":   (3, 3, 1, 1, 0, 2, 1, 1),
    "p2x0":   (3, 3, 1, 1, 2, 0, 1, 1),
    "d1x2":   (3, 3, 1, 1, 1, 2, 1, 2),
    "d2x1":   (3, 3, 1, 1, 2, 1, 2, 1),
    "all":    (3, 2, 1, 2, 2, 1, 2, 1),
    "all_T":  (2, 3, 2, 1, 1, 2, 1, 2),
}
NAMES = list(GEOMETRIES)
MAPS = [(19, 26), (5, 23)]     # several 8 x 8 output tiles with ragged right / bottom tiles; an output lower than one tile
SCALES = (1.0, 1.7)
N, G = 2, 2
# standard deviation of the offsets in pixels per (entry, map); 2.5 (the recipe of test_backward_f32_vs_oracle) unless a case would
# leave the accepted-share band [0.30, 0.95] that test_dcnv3_geometry_cpu.py asserts
OFFSET_SPREAD = {}


def scale_of(name):
    """the one scale of a parameter set that takes one: 1.0 and 1.7 alternate over the table"""
    return SCALES[NAMES.index(name) % 2]


def out_size(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    """dcnv3_cuda.cu:40-45"""
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def _rng(*what):
    return np.random.default_rng(zlib.crc32("/".join(str(w) for w in what).encode()))


def make_points(name, H, W):
    """-> (offset [N, Ho, Wo, G kh kw 2], mask [N, Ho, Wo, G kh kw]) in fp32: normal offsets, uniform mask; the same for every channel
    count and scale, so the conditions the CPU test asserts on them hold for every GPU case."""
    kh, kw = GEOMETRIES[name][:2]
    Ho, Wo = out_size(H, W, *GEOMETRIES[name])
    rng = _rng("points", name, H, W)
    off = (rng.standard_normal((N, Ho, Wo, G * kh * kw * 2)) * OFFSET_SPREAD.get((name, H, W), 2.5)).astype(np.float32)
    msk = rng.random((N, Ho, Wo, G * kh * kw)).astype(np.float32)
    return off, msk


def make_inputs(name, H, W, C):
    """-> (input, offset, mask, grad_out) in fp32 for C channels per group: standard-normal input and grad_out."""
    Ho, Wo = out_size(H, W, *GEOMETRIES[name])
    off, msk = make_points(name, H, W)
    rng = _rng("maps", name, H, W, C)
    inp = rng.standard_normal((N, H, W, G * C)).astype(np.float32)
    go = rng.standard_normal((N, Ho, Wo, G * C)).astype(np.float32)
    return inp, off, msk, go


def locations(off, H, W, kh, kw, sh, sw, ph, pw, dh, dw, scale):
    """Sampling locations (loc_h, loc_w), each [N, Ho, Wo, G, kh kw], in the dtype of `off` (a torch tensor): the statements of
    dcnv3_im2col_cuda.cuh:232-260 -- p0, the centre term, kernel_w OUTER / kernel_h INNER point order,
    loc = p0_ + (i * dilation + offset) * offset_scale."""
    n, Ho, Wo, _ = off.shape
    off = off.reshape(n, Ho, Wo, -1, kh * kw, 2)
    p0_w = ((dw * (kw - 1)) >> 1) - pw + torch.arange(Wo, dtype=off.dtype) * sw
    p0_h = ((dh * (kh - 1)) >> 1) - ph + torch.arange(Ho, dtype=off.dtype) * sh
    p0_w_ = p0_w - ((dw * (kw - 1)) >> 1) * scale
    p0_h_ = p0_h - ((dh * (kh - 1)) >> 1) * scale
    i = torch.arange(kw, dtype=off.dtype).repeat_interleave(kh)    # for i < kernel_w: for j < kernel_h
    j = torch.arange(kh, dtype=off.dtype).repeat(kw)
    loc_w = p0_w_[None, None, :, None, None] + (i * dw + off[..., 0]) * scale
    loc_h = p0_h_[None, :, None, None, None] + (j * dh + off[..., 1]) * scale
    return loc_h, loc_w


def accepted_share(case):
    """case = (name, H, W, scale) -> the share of sampling points that pass the operator's acceptance test (-1 < x < W, -1 < y < H),
    in fp64."""
    name, H, W, scale = case
    off, _ = make_points(name, H, W)
    loc_h, loc_w = locations(torch.from_numpy(off).double(), H, W, *GEOMETRIES[name], scale)
    return float(((loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)).double().mean())


def reference_fp64(inp, off, msk, kh, kw, sh, sw, ph, pw, dh, dw, group, group_channels, scale):
    """The operator as dcnv3_im2col_cuda.cuh:232-260 states it, in torch fp64 on the CPU, unoptimised and differentiable in `inp`, `off`
    and `msk` (torch tensors): locations, floor, four corners gathered by index under their validity masks, times the mask weight,
    summed over the points in the kernel's order.  Written from the reference's statements, not from oracle/dcnv3_oracle.c."""
    n, H, W, _ = inp.shape
    _, Ho, Wo, _ = off.shape
    K, C = kh * kw, group_channels
    loc_h, loc_w = locations(off.double(), H, W, kh, kw, sh, sw, ph, pw, dh, dw, scale)
    ok = (loc_h > -1) & (loc_w > -1) & (loc_h < H) & (loc_w < W)
    h_low, w_low = torch.floor(loc_h.detach()), torch.floor(loc_w.detach())
    lh, lw = loc_h - h_low, loc_w - w_low
    hh, hw = 1 - lh, 1 - lw
    im = inp.double().reshape(n, H * W, group, C).permute(0, 2, 1, 3)               # [n, G, H W, C]
    val = 0
    for y, x, wgt in ((h_low, w_low, hh * hw), (h_low, w_low + 1, hh * lw), (h_low + 1, w_low, lh * hw), (h_low + 1, w_low + 1, lh * lw)):
        valid = ok & (y >= 0) & (y <= H - 1) & (x >= 0) & (x <= W - 1)
        idx = (y.clamp(0, H - 1) * W + x.clamp(0, W - 1)).long().permute(0, 3, 1, 2, 4).reshape(n, group, Ho * Wo * K, 1)
        v = torch.gather(im, 2, idx.expand(-1, -1, -1, C)).reshape(n, group, Ho, Wo, K, C).permute(0, 2, 3, 1, 4, 5)
        val = val + torch.where(valid, wgt, torch.zeros_like(wgt))[..., None] * v   # [n, Ho, Wo, G, K, C]
    m = msk.double().reshape(n, Ho, Wo, group, K)
    col = 0
    for p in range(K):
        col = col + val[..., p, :] * m[..., p, None]
    return col.reshape(n, Ho, Wo, group * C)


def reference_grads(inp, off, msk, go, geo, group, group_channels, scale):
    """numpy operands -> (out, grad_input, grad_offset, grad_mask) of reference_fp64 and torch's fp64 autograd, as numpy fp64."""
    a, b, c = (torch.from_numpy(np.asarray(t, np.float64)).requires_grad_(True) for t in (inp, off, msk))
    out = reference_fp64(a, b, c, *geo, group, group_channels, scale)
    out.backward(torch.from_numpy(np.asarray(go, np.float64)))
    return out.detach().numpy(), a.grad.numpy(), b.grad.numpy(), c.grad.numpy()
