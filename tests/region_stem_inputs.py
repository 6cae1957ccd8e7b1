"""Inputs and fp64 references for the native region-encoder route (test_region_stem_cpu.py, test_region_stem_gpu.py).

Sampling positions come from region_train_inputs.make_coords (built off pixel borders: a position fp32 floors into one cell and fp64
into the next would touch another set of pixels).  Nothing here touches torch.cuda at import."""
import torch
import torch.nn.functional as F

import region_train_inputs as RT
from oracle import region as O


def make_points(L, n, P, h, w, seed, short=None, empty=None):
    """-> coords [L, n, P, 2] fp32 (x, y), valid [L, n, P] bool.  Region ``short`` has fewer valid points than P at every level, region
    ``empty`` none at all; every other point is valid."""
    gen = torch.Generator().manual_seed(seed)
    coords = torch.stack([RT.make_coords(n, P, h, w, gen) for _ in range(L)])
    valid = torch.ones(L, n, P, dtype=torch.bool)
    if short is not None:
        valid[:, short, P // 3:] = False
    if empty is not None:
        valid[:, empty] = False
    return coords, valid


def level_weights_ref(coords, valid, h, w):
    """fp64: A_l[n, pix] / cnt_l[n] for every level, [L, n, h w] -- the masked mean of the sampled one-hot maps, i.e. the weights the
    module's own statements put on every pixel; 0 everywhere for a region without a valid point (the module's nan_to_num)."""
    L, n = valid.shape[:2]
    eye = torch.eye(h * w, dtype=torch.float64).reshape(1, h * w, h, w).expand(n, -1, -1, -1)
    return torch.stack([O.masked_mean(O.point_sample(eye, coords[l].double()), valid[l]) for l in range(L)])


def pool_weights_ref(coords, valid, h, w):
    """fp64: w_k = (1 / L) sum_{l >= k} A_l / cnt_l, [L, n, h w]."""
    a = level_weights_ref(coords, valid, h, w)
    return a.flip(0).cumsum(0).flip(0) / a.shape[0]


def module_pool_statements(stem, levels, coords, valid, up_w, up_b):
    """The statements of RegionEncoder.forward behind the stem, in the tensors' dtype: feat = feat + level, masked mean of the sampled
    points, up_dim, stack, mean.  stem and levels channels-last [n, h, w, C]."""
    feat = stem.permute(0, 3, 1, 2)
    pooled = []
    for l, level in enumerate(levels):
        feat = feat + level.permute(0, 3, 1, 2)
        region = O.masked_mean(O.point_sample(feat, coords[l].to(feat.dtype)), valid[l])
        pooled.append(F.linear(region, up_w, up_b))
    return torch.stack(pooled).mean(dim=0)


def folded_pool(stem, levels, wk, up_w, up_b):
    """The native route's form of the same: pooled = sum_pix (w_0 stem + sum_k w_k level_k), then up_dim once."""
    n, h, w, C = stem.shape
    pooled = (wk[0][:, :, None] * stem.reshape(n, h * w, C)).sum(1)
    for k, level in enumerate(levels):
        pooled = pooled + (wk[k][:, :, None] * level.reshape(n, h * w, C)).sum(1)
    return F.linear(pooled, up_w, up_b)


def im2col_ref(images, masks, patch, kpad):
    """torch restatement of the 4-channel im2col in the tensors' dtype: rows (n, y2, x2, dy, dx), columns (c, ky, kx), zero pad columns."""
    k = patch // 2
    x = torch.cat([images, masks], 1)
    n, _, H, W = x.shape
    h2, w2 = H // patch, W // patch
    cols = F.unfold(x.float(), kernel_size=k, stride=k)                    # [n, 4 k k, (2 h2)(2 w2)], positions (y1, x1)
    cols = cols.reshape(n, 4 * k * k, h2, 2, w2, 2).permute(0, 2, 4, 3, 5, 1)   # n, y2, x2, dy, dx, col
    out = torch.zeros(n * h2 * w2 * 4, kpad)
    out[:, :4 * k * k] = cols.reshape(-1, 4 * k * k)
    return out.to(torch.bfloat16)


def ln_gelu_ref(x, w, b, eps):
    """fp64 of LayerNorm2d's statements on rows + erf GELU -> (pre, y)."""
    x = x.double()
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    pre = w.double() * ((x - u) / torch.sqrt(s + eps)) + b.double()
    return pre, F.gelu(pre)
