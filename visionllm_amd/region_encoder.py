"""Region encoder (visual-prompt masks -> one embedding per region): host-side mirror, SURVEY.md section 8 row f4.

Same names and parameter layout as visionllmv2/model/region_encoder.py: ``LayerNorm2d`` (:9-21), ``point_sample``
(:24-47), ``rand_sample`` (:50-65), ``RegionEncoder`` (:68-147).  The convolutional mask embedding stays torch modules
(MIOpen); the per-region pooling of the 'grid_sample' type -- bilinear sampling of up to 2304 points per region and their
masked mean -- is ONE native call (libvllm_hip.so: vllm_point_sample_mean_f32) instead of grid_sample + mask + sum + div.
Under autograd (the feature map requires grad: the reference trains the region encoder) the same forward kernels run inside
``torch.autograd.Function``s whose backward is native too (vllm_point_sample_mean_backward_f32 / _bf16: an outer product of
the region's pixel weights and grad_out, include/vllm_hip.h section f4); gradients with respect to the sampling positions
are not implemented.
``RegionEncoder.native_branch = True`` replaces all of that -- the stem, the per-level add and pooling, up_dim, and torch's
autograd of them -- by ONE native call forward (vllm_region_encoder_forward) and one backward (vllm_region_encoder_backward),
channels-last, bf16, for the configuration the model builds ('grid_sample'); ``rand_sample`` and the point bookkeeping stay here.
"""
import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib


class LayerNorm2d(nn.Module):
    def __init__(self, num_channels: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))
        self.eps = eps

    def forward(self, x):
        u = x.mean(1, keepdim=True)
        s = (x - u).pow(2).mean(1, keepdim=True)
        x = (x - u) / torch.sqrt(s + self.eps)
        return self.weight[:, None, None] * x + self.bias[:, None, None]


def _check_ps(input, point_coords, kwargs):
    if kwargs.get("mode", "bilinear") != "bilinear" or kwargs.get("padding_mode", "zeros") != "zeros" or \
            kwargs.get("align_corners", False):
        raise NotImplementedError("point_sample: the native kernel implements bilinear / zeros / align_corners=False "
                                  "(the only combination the reference uses, region_encoder.py:135)")
    if not input.is_cuda:
        raise RuntimeError("point_sample: input must be a CUDA tensor (no CPU fallback)")
    if input.dim() != 4 or point_coords.shape[-1] != 2 or point_coords.shape[0] != input.shape[0]:
        raise ValueError("point_sample: input must be (N, C, H, W) and point_coords (N, P, 2) or (N, Hg, Wg, 2)")


def _no_coord_grad(who, point_coords):
    if point_coords.requires_grad:
        raise NotImplementedError(f"{who} (native): point_coords requires grad, and the native backward differentiates the "
                                  "feature map only (VisionLLMv2 takes the sampling positions from nonzero())")


def _train_map(input):
    """The differentiable calls take the map in fp32 or bf16; any other dtype is converted here, under autograd."""
    return input if input.dtype in (torch.float32, torch.bfloat16) else input.to(torch.float32)


class _PointSampleMaskedMean(torch.autograd.Function):
    """Masked mean under autograd.  It is linear in the map, so the backward needs only the points: the map is never saved.
    grad_in = (pixel weights / count) (x) grad_out, written once, in the map's dtype (zeros for a region without points)."""

    @staticmethod
    def forward(ctx, input, pts, v):
        N, C, H, W = input.shape
        P = pts.shape[1]
        x = input.to(torch.float32).contiguous()
        out = torch.empty((N, C), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().vllm_point_sample_mean_f32(_lib.ptr(x), _lib.ptr(pts), _lib.ptr(v), N, C, H, W, P, _lib.ptr(out),
                                                             _lib.current_stream(x.device)), "vllm_point_sample_mean_f32")
        ctx.save_for_backward(pts, v)
        ctx.map_shape, ctx.map_dtype = (N, C, H, W), input.dtype
        return out.to(input.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pts, v = ctx.saved_tensors
        N, C, H, W = ctx.map_shape
        P = pts.shape[1]
        g = grad_out.to(torch.float32).contiguous()
        grad_in = torch.empty(ctx.map_shape, dtype=ctx.map_dtype, device=g.device)
        name = "vllm_point_sample_mean_backward_bf16" if ctx.map_dtype == torch.bfloat16 else "vllm_point_sample_mean_backward_f32"
        with torch.cuda.device(g.device):
            ws, nbytes = _lib.sized_workspace(g.device, _lib.lib().vllm_point_sample_backward_workspace_bytes(N, C, H, W, P),
                                              "vllm_point_sample_backward_workspace_bytes")
            _lib.check(getattr(_lib.lib(), name)(_lib.ptr(pts), _lib.ptr(v), _lib.ptr(g), N, C, H, W, P, _lib.ptr(grad_in),
                                                 _lib.ptr(ws), nbytes, _lib.current_stream(g.device)), name)
        return grad_in, None, None


class _PointSample(torch.autograd.Function):
    """point_sample under autograd: grad_in[n, c, pix] = sum_p w(p, pix) grad_out[n, c, p], an fp32 kernel that sums with float
    atomics (the last bits may differ between runs).  Nothing in the model trains through this entry.  The map is not saved."""

    @staticmethod
    def forward(ctx, input, pts):
        N, C, H, W = input.shape
        P = pts.shape[1]
        x = input.to(torch.float32).contiguous()
        out = torch.empty((N, C, P), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().vllm_point_sample_f32(_lib.ptr(x), _lib.ptr(pts), N, C, H, W, P, _lib.ptr(out),
                                                        _lib.current_stream(x.device)), "vllm_point_sample_f32")
        ctx.save_for_backward(pts)
        ctx.map_shape, ctx.map_dtype = (N, C, H, W), input.dtype
        return out.to(input.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (pts,) = ctx.saved_tensors
        N, C, H, W = ctx.map_shape
        P = pts.shape[1]
        g = grad_out.to(torch.float32).contiguous()
        grad_in = torch.empty(ctx.map_shape, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _lib.check(_lib.lib().vllm_point_sample_backward_f32(_lib.ptr(pts), _lib.ptr(g), N, C, H, W, P, _lib.ptr(grad_in), None, 0,
                                                                 _lib.current_stream(g.device)), "vllm_point_sample_backward_f32")
        return grad_in.to(ctx.map_dtype), None


def point_sample(input, point_coords, **kwargs):
    """(N, C, H, W), (N, P, 2) or (N, Hg, Wg, 2) in [0, 1]^2 -> (N, C, P) or (N, C, Hg, Wg).  Differentiable in ``input``."""
    _check_ps(input, point_coords, kwargs)
    N, C, H, W = input.shape
    grid = point_coords.dim() == 4
    pts = _lib.aligned(point_coords.reshape(N, -1, 2).to(torch.float32), 8)   # (coordinate pairs are read as 8-byte vectors)
    if torch.is_grad_enabled() and (input.requires_grad or point_coords.requires_grad):
        _no_coord_grad("point_sample", point_coords)
        out = _PointSample.apply(_train_map(input), pts).to(input.dtype)
        return out.reshape(N, C, point_coords.shape[1], point_coords.shape[2]) if grid else out
    x = input.to(torch.float32).contiguous()
    P = pts.shape[1]
    out = torch.empty((N, C, P), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vllm_point_sample_f32(_lib.ptr(x), _lib.ptr(pts), N, C, H, W, P, _lib.ptr(out),
                                                    _lib.current_stream(x.device)), "vllm_point_sample_f32")
    out = out.to(input.dtype)
    return out.reshape(N, C, point_coords.shape[1], point_coords.shape[2]) if grid else out


def point_sample_masked_mean(input, point_coords, valid):
    """Fused form of region_encoder.py:135-140: mean over the valid points of every region, (N, C).  Differentiable in ``input``
    (region_encoder.py:135-140 trains mask_embedding through grid_sample: here through the native backward)."""
    _check_ps(input, point_coords, {})
    N, C, H, W = input.shape
    pts = _lib.aligned(point_coords.to(torch.float32), 8)   # (coordinate pairs are read as 8-byte vectors)
    P = pts.shape[1]
    v = valid.to(torch.uint8).contiguous()
    if torch.is_grad_enabled() and (input.requires_grad or point_coords.requires_grad):
        _no_coord_grad("point_sample_masked_mean", point_coords)
        return _PointSampleMaskedMean.apply(_train_map(input), pts, v).to(input.dtype)
    x = input.to(torch.float32).contiguous()
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vllm_point_sample_mean_f32(_lib.ptr(x), _lib.ptr(pts), _lib.ptr(v), N, C, H, W, P, _lib.ptr(out),
                                                         _lib.current_stream(x.device)), "vllm_point_sample_mean_f32")
    return out.to(input.dtype)


def rand_sample(x, divisor, max_len):
    """region_encoder.py:50-65: up to ``max_len`` random non-zero positions of a region mask ``x`` [n_masks, H, W], each
    mask channel carrying the same probability mass; rows of the result are (mask id, y / H, x / W), sorted by position."""
    idx = x.nonzero()
    if idx.shape[0] == 0:
        return idx
    pts = idx / divisor                                   # [n, 3]
    ids = idx[:, 0]
    counts = torch.bincount(ids)
    mass = 1.0 / ((counts > 0).sum() * counts[ids])       # 1 / (masks present * points of this mask)
    keep = torch.multinomial(mass.to(pts.dtype), num_samples=min(max_len, mass.numel()), replacement=False).sort()[0]
    return pts[keep]


def _mask_stem(hidden_dim, embed_dim, kernel_size):
    """4-channel (RGB + mask) stem down to the ViT patch grid: stride patch/2, then stride 2 (region_encoder.py:76-84)."""
    return nn.Sequential(
        nn.Conv2d(4, hidden_dim // 4, kernel_size=kernel_size, stride=kernel_size),
        LayerNorm2d(hidden_dim // 4),
        nn.GELU(),
        nn.Conv2d(hidden_dim // 4, hidden_dim, kernel_size=2, stride=2),
        LayerNorm2d(hidden_dim),
        nn.GELU(),
        nn.Conv2d(hidden_dim, embed_dim, kernel_size=1),
    )


_NATIVE_PARAMS = ("mask_embedding.0.weight", "mask_embedding.0.bias", "mask_embedding.1.weight", "mask_embedding.1.bias",
                  "mask_embedding.3.weight", "mask_embedding.3.bias", "mask_embedding.4.weight", "mask_embedding.4.bias",
                  "mask_embedding.6.weight", "mask_embedding.6.bias", "up_dim.weight", "up_dim.bias")   # (_lib.REGION_PARAMS' order)
_NATIVE_SAVED = _lib.pointer_fields(_lib.VllmRegionEncoderSaved)
_MAX_LEVELS = 4


def _native_desc(geo, params, levels):
    hidden, embed, out_dim, patch, n, H, W, P, is_f32, eps = geo
    d = _lib.VllmRegionEncoder(hidden=hidden, embed=embed, out_dim=out_dim, patch=patch, n=n, H=H, W=W, levels=len(levels), points=P,
                               pixel_is_f32=is_f32, eps=eps, **{k: p.data_ptr() for k, p in zip(_lib.REGION_PARAMS, params)})
    for i, lv in enumerate(levels):
        d.level[i], d.level_row_stride[i], d.level_image_stride[i] = lv.data_ptr(), lv.stride(1), lv.stride(0)
    return d


def _native_saved(geo, device):
    hidden, embed, _, patch, n, H, W = geo[:7]
    m2 = n * (H // patch) * (W // patch)
    kpad = (patch * patch + 63) // 64 * 64
    cols = (kpad, hidden // 4, hidden // 4, hidden // 4, hidden, hidden, hidden, embed)
    saved = [torch.empty((4 * m2 if i < 4 else m2, c), dtype=torch.bfloat16, device=device) for i, c in enumerate(cols)]
    return saved + [torch.empty((n, embed), dtype=torch.bfloat16, device=device)]


def _native_forward(geo, images, masks, coords, valid, params, levels):
    """One call of vllm_region_encoder_forward -> (out [n, out_dim] bf16, the tensors it keeps for the backward)."""
    dev = images.device
    L = _lib.lib()
    d = _native_desc(geo, params, levels)
    saved = _native_saved(geo, dev)
    sv = _lib.VllmRegionEncoderSaved(**{k: t.data_ptr() for k, t in zip(_NATIVE_SAVED, saved)})
    out = torch.empty((geo[4], geo[2]), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _lib.sized_workspace(dev, L.vllm_region_encoder_workspace_bytes(ctypes.byref(d)), "vllm_region_encoder_workspace_bytes")
        _lib.check(L.vllm_region_encoder_forward(ctypes.byref(d), _lib.ptr(images), _lib.ptr(masks), _lib.ptr(coords), _lib.ptr(valid), _lib.ptr(out),
                                                 ctypes.byref(sv), _lib.ptr(ws), nbytes, _lib.current_stream(dev)), "vllm_region_encoder_forward")
    return out, saved


class _RegionEncoderFn(torch.autograd.Function):
    """The native region encoder under autograd: vllm_region_encoder_forward / vllm_region_encoder_backward.  Differentiable in the twelve
    parameters and in the levels; the levels themselves are not kept (the pooling is linear in them)."""

    @staticmethod
    def forward(ctx, geo, images, masks, coords, valid, *tensors):
        params, levels = tensors[:12], tensors[12:]
        out, saved = _native_forward(geo, images, masks, coords, valid, params, levels)
        ctx.save_for_backward(coords, valid, *params, *saved)
        ctx.geo, ctx.n_levels = geo, len(levels)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        coords, valid = ctx.saved_tensors[:2]
        params, saved = ctx.saved_tensors[2:14], ctx.saved_tensors[14:]
        geo, nl = ctx.geo, ctx.n_levels
        hidden, embed, _, patch, n, H, W = geo[:7]
        dev = grad_out.device
        need = ctx.needs_input_grad[5:]
        g = _lib.aligned(grad_out.to(torch.bfloat16))
        # (a bias gradient comes out of its weight gradient's launch: a frozen weight beside a trained bias gets a buffer that is dropped)
        want = [need[i] or (i % 2 == 0 and i not in (2, 6) and need[i + 1]) for i in range(12)]
        grads = [torch.empty_like(p) if w else None for p, w in zip(params, want)]
        glev = [torch.empty((n, (H // patch) * (W // patch), embed), dtype=torch.bfloat16, device=dev) if need[12 + i] else None for i in range(nl)]
        gs = _lib.VllmRegionEncoderGrads(**{k: (t.data_ptr() if t is not None else None) for k, t in zip(_lib.REGION_PARAMS, grads)})
        for i, t in enumerate(glev):
            gs.level[i] = t.data_ptr() if t is not None else None
        # (the backward reads no level: the descriptor names none)
        d = _native_desc(geo, params, [])
        d.levels = nl
        sv = _lib.VllmRegionEncoderSaved(**{k: t.data_ptr() for k, t in zip(_NATIVE_SAVED, saved)})
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws, nbytes = _lib.sized_workspace(dev, L.vllm_region_encoder_workspace_bytes(ctypes.byref(d)), "vllm_region_encoder_workspace_bytes")
            _lib.check(L.vllm_region_encoder_backward(ctypes.byref(d), _lib.ptr(coords), _lib.ptr(valid), _lib.ptr(g), ctypes.byref(sv), ctypes.byref(gs),
                                                      _lib.ptr(ws), nbytes, _lib.current_stream(dev)), "vllm_region_encoder_backward")
        grads = [t if nd else None for t, nd in zip(grads, need[:12])]
        return (None, None, None, None, None, *grads, *glev)


class RegionEncoder(nn.Module):
    """region_encoder.py:68-147 with the reference's parameter names (mask_embedding.*, region_query, region_attn.*,
    up_dim.*).  ``native_branch = True`` (grid_sample pooling, bf16) runs the whole branch -- stem, level pooling, up_dim -- as ONE native
    call forward and one backward instead of the torch modules below; the default keeps every statement of ``forward`` as it is."""

    POOL_TYPES = ("mean", "cross_attn", "grid_sample")
    native_branch = False

    def __init__(self, hidden_dim, embed_dim, out_dim, patch_size=14, mask_pool_type="mean"):
        super().__init__()
        if patch_size % 2 != 0:
            raise AssertionError("patch_size must be even (the stem strides by patch_size / 2, then by 2)")
        if mask_pool_type not in self.POOL_TYPES:
            raise AssertionError(f"mask_pool_type must be one of {self.POOL_TYPES}")
        self.patch_size = patch_size
        self.mask_pool_type = mask_pool_type
        self.mask_embedding = _mask_stem(hidden_dim, embed_dim, patch_size // 2)
        if mask_pool_type == "cross_attn":
            self.region_query = nn.Embedding(1, embed_dim)
            self.region_attn = nn.MultiheadAttention(embed_dim=embed_dim, num_heads=8, dropout=0.0, batch_first=True)
        elif mask_pool_type == "grid_sample":
            self.num_points = 2304   # 48 x 48
        self.up_dim = nn.Linear(embed_dim, out_dim)

    # -- the three pooling flavours (:117-141) --
    def _pool_mean(self, feat, masks):
        h, w = feat.shape[-2:]
        inside = F.interpolate(masks.float(), size=(h, w), mode="bilinear", align_corners=False) > 0.5
        feat = feat * inside
        return feat, feat.mean(-1).mean(-1)

    def _pool_attn(self, feat):
        kv = feat.flatten(-2).transpose(1, 2)
        q = self.region_query.weight.unsqueeze(0).repeat(feat.shape[0], 1, 1)
        return kv, self.region_attn(q, kv, kv)[0].squeeze(1)

    def _sample_points(self, masks):
        """The index bookkeeping of one level (:127-134) -> (coords [regions, points, (x, y)], valid [regions, points])."""
        H, W = masks.shape[-2:]
        divisor = torch.tensor([1, H, W], device=masks.device)[None,]
        pts = nn.utils.rnn.pad_sequence([rand_sample(m, divisor, self.num_points) for m in masks], padding_value=-1)
        pts = pts.permute(1, 0, 2)                        # [regions, points, (id, y, x)], -1 padded
        valid = pts.sum(dim=-1) >= 0
        return pts[:, :, -2:].flip(dims=[-1]), valid

    def _pool_points(self, feat, masks):
        return point_sample_masked_mean(feat, *self._sample_points(masks))   # native: sample + masked mean

    def _native_refuse(self, images, masks, image_features):
        """The limits of the native route, each named before any launch."""
        who = "RegionEncoder (native_branch)"
        if self.mask_pool_type != "grid_sample":
            raise NotImplementedError(f"{who}: mask_pool_type '{self.mask_pool_type}': only 'grid_sample' has a native route")
        params = [self.get_parameter(k) for k in _NATIVE_PARAMS]
        hidden, embed, out_dim = params[4].shape[0], params[8].shape[0], params[10].shape[0]
        if hidden % 4 or (hidden // 4) % 64 or hidden % 64:
            raise ValueError(f"{who}: hidden_dim {hidden}: hidden_dim // 4 and hidden_dim must be multiples of 64")
        if embed % 64 or out_dim % 64:
            raise ValueError(f"{who}: embed_dim {embed} and out_dim {out_dim} must be multiples of 64")
        H, W = images.shape[-2:]
        if H % self.patch_size or W % self.patch_size:
            raise ValueError(f"{who}: H {H} and W {W} must be multiples of patch_size {self.patch_size}")
        if not 1 <= len(image_features) <= _MAX_LEVELS:
            raise ValueError(f"{who}: {len(image_features)} levels: at most {_MAX_LEVELS} levels (and at least one)")
        if images.requires_grad or masks.requires_grad:
            raise NotImplementedError(f"{who}: images / masks require grad, and the native backward produces no pixel gradients")
        if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
            raise RuntimeError(f"{who}: the parameters must be bf16 CUDA tensors (no CPU fallback, no other dtype)")
        if not images.is_cuda or images.dtype not in (torch.bfloat16, torch.float32):
            raise RuntimeError(f"{who}: images must be a bf16 or fp32 CUDA tensor")
        return params, hidden, embed, out_dim

    def _forward_native(self, images, masks, image_features):
        image_features = list(image_features)
        params, hidden, embed, out_dim = self._native_refuse(images, masks, image_features)
        masks = masks.to(images.dtype)
        n, (H, W) = len(images), images.shape[-2:]
        hw = (H // self.patch_size) * (W // self.patch_size)
        levels, drawn = [], []
        for level in image_features:
            if level.dim() == 4:
                level = level.permute(0, 2, 3, 1).reshape(n, hw, -1)
            if level.shape != (n, hw, embed):
                raise ValueError(f"RegionEncoder (native_branch): a level of shape {tuple(level.shape)}, expected {(n, hw, embed)}")
            level = level.to(torch.bfloat16)
            # read in place, strided views included (hidden states [:, 1:]); copied only where 16-byte rows fail
            if level.stride(2) != 1 or level.stride(1) % 8 or level.stride(0) % 8 or level.data_ptr() % 16:
                level = _lib.aligned(level)
            levels.append(level)
            drawn.append(self._sample_points(masks))          # (once per level, in level order: the generator use of forward())
        P = max(1, max(c.shape[1] for c, _ in drawn))
        coords = torch.zeros((len(drawn), n, P, 2), dtype=torch.float32, device=images.device)
        valid = torch.zeros((len(drawn), n, P), dtype=torch.uint8, device=images.device)
        for l, (c, v) in enumerate(drawn):
            coords[l, :c.shape[0], :c.shape[1]] = c
            valid[l, :v.shape[0], :v.shape[1]] = v
        geo = (hidden, embed, out_dim, self.patch_size, n, H, W, P, int(images.dtype == torch.float32), self.mask_embedding[1].eps)
        params = [_lib.aligned(p) for p in params]
        images, masks = images.contiguous(), masks.contiguous()
        if torch.is_grad_enabled() and any(t.requires_grad for t in params + levels):
            return _RegionEncoderFn.apply(geo, images, masks, coords, valid, *params, *levels)
        return _native_forward(geo, images, masks, coords, valid, [p.detach() for p in params], [lv.detach() for lv in levels])[0]

    def forward(self, images, masks, image_features):
        assert images.shape[-2:] == masks.shape[-2:]
        if self.native_branch:
            return self._forward_native(images, masks, image_features)
        masks = masks.to(images.dtype)
        feat = self.mask_embedding(torch.cat([images, masks], dim=1))
        n, (h, w) = len(images), feat.shape[-2:]
        pooled = []
        for level in image_features:
            if level.dim() == 3:
                level = level.reshape(n, h, w, -1).permute(0, 3, 1, 2)
            assert feat.shape[-2:] == level.shape[-2:]
            feat = feat + level
            if self.mask_pool_type == "mean":
                feat, region = self._pool_mean(feat, masks)      # (the reference carries the masked map to the next level)
            elif self.mask_pool_type == "cross_attn":
                feat, region = self._pool_attn(feat)             # (and the flattened one here)
            else:
                region = self._pool_points(feat, masks)
            pooled.append(self.up_dim(region))
        return torch.stack(pooled).mean(dim=0)
