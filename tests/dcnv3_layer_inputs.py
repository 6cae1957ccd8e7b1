"""Inputs and fp64 references shared by test_dcnv3_layer_cpu.py / test_dcnv3_layer_gpu.py (the native DCNv3 layer, header section f3b).

A case is (C, G, H, W, N, dwk, dilation, center_feature_scale, offset_scale).  Every parameter and the input are rounded to bf16 and then
widened, so the bf16 module, its fp64 twin and the kernels all see the same numbers.  Nothing here touches torch.cuda at import."""
import copy
import math

import torch
import torch.nn.functional as F

from visionllm_amd.dcnv3 import DCNv3

#        C,   G,  H,  W, N, dwk, dil, cfs,   offset_scale
CASES = [
    (64, 4, 5, 7, 2, 5, 1, True, 1.0),       # 28 G = 112 used rows: already a multiple of 8
    (128, 4, 9, 6, 3, 3, 1, False, 1.7),     # 27 G = 108 used rows -> 4 zero rows
    (320, 10, 6, 6, 1, 5, 1, True, 1.0),     # InternImage-H stage 1 channels: 40 lanes per pixel, one partly filled wave
    (64, 4, 7, 5, 2, 3, 2, True, 1.0),       # dilation 2
    (64, 2, 3, 4, 1, 5, 1, False, 1.0),      # dw kernel larger than the map; group channels 32
    (320, 10, 24, 40, 1, 5, 1, True, 1.7),   # several blocks of both kernels, five full strips per row
]
# The offset scales are placed so that the share of accepted sampling points (accepted_share, fp64, seeds = case index) is
# 0.69, 0.53, 0.69, 0.58, 0.51, 0.86: inside the [0.4, 0.9] every test asserts, i.e. both the inside and the border / outside
# branches of the sampling kernel run.  (At the other scale the dilation-2 and the tiny map fall below 0.4, the 24 x 40 map above 0.9.)
IDS = ["c64g4", "c128g4_nocfs", "c320g10", "c64g4_dil2", "c64g2_tiny", "c320g10_blocks"]
FP32_PARAMS = ("center_feature_scale_proj_weight", "center_feature_scale_proj_bias")


def make_module(C, G, dwk, dil, cfs, scale, seed=0, **kw):
    """fp32 CPU module whose parameters hold bf16-representable values: non-zero offset / mask / centre linears (std 1.5 / sqrt(0.43 C):
    x1 = GELU(LayerNorm(.)) has a second moment of about 0.43, so the offsets come out at about 1.5 px), biases of std 0.5, the
    depth-wise conv and its LayerNorm perturbed by 0.2 randn."""
    torch.manual_seed(seed)
    m = DCNv3(channels=C, group=G, dw_kernel_size=dwk, dilation=dil, pad=dil, offset_scale=scale, center_feature_scale=cfs, **kw)
    std = 1.5 / math.sqrt(0.43 * C)
    with torch.no_grad():
        lin = [(m.offset.weight, m.offset.bias), (m.mask.weight, m.mask.bias)]
        if cfs:
            lin.append((m.center_feature_scale_proj_weight, m.center_feature_scale_proj_bias))
        for w, b in lin:
            w.normal_(0, std)
            b.normal_(0, 0.5)
        for p in m.dw_conv.parameters():
            p.add_(0.2 * torch.randn_like(p))
        m.input_proj.bias.normal_(0, 0.1)
        m.output_proj.bias.normal_(0, 0.1)
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return m.eval()


def as_bf16(m, device):
    """The inference-dtype twin: every parameter bf16 except the two centre-feature-scale parameters, which the reference declares fp32."""
    b = copy.deepcopy(m).to(device).to(torch.bfloat16)
    for name in FP32_PARAMS:
        if hasattr(b, name):
            getattr(b, name).data = getattr(b, name).data.float()
    return b


def as_f64(m, device):
    return copy.deepcopy(m).to(device).double()


def make_input(C, H, W, N, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(N, H, W, C, generator=g).to(torch.bfloat16)


def share_of_offsets(off, d, s):
    """off [N, H, W, G * 18] fp64 (x, y pairs, kernel_w-outer / kernel_h-inner points) -> share of the sampling points that pass the
    operator's acceptance test (-1 < x < W, -1 < y < H; a NaN location fails it) at stride 1, pad == dilation == d, offset scale s."""
    N, H, W, _ = off.shape
    off = off.reshape(N, H, W, -1, 3, 3, 2)   # [.., i (kernel_w), j (kernel_h), (x, y)]
    ii = (torch.arange(3, dtype=torch.float64, device=off.device) - 1) * d
    xs = torch.arange(W, dtype=torch.float64, device=off.device)[None, None, :, None, None, None]
    ys = torch.arange(H, dtype=torch.float64, device=off.device)[None, :, None, None, None, None]
    loc_w = xs + (ii[:, None] + off[..., 0]) * s
    loc_h = ys + (ii[None, :] + off[..., 1]) * s
    ok = (loc_w > -1) & (loc_w < W) & (loc_h > -1) & (loc_h < H)
    return ok.double().mean().item()


def accepted_share(m64, x64):
    """share_of_offsets for the offsets the fp64 module computes from x64 [N, H, W, C]."""
    with torch.no_grad():
        off = m64.offset(m64.dw_conv(x64.permute(0, 3, 1, 2)))
    return share_of_offsets(off, m64.dilation, m64.offset_scale)


BAD_OFFSETS = (float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 3e9)


def sampling_rows(G, H, W, N, dil, scale, cfs, pad_cols=8, seed=0):
    """The fp32 rows the fused sampling kernel reads, [N H W, ld_om] with ld_om = round8(used) + pad_cols: 18 G offsets of std 1.6 px,
    9 G logits of std 1.5, G centre logits (with the flag) of std 1.5, then columns the kernel must never read (NaN / inf, the zero
    padding of the packed projection's place included).  Special pixels, where the map has them:
      pixel 0 of image 0: offsets that put every location exactly on an integer (exactly, at scale 1);
      pixel 1: those plus / minus 2^-10;
      pixel 2: locations on the acceptance edges -1, W and H (x of point k on -1 / W alternately, y on H / -1), pixels 3 and 4: those
      moved 2^-10 to the inside and to the outside;
      the last pixel of every image: every point rejected (NaN, +-inf, +-1e30, 3e9 in x).
    -> (om, ld_om, index tensor of the all-rejected rows)"""
    g = torch.Generator().manual_seed(2000 + seed)
    R, used = N * H * W, (28 if cfs else 27) * G
    ld = (used + 7) // 8 * 8 + pad_cols
    om = torch.empty(R, ld)
    om[:, :18 * G] = torch.randn(R, 18 * G, generator=g) * 1.6
    om[:, 18 * G:used] = torch.randn(R, used - 18 * G, generator=g) * 1.5
    om[:, used::2] = float("nan")
    om[:, used + 1::2] = float("inf")
    off = om[:, :18 * G].reshape(R, G, 3, 3, 2)          # a view: [row, g, i, j, (x, y)]
    tap = (torch.arange(3, dtype=torch.float32) - 1) * dil
    eps = 2.0 ** -10
    sign = torch.tensor([1.0, -1.0]).repeat(5)[:9].reshape(3, 3)
    if R >= 6:
        ints = torch.randint(-1, 3, (G, 3, 3, 2), generator=g).float()
        off[0] = ints                                     # pixel (0, 0) of image 0: loc = 0 + ((i - 1) d + int) * scale
        off[1] = ints + eps * sign[None, :, :, None]
        # pixel 2 is (y, x) = (2 // W, 2 % W): loc_w = x + (tap_i + off) * scale = target  <=>  off = (target - x) / scale - tap_i
        for r, delta in ((2, 0.0), (3, eps), (4, -eps)):                                      # on the edge, just inside, just outside
            y, x = r // W, r % W
            tw = torch.where(sign > 0, torch.tensor(-1.0), torch.tensor(float(W)))            # alternate the two edges over the points
            th = torch.where(sign > 0, torch.tensor(float(H)), torch.tensor(-1.0))
            off[r, :, :, :, 0] = ((tw + sign * delta - x) / scale - tap[:, None])[None]
            off[r, :, :, :, 1] = ((th - sign * delta - y) / scale - tap[None, :])[None]
    rejected = torch.arange(N) * H * W + H * W - 1
    bad = torch.tensor(BAD_OFFSETS).repeat(G * 9 // len(BAD_OFFSETS) + 1)[:G * 9].reshape(G, 3, 3)
    off[rejected, :, :, :, 0] = bad
    off[rejected, :, :, :, 1] = 0.0
    return om, ld, rejected


def conv_ln_gelu_ref(x, dw_w, dw_b, ln_w, ln_b, dwk, eps):
    """fp64: x [N, H, W, C], dw_w [C, 1, k, k] -> (GELU_erf(LayerNorm(dwconv(x))), the bound's magnitude
    |gamma| (sum_taps |w x| + |b|) / sigma + |beta|), both [N, H, W, C]."""
    C = x.shape[-1]
    xc = x.double().permute(0, 3, 1, 2)
    w = dw_w.double().reshape(C, 1, dwk, dwk)
    y = F.conv2d(xc, w, dw_b.double(), padding=dwk // 2, groups=C).permute(0, 2, 3, 1)
    # (a NaN input makes its windows NaN in both; the magnitude is only used where the reference is finite)
    a = F.conv2d(xc.abs(), w.abs(), dw_b.double().abs(), padding=dwk // 2, groups=C).permute(0, 2, 3, 1)
    sigma = (y.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
    z = F.layer_norm(y, (C,), ln_w.double(), ln_b.double(), eps)
    return F.gelu(z), ln_w.double().abs() * a / sigma + ln_b.double().abs()


def pack_reference(m):
    """The packed projection as the header states it, built independently of DCNv3.packed_projection: -> (weight, bias, used rows)."""
    ws, bs = [m.offset.weight, m.mask.weight], [m.offset.bias, m.mask.bias]
    if m.center_feature_scale:
        ws.append(m.center_feature_scale_proj_weight)
        bs.append(m.center_feature_scale_proj_bias)
    dt = m.offset.weight.dtype
    w = torch.cat([t.detach().to(dt) for t in ws], 0)
    b = torch.cat([t.detach().to(dt) for t in bs], 0)
    used = w.shape[0]
    pad = (-used) % 8
    return torch.cat([w, w.new_zeros(pad, w.shape[1])], 0), torch.cat([b, b.new_zeros(pad)], 0), used
