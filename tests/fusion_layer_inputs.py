"""Shapes, seeds, mask builders and the fp64 yardsticks of the fusion layer's tests (test_fusion_layer_cpu.py, test_fusion_layer_gpu.py).

The attention kernel (vllm_xattn_fwd_bf16).  q, k, v are randn rounded to bf16, q times 2, so that the scaled scores have a standard
deviation near 2: a softmax that is neither flat nor one-hot.  Short keys (one split): the (Lq, Lk) of SHORT; long keys (split): Lq of
LONG_LQ against Lk3 = the smallest Lk for which vllm_xattn_plan gives three splits with a last split of ONE key.  The yardstick is the
exact masked softmax in fp64 from the bf16 operands (``xattn_reference``: out, mag = sum_j p_j |v_j|, the share of masked keys).

The layer.  Two shapes (LAYER_SHAPES); every parameter is the module's initial value plus 0.1 randn rounded to bf16, ``vision_proj`` /
``text_proj`` are then scaled so that the fp64 scores have a standard deviation of about 2, ``vision_param`` / ``text_param`` are drawn
uniformly from [0.5, 1.5] (at the constructor's 1e-4 the attention output is invisible in bf16 and a broken kernel would pass).  The
yardstick (``reference``) is the mirror's own composed ``forward`` on a ``.double()`` CPU copy; it never calls the native library.

``clamped_attention`` says the reference's statements (global maximum, both clamps, column maximum over ALL keys) in fp64 for one
direction, so that a CPU test can show that the exact softmax and the reference's agree on every input used here.
Nothing here touches torch.cuda at import."""
import copy
import ctypes
import functools
import types

import torch
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import fusion_layer as FL

KEY_TILE = 64
XA_D, XA_H, XA_B = (128, 256), (1, 3), (1, 2)
SHORT = [(300, 1), (300, 7), (65, 64), (130, 65), (130, 256)]
LONG_LQ = (1, 7, 65, 256)
SHORT_PATTERNS = (None, "ragged", "first_key", "dead_image")
LONG_PATTERNS = (None, "ragged", "first_split", "middle_split", "dead_image")


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------
def plan(B, Lq, Lk, H, D):
    """-> (splits, keys_per_split) of vllm_xattn_plan"""
    s, k = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().vllm_xattn_plan(B, Lq, Lk, H, D, ctypes.byref(s), ctypes.byref(k)), "vllm_xattn_plan")
    return s.value, k.value


@functools.lru_cache(maxsize=None)
def lk3(B, Lq, H, D):
    """the smallest Lk whose plan has three splits and a last split of one key"""
    for Lk in range(1, 1 << 14):
        s, kps = plan(B, Lq, Lk, H, D)
        if s == 3 and Lk - 2 * kps == 1:
            return Lk
    raise AssertionError("no Lk below 2^14 gives three splits with a last split of one key")


# ---- the kernel's inputs ------------------------------------------------------------------------------------------------------------------------
def patterns(Lk, long_keys):
    """the mask patterns this Lk can carry"""
    if long_keys:
        return LONG_PATTERNS
    return tuple(p for p in SHORT_PATTERNS if p in (None, "dead_image") or (p == "ragged" and Lk >= 4) or (p == "first_key" and Lk >= 2))


@functools.lru_cache(maxsize=None)
def xattn_inputs(D, Lq, Lk, H, B):
    """-> (q [B, Lq, H D], k, v [B, Lk, H D]) bf16 CPU tensors.  Cached: leave them unchanged."""
    g = torch.Generator().manual_seed(D * 7 + Lq * 131 + Lk * 17 + H * 3 + B)
    q = (2 * torch.randn(B, Lq, H * D, generator=g)).to(torch.bfloat16)
    k = torch.randn(B, Lk, H * D, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Lk, H * D, generator=g).to(torch.bfloat16)
    return q, k, v


def key_mask(pattern, B, Lk, kps=0):
    """-> (bool [B, Lk] with True = ignore the key, or None; the share of keys it says it masks; the images it leaves without a key)"""
    if pattern is None:
        return None, 0.0, []
    m = torch.zeros(B, Lk, dtype=torch.bool)
    if pattern == "ragged":          # image b loses its last (b + 1) Lk // 4 keys
        n = [(b + 1) * Lk // 4 for b in range(B)]
        for b in range(B):
            m[b, Lk - n[b]:] = True
        return m, sum(n) / (B * Lk), []
    if pattern == "first_key":
        m[:, 0] = True
        return m, 1 / Lk, []
    if pattern == "dead_image":      # the last image has no key left
        m[B - 1] = True
        return m, 1 / B, [B - 1]
    if pattern == "first_split":
        m[:, :kps] = True
        return m, kps / Lk, []
    if pattern == "middle_split":
        m[:, kps:2 * kps] = True
        return m, kps / Lk, []
    raise KeyError(pattern)


def exact_attention(q, k, v, mask, scale):
    """q [B, H, Lq, D], k, v [B, H, Lk, D] fp64, mask bool [B, Lk] or None -> (out, mag = sum_j p_j |v_j|, the scaled scores)"""
    s = (q @ k.transpose(-2, -1)) * scale
    sm = s if mask is None else s.masked_fill(mask[:, None, None, :], float("-inf"))
    p = torch.softmax(sm, -1)          # an all -inf row: NaN
    return p @ v, p @ v.abs(), s


def clamped_attention(q, k, v, mask, scale):
    """The same product by the reference's statements (...mask_dn.py:947-977, both directions' treatment at once): the global maximum
    of the call's scores subtracted, clamp to +-50000, the row maximum over ALL keys (masked ones included) subtracted, clamp, mask, softmax."""
    s = (q * scale) @ k.transpose(-2, -1)
    s = s - s.max()
    s = torch.clamp(s, min=-50000, max=50000)
    s = s - torch.max(s, dim=-1, keepdim=True)[0]
    s = torch.clamp(s, min=-50000, max=50000)
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float("-inf"))
    return s.softmax(dim=-1) @ v


def _heads(x, B, H, D):
    return x.double().reshape(B, -1, H, D).transpose(1, 2)


@functools.lru_cache(maxsize=None)
def xattn_reference(D, Lq, Lk, H, B, pattern):
    """-> (out [B, Lq, H, D] fp64 with NaN rows where every key is masked, mag, share of masked keys, score std) on the CPU.  Cached."""
    q, k, v = (_heads(x, B, H, D) for x in xattn_inputs(D, Lq, Lk, H, B))
    mask, _, _ = key_mask(pattern, B, Lk, plan(B, Lq, Lk, H, D)[1])
    out, mag, s = exact_attention(q, k, v, mask, D ** -0.5)
    share = 0.0 if mask is None else mask.double().mean().item()
    return out.transpose(1, 2), mag.transpose(1, 2), share, s.std(unbiased=False).item()


def xattn_clamped(D, Lq, Lk, H, B, pattern):
    q, k, v = (_heads(x, B, H, D) for x in xattn_inputs(D, Lq, Lk, H, B))
    mask, _, _ = key_mask(pattern, B, Lk, plan(B, Lq, Lk, H, D)[1])
    return clamped_attention(q, k, v, mask, D ** -0.5).transpose(1, 2)


def xattn_cases():
    """every (D, Lq, Lk, H, B, long_keys) of the kernel tests"""
    out = []
    for D in XA_D:
        for H in XA_H:
            for B in XA_B:
                out += [(D, Lq, Lk, H, B, False) for Lq, Lk in SHORT]
                out += [(D, Lq, lk3(B, Lq, H, D), H, B, True) for Lq in LONG_LQ]
    return out


# ---- the layer ----------------------------------------------------------------------------------------------------------------------------------
# (split refers to the text -> image direction; S of "split" is Lk3 of its shape)
LAYER_SHAPES = {
    "one_split": dict(B=2, S=300, Lt=7, C=64, FFN=512, HEADS=4),      # embed 256 over 2 heads: head dim 128
    "split": dict(B=2, S=None, Lt=70, C=256, FFN=1024, HEADS=4),      # embed 512 over 2 heads: head dim 256
}
MASKS = ("none", "both", "one_text_token")
DEAD = "dead_text_image"          # image 1 has every text token masked: its vision output is NaN
LAYER_CASES = [(s, m) for s in LAYER_SHAPES for m in MASKS + (DEAD,)]


def shape_of(name):
    d = dict(LAYER_SHAPES[name])
    d["E"], d["H"] = d["FFN"] // 2, d["HEADS"] // 2
    d["D"] = d["E"] // d["H"]
    if d["S"] is None:
        d["S"] = lk3(d["B"], d["Lt"], d["H"], d["D"])
    return types.SimpleNamespace(**d)


def config(name, **kw):
    s = LAYER_SHAPES[name]
    c = dict(d_model=s["C"], encoder_ffn_dim=s["FFN"], encoder_attention_heads=s["HEADS"], fusion_dropout=0.0, fusion_droppath=0.0)
    c.update(kw)
    return types.SimpleNamespace(**c)


def _round(m):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())


def _scores(m, vision, text):
    """the fp64 scaled scores [B, H, S, Lt] of the layer on these inputs"""
    d = copy.deepcopy(m).double()
    a = d.attn
    with torch.no_grad():
        v, t = d.layer_norm_vision(vision.double()), d.layer_norm_text(text.double())
        B = v.shape[0]
        q, k = _heads(a.vision_proj(v), B, a.num_heads, a.head_dim), _heads(a.text_proj(t), B, a.num_heads, a.head_dim)
        return (q @ k.transpose(-2, -1)) * a.scale


@functools.lru_cache(maxsize=None)
def make_layer(name):
    """-> the module in fp32 (eval mode) whose parameters are bf16 values.  Cached: deep-copy before changing it."""
    torch.manual_seed(11)
    m = FL.GroundingDinoFusionLayer(config(name))
    g = torch.Generator().manual_seed(111)
    C = LAYER_SHAPES[name]["C"]
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        m.vision_param.copy_(0.5 + torch.rand(C, generator=g))
        m.text_param.copy_(0.5 + torch.rand(C, generator=g))
    _round(m)
    vision, text = raw_inputs(name)
    for _ in range(2):          # both projections by sqrt(2 / std): the product's deviation goes to 2 (the second pass: after rounding)
        f = (2.0 / _scores(m, vision, text).std(unbiased=False).item()) ** 0.5
        with torch.no_grad():
            for lin in (m.attn.vision_proj, m.attn.text_proj):
                lin.weight.mul_(f)
                lin.bias.mul_(f)
        _round(m)
    return m.eval()


def as_bf16(m, device):
    return copy.deepcopy(m).to(device).to(torch.bfloat16).eval()


@functools.lru_cache(maxsize=None)
def raw_inputs(name):
    s = shape_of(name)
    g = torch.Generator().manual_seed(500 + s.S)
    return torch.randn(s.B, s.S, s.C, generator=g).to(torch.bfloat16), torch.randn(s.B, s.Lt, s.C, generator=g).to(torch.bfloat16)


def layer_masks(name, masks):
    """-> (attention_mask_vision bool [B, S] or None, attention_mask_text bool [B, Lt] or None, share of image tokens / of text tokens masked)"""
    s = shape_of(name)
    vm = tm = None
    if masks in ("both", DEAD):
        vm = torch.zeros(s.B, s.S, dtype=torch.bool)
        vm[0, s.S - s.S // 5:] = True
        vm[1, : s.S // 3] = True
        tm = torch.zeros(s.B, s.Lt, dtype=torch.bool)
        tm[0, s.Lt - 2:] = True
        tm[1, 0] = True
        if masks == DEAD:
            tm[1] = True
    elif masks == "one_text_token":
        tm = torch.ones(s.B, s.Lt, dtype=torch.bool)
        tm[:, 1] = False
    else:
        assert masks == "none"
    return vm, tm


def said_shares(name, masks):
    """what layer_masks says it masks: (share of image tokens, share of text tokens)"""
    s = shape_of(name)
    if masks == "none":
        return 0.0, 0.0
    if masks == "one_text_token":
        return 0.0, (s.Lt - 1) / s.Lt
    v = (s.S // 5 + s.S // 3) / (2 * s.S)
    return v, ((2 + s.Lt) if masks == DEAD else 3) / (2 * s.Lt)


def make_inputs(name, masks):
    """-> dict of CPU tensors: vision [B, S, C], text [B, Lt, C] (bf16), attention_mask_vision / attention_mask_text (bool or None)"""
    vision, text = raw_inputs(name)
    vm, tm = layer_masks(name, masks)
    return dict(vision=vision, text=text, attention_mask_vision=vm, attention_mask_text=tm)


def to(t, device, dtype=None):
    out = {}
    for k, v in t.items():
        if v is not None:
            v = v.to(device)
            v = v.to(dtype) if dtype is not None and v.is_floating_point() else v
        out[k] = v
    return out


def call(m, t):
    """-> (vision_features, text_features, the two weight slots)"""
    (ov, wv), (ot, wt) = m(t["vision"], t["text"], t["attention_mask_vision"], t["attention_mask_text"])
    return ov, ot, (wv, wt)


def reasons(m, t):
    return m.native_layer_reasons(t["vision"], t["text"], t["attention_mask_vision"], t["attention_mask_text"])


@functools.lru_cache(maxsize=None)
def reference(name, masks):
    """-> (vision_features, text_features) of the fp64 module on the bf16-valued inputs.  Computed once on the CPU; leave it unchanged."""
    m = copy.deepcopy(make_layer(name)).double()
    with torch.no_grad():
        ov, ot, _ = call(m, to(make_inputs(name, masks), "cpu", torch.float64))
    return ov, ot


def layer_scores(name):
    return _scores(make_layer(name), *raw_inputs(name))


# ---- routing on a CPU box -------------------------------------------------------------------------------------------------------------------------
class FakeCuda(torch.Tensor):
    """a CPU tensor that says it is on the GPU: the reasons are decided from dtypes, shapes and flags alone"""
    @property
    def is_cuda(self):
        return True


def fake(t):
    return None if t is None else t.as_subclass(FakeCuda)


def fake_module(m):
    m = as_bf16(m, "cpu")
    for mod in m.modules():
        for k, p in list(mod._parameters.items()):
            if p is not None:
                mod._parameters[k] = nn.Parameter(p.data, requires_grad=p.requires_grad).as_subclass(FakeCuda)
    return m
