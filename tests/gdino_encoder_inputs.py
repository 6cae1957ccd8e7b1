"""Modules, inputs and the fp64 yardsticks of the Grounding-DINO encoder's tests (test_gdino_encoder_cpu.py, test_gdino_encoder_gpu.py).

Two module configurations:
    a   d_model  64 / encoder_attention_heads 4 / encoder_ffn_dim  512 / levels [[6, 5], [3, 2]]         / B 3   enhancer D 32, fusion D 128
    b   d_model 128 / encoder_attention_heads 4 / encoder_ffn_dim 1024 / levels [[8, 7], [4, 4], [2, 2]] / B 2   enhancer D 64, fusion D 256
(the enhancer and the fusion layer run encoder_attention_heads / 2 = 2 heads).  Every parameter is the module's own initial value plus
0.2 randn rounded to bf16 (deform_encoder_layer_inputs.py), ``vision_param`` / ``text_param`` are drawn from [0.5, 1.5], so that the fp64
module and the bf16 module hold the same numbers.  One thing more, as fusion_layer_inputs.py does it: the query / key projections of
every fusion layer (``vision_proj``, ``text_proj``) and of every enhancer inside an encoder (rows 0 .. 2C of ``in_proj``) are then
scaled by one factor each so that their fp64 attention scores have a standard deviation of about 2, and the fusion layers' output
projections so that what a fusion layer adds to its normalised input has about unit size (the two blocks behind it have no LayerNorm in
front).  At the raw 0.2 randn the fused tokens are five times unit size and the scores
have a standard deviation of 4 to 7 at head dims 32 .. 256: softmaxes that are nearly one-hot, where an error in P V hides, and where a
near-tie flips with the rounding of the layer's INPUT to bf16 -- the composed bf16 module is then 3 to 16 % away from its own fp64 run
and the comparison of two bf16 routes measures luck.  test_gdino_encoder_cpu.py asserts the score deviations on the fp64 run.

Text: Lt tokens in phrases that differ per image (Lt 1: one phrase; Lt 5: two, split behind token (2, 3, 1)[b]; longer: lengths that
cycle); ``text_self_attention_masks`` [B, Lt, Lt] is True inside a phrase (what the reference is given: it inverts it), position ids
restart per phrase, the text padding mask pads the last token of every image but the first (its row of the self-attention mask keeps
the diagonal, so every row has a key).  Vision: the padding mask pads the tail of image b, 12 % + 8 % b of its rows; valid ratios lie in
(0.5, 1] and one is exactly 1.

The enhancer alone is fed ``enh_text`` / ``enh_pos``: ``text`` / ``text_pos`` times the one factor per configuration (``enhancer_scale``)
that gives the fp64 attention scores of its module a standard deviation of about 2 -- a softmax that is neither flat nor one-hot, as the
other attention tests arrange it (at the raw inputs the 0.2 randn on ``in_proj`` gives scores with a standard deviation of 4 to 7:
nearly one-hot rows, where an error in P V hides and one near-tie decides a ten-row figure).  Inside the encoder the enhancer sees the
fusion layer's output as it comes.

The yardstick (``reference_*``) is the mirror itself on a ``.double()`` CPU copy with the deformable operator replaced by the
reference's pure-PyTorch twin (deform_encoder_layer_inputs.cpu_operator); it never calls the native library.  Nothing here touches
torch.cuda at import."""
import copy
import functools
import types

import torch

from deform_encoder_layer_inputs import cpu_operator
from oracle import msda as O
from visionllm_amd import gdino_encoder as G

CONFIGS = {
    "a": dict(C=64, HEADS=4, FFN=512, maps=[(6, 5), (3, 2)], B=3),
    "b": dict(C=128, HEADS=4, FFN=1024, maps=[(8, 7), (4, 4), (2, 2)], B=2),
}
SEEDS = {"a": 31, "b": 32}
LTS = (1, 5, 70)


def tokens(name):
    return sum(h * w for h, w in CONFIGS[name]["maps"])


def config(name, n_layers=1, **kw):
    c = CONFIGS[name]
    d = dict(d_model=c["C"], encoder_ffn_dim=c["FFN"], encoder_attention_heads=c["HEADS"], fusion_dropout=0.0, fusion_droppath=0.1,
             text_enhancer_dropout=0.0, activation_function="relu", num_feature_levels=len(c["maps"]), encoder_n_points=4, dropout=0.1,
             activation_dropout=0.0, disable_custom_kernels=False, encoder_layers=n_layers)
    d.update(kw)
    return types.SimpleNamespace(**d)


def _score_std(q, k, H):
    """standard deviation of q . k / sqrt(D) over heads; q [n, H D], k [m, H D]"""
    q, k = q.reshape(q.shape[0], H, -1), k.reshape(k.shape[0], H, -1)
    return (torch.einsum("qhd,khd->hqk", q, k) / q.shape[-1] ** 0.5).std().item()


def _perturb(m, seed, condition=True):
    """every parameter += 0.2 randn, the layer scales from [0.5, 1.5]; then (``condition``) the query / key projections of the fusion
    layers and of the enhancers inside an encoder are scaled by one factor each so that their fp64 scores on unit-normal tokens have a
    standard deviation of about 2 (module docstring); everything rounded to bf16"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p + 0.2 * torch.randn(p.shape, generator=g))
        for mod in m.modules():
            if isinstance(mod, G.GroundingDinoFusionLayer):
                for p in (mod.vision_param, mod.text_param):
                    p.copy_(0.5 + torch.rand(p.shape, generator=g))
        x, y = torch.randn(256, 1, generator=g), torch.randn(256, 1, generator=g)
        for mod in m.modules() if condition else ():
            if isinstance(mod, G.GroundingDinoFusionLayer):
                C = mod.attn.vision_dim
                xv, xt = torch.randn(256, C, generator=g), torch.randn(64, C, generator=g)
                std = _score_std(mod.attn.vision_proj(mod.layer_norm_vision(xv)), mod.attn.text_proj(mod.layer_norm_text(xt)), mod.attn.num_heads)
                for lin in (mod.attn.vision_proj, mod.attn.text_proj):
                    lin.weight.mul_((2.0 / std) ** 0.5)
                    lin.bias.mul_((2.0 / std) ** 0.5)
                # and the output projections so that what the layer adds to its (normalised) input has about unit size: the deformable
                # layer and the enhancer behind it have no LayerNorm in front and would otherwise see tokens five times unit size
                for out, val, ln, xs in ((mod.attn.out_vision_proj, mod.attn.values_text_proj, mod.layer_norm_text, xt),
                                         (mod.attn.out_text_proj, mod.attn.values_vision_proj, mod.layer_norm_vision, xv)):
                    size = out(val(ln(xs))).std().item()
                    out.weight.div_(size)
                    out.bias.div_(size)
            if isinstance(mod, G.GroundingDinoEncoderLayer):          # its enhancer sees the fusion layer's text (about unit size) + a sine embedding
                mha = mod.text_enhancer_layer.self_attn
                C = mha.embed_dim
                xq = torch.randn(256, C, generator=g) + 0.7 * torch.randn(256, C, generator=g)
                W, b = mha.in_proj_weight, mha.in_proj_bias
                std = _score_std(xq @ W[:C].T + b[:C], xq @ W[C:2 * C].T + b[C:2 * C], mha.num_heads)
                W[:2 * C].mul_((2.0 / std) ** 0.5)
                b[:2 * C].mul_((2.0 / std) ** 0.5)
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    return m.eval()


def make_encoder(name, n_layers=1, **kw):
    """-> GroundingDinoEncoder in fp32 (eval mode) whose parameters are bf16 values"""
    torch.manual_seed(SEEDS[name] + 10 * n_layers)
    return _perturb(G.GroundingDinoEncoder(config(name, n_layers, **kw)), 100 + SEEDS[name] + 10 * n_layers)


def make_enhancer(name, **kw):
    torch.manual_seed(SEEDS[name] + 5)
    return _perturb(G.GroundingDinoTextEnhancerLayer(config(name, **kw)), 300 + SEEDS[name])


def as_bf16(m, device):
    return copy.deepcopy(m).to(device).to(torch.bfloat16).eval()


def phrases(b, Lt):
    """-> [(lo, hi)] of image b's phrases"""
    if Lt == 1:
        return [(0, 1)]
    if Lt == 5:
        cut = (2, 3, 1)[b % 3]
        return [(0, cut), (cut, Lt)]
    out, lo, k = [], 0, 0
    while lo < Lt:
        hi = min(Lt, lo + 1 + (5 * b + 3 * k) % 9)
        out.append((lo, hi))
        lo, k = hi, k + 1
    return out


@functools.lru_cache(maxsize=None)
def enhancer_scale(name):
    """the factor on (text, text_pos) at which make_enhancer(name)'s fp64 scores q . k / sqrt(D) have a standard deviation of 2 (scores
    are quadratic in the inputs; measured once on 256 unscaled tokens)"""
    m = copy.deepcopy(make_enhancer(name)).double()
    C, H = m.self_attn.embed_dim, m.num_heads
    g = torch.Generator().manual_seed(400 + SEEDS[name])
    x = (torch.randn(256, C, generator=g) + 0.5 * torch.randn(256, C, generator=g)).double()
    W, b = m.self_attn.in_proj_weight.detach(), m.self_attn.in_proj_bias.detach()
    q, k = (x @ W[:C].T + b[:C]).reshape(256, H, -1), (x @ W[C:2 * C].T + b[C:2 * C]).reshape(256, H, -1)
    std = (torch.einsum("qhd,khd->hqk", q, k) / (C // H) ** 0.5).std().item()
    return (2.0 / std) ** 0.5


@functools.lru_cache(maxsize=None)
def make_inputs(name, Lt):
    """-> dict of CPU tensors (floating ones bf16, valid_ratios fp32).  Cached: leave it unchanged."""
    c = CONFIGS[name]
    S, L, B, C = tokens(name), len(c["maps"]), c["B"], c["C"]
    g = torch.Generator().manual_seed(200 + SEEDS[name] + Lt)
    vision = torch.randn(B, S, C, generator=g).to(torch.bfloat16)
    vision_pos = (0.5 * torch.randn(B, S, C, generator=g)).to(torch.bfloat16)
    text = torch.randn(B, Lt, C, generator=g).to(torch.bfloat16)
    text_pos = (0.5 * torch.randn(B, Lt, C, generator=g)).to(torch.bfloat16)
    vr = 0.5 + 0.5 * torch.rand(B, L, 2, generator=g)
    vr = vr.clamp(min=0.5 + 2.0 ** -10)
    vr[0, 0, 0] = 1.0
    vr[B - 1, L - 1, 1] = 1.0
    vmask = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        vmask[b, S - int(round(S * (0.12 + 0.08 * b))):] = True
    tmask = torch.zeros(B, Lt, dtype=torch.bool)
    allowed = torch.zeros(B, Lt, Lt, dtype=torch.bool)     # True = may attend
    ids = torch.zeros(B, Lt, dtype=torch.int64)
    for b in range(B):
        for lo, hi in phrases(b, Lt):
            allowed[b, lo:hi, lo:hi] = True
            ids[b, lo:hi] = torch.arange(hi - lo)
        if b > 0 and Lt > 1:     # the last token is padding: it sees itself only and nobody sees it
            tmask[b, Lt - 1] = True
            allowed[b, Lt - 1, :] = False
            allowed[b, :, Lt - 1] = False
            allowed[b, Lt - 1, Lt - 1] = True
    es = enhancer_scale(name)
    return dict(vision=vision, vision_pos=vision_pos, text=text, text_pos=text_pos, valid_ratios=vr,
                enh_text=(es * text.float()).to(torch.bfloat16), enh_pos=(es * text_pos.float()).to(torch.bfloat16),
                spatial_shapes=torch.tensor(c["maps"], dtype=torch.int64), level_start_index=torch.from_numpy(O.level_start_index(c["maps"])),
                vision_mask=vmask, text_mask=tmask, text_self_attention_masks=allowed, text_position_ids=ids)


def to(t, device, dtype=None):
    out = {}
    for k, v in t.items():
        if torch.is_tensor(v):
            v = v.to(device)
            if dtype is not None and v.is_floating_point():
                v = v.to(dtype)
        out[k] = v
    return out


def encoder_call(m, t, vmask=True, tmask=True, pos="ids", **kw):
    """the encoder's forward on make_inputs' tensors; ``pos``: "ids" (text_position_ids), "none" or "embedding" (text_pos)"""
    return m(t["vision"], t["vision_mask"] if vmask else None, t["vision_pos"], t["spatial_shapes"], t["level_start_index"], t["valid_ratios"],
             t["text"], t["text_mask"] if tmask else None, t["text_pos"] if pos == "embedding" else None, t["text_self_attention_masks"],
             t["text_position_ids"] if pos == "ids" else None, **kw)


def enhancer_mask(t, kind, H):
    """the enhancer's ``attention_masks`` (True = may NOT attend): "B" [B, Lt, Lt], different per image; "2d" [Lt, Lt], image 0's;
    "BH" [B H, Lt, Lt], image b's for each of its heads, the second head's with the first key masked too where the row keeps another"""
    m = ~t["text_self_attention_masks"]
    if kind == "B":
        return m
    if kind == "2d":
        return m[0]
    B, Lt, _ = m.shape
    out = m[:, None].repeat(1, H, 1, 1).clone()
    for h in range(1, H):
        keep = (~out[:, h]).sum(-1) > 1           # rows with more than one key left
        out[:, h, :, 0] |= keep
    return out.reshape(B * H, Lt, Lt)


@functools.lru_cache(maxsize=None)
def reference_encoder(name, n_layers, Lt, vmask=True, tmask=True, pos="ids"):
    """-> (vision, text, record): the fp64 module's outputs and, per hooked module name, the tensors that went through it.  Cached."""
    m = copy.deepcopy(make_encoder(name, n_layers)).double()
    t = to(make_inputs(name, Lt), "cpu", torch.float64)
    rec = {}
    hooks = []
    for i, layer in enumerate(m.layers):
        for key, mod in ((f"{i}.enhancer_fc1", layer.text_enhancer_layer.fc1), (f"{i}.deformable_fc1", layer.deformable_layer.fc1)):
            hooks.append(mod.register_forward_hook(lambda mod_, inp, out, key=key: rec.__setitem__(key, out.detach())))
    with torch.no_grad(), cpu_operator():
        v, x = encoder_call(m, t, vmask, tmask, pos, return_dict=False)
    for h in hooks:
        h.remove()
    return v, x, rec


@functools.lru_cache(maxsize=None)
def reference_enhancer(name, Lt, kind, with_pos):
    """-> (out, attention weights, fc1's output) of the fp64 enhancer on enh_text / enh_pos.  Cached."""
    m = copy.deepcopy(make_enhancer(name)).double()
    t = to(make_inputs(name, Lt), "cpu", torch.float64)
    pre = []
    hook = m.fc1.register_forward_hook(lambda mod, inp, out: pre.append(out.detach()))
    with torch.no_grad():
        out, w = m(t["enh_text"], enhancer_mask(t, kind, m.num_heads), t["enh_pos"] if with_pos else None)
    hook.remove()
    return out, w, pre[0]


def rel_rms(x, ref):
    x, ref = x.detach().double().cpu(), ref.detach().double().cpu()
    return ((x - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def quirk_attention(q, k, v, masks, H, by_image):
    """Hand-written attention of nn.MultiheadAttention's core for a [B, Lt, Lt] mask: image b, head h under mask (b H + h) % B (the
    reference's repeat), or under mask b where ``by_image``.  q, k, v [B, Lt, C] already projected; -> the context [B, Lt, C]."""
    B, Lt, C = q.shape
    D = C // H
    out = torch.zeros_like(q)
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            s = (q[b, :, sl] @ k[b, :, sl].T) / D ** 0.5
            s = s.masked_fill(masks[b if by_image else (b * H + h) % B], float("-inf"))
            out[b, :, sl] = torch.softmax(s, -1) @ v[b, :, sl]
    return out
