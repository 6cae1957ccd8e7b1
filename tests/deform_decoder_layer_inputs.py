"""Modules, inputs and the fp64 yardstick of the deformable decoder layer's tests (test_deform_decoder_layer_cpu.py,
test_deform_decoder_layer_gpu.py).

Three shapes for both flavours (``unipose``: DeformableTransformerDecoderLayer, ``gdino``: GroundingDinoDecoderLayer):
    small   d_model  64 / 2 heads (D 32) / 2 levels [[6, 5], [3, 2]]                    / 4 points / d_ffn 128 / B 2 / Lq  37 / Lt 5 / relu
    tile    d_model 256 / 8 heads (D 32) / 4 levels [[12, 10], [6, 5], [3, 3], [2, 1]] / 4 points / d_ffn 512 / B 2 / Lq 130 / Lt 9 / relu
    wide    d_model 256 / 4 heads (D 64) / 3 levels [[8, 7], [4, 4], [2, 2]]            / 4 points / d_ffn 192 / B 1 / Lq  70 / Lt 3 / gelu
each with 2-d and 4-d reference points, with and without ``query_pos`` and with and without the three masks; UniPose additionally with
``use_4D_normalizer``, without the text attention and after ``rm_self_attn_modules()`` (``VARIANTS``).  Every parameter is the module's
own initial value plus 0.2 randn, rounded to bf16, so that the fp64 module and the bf16 module hold the same numbers.  Tensors are kept
batch-first here; ``call`` hands the UniPose layer its sequence-first views.

The yardstick (``reference``) is the module itself in fp64 on the CPU, with the one statement that has no CPU form -- the operator
behind ``_msda_apply_fp32`` -- replaced by the reference's pure-PyTorch twin (``oracle.msda.grid_sample_twin``).  It never calls the
native library.

The attention kernel's own cases (``MHA_*``, ``mha_inputs``, ``mha_masks``, ``mha_reference``) are here too.  Mask patterns:
    denoise     a denoising-style block mask (Lq == Lk): 40 % of the rows are two denoising groups that see only themselves, the matching
                rows behind them see no denoising row
    first_tile  the rows of the first half (rounded up) are hidden from the WHOLE first key tile (keys 0 .. 63); Lk > 64
    full_row    a random mask of density 0.3 with one row whose every key is masked
    kpm         a key-padding mask over the tail of image b: ceil((15 % + 10 % b) Lk) keys
``mha_conditions`` is the fact every masked case must show on the fp64 run: the share of (row, key) pairs that are masked, 20-80 % for
every case with an attention mask and for the key-padding mask alone at B = 2 (at B = 1 it pads 15 %, as the pattern is defined; a
single key is never padded, so (1, 1) has no masked case).
Nothing here touches torch.cuda at import."""
import contextlib
import copy
import functools
import itertools
import math
import types

import torch

from oracle import msda as O
from visionllm_amd import deformable_decoder as D
from visionllm_amd import ms_deform_attn as A

SHAPES = {
    "small": dict(C=64, M=2, maps=[(6, 5), (3, 2)], P=4, F=128, B=2, Lq=37, Lt=5, act="relu"),
    "tile": dict(C=256, M=8, maps=[(12, 10), (6, 5), (3, 3), (2, 1)], P=4, F=512, B=2, Lq=130, Lt=9, act="relu"),
    "wide": dict(C=256, M=4, maps=[(8, 7), (4, 4), (2, 2)], P=4, F=192, B=1, Lq=70, Lt=3, act="gelu"),
}
SEEDS = {"small": 21, "tile": 22, "wide": 23}
FLAVOURS = ("unipose", "gdino")
# (shape, ref_dim, with pos, with masks)
CASES = list(itertools.product(SHAPES, (2, 4), (True, False), (True, False)))
IDS = [f"{s}-ref{r}-{'pos' if p else 'nopos'}-{'masks' if m else 'nomasks'}" for s, r, p, m in CASES]
# UniPose only: keyword arguments of make_layer
VARIANTS = {"4d_normalizer": dict(use_4d=True), "no_text": dict(text=False), "no_self_attn": dict(rm_sa=True),
            "cross_attn_only": dict(text=False, rm_sa=True)}


def tokens(shape):
    return sum(h * w for h, w in SHAPES[shape]["maps"])


def make_layer(flavour, shape, activation=None, dropout=0.1, text=True, rm_sa=False, use_4d=False, heads=None):
    """-> the flavour's module in fp32 (eval mode) whose parameters are bf16 values: initial value + 0.2 randn"""
    c = SHAPES[shape]
    act = activation or c["act"]
    M = heads or c["M"]
    torch.manual_seed(SEEDS[shape])
    if flavour == "unipose":
        m = D.DeformableTransformerDecoderLayer(d_model=c["C"], d_ffn=c["F"], dropout=dropout, activation=act, n_levels=len(c["maps"]),
                                                n_heads=M, n_points=c["P"], use_text_cross_attention=text)
        m.cross_attn.use_4D_normalizer = use_4d
    else:
        assert text and not rm_sa and not use_4d
        cfg = types.SimpleNamespace(d_model=c["C"], num_feature_levels=len(c["maps"]), decoder_attention_heads=M,
                                    decoder_n_points=c["P"], decoder_ffn_dim=c["F"], dropout=dropout, attention_dropout=dropout,
                                    activation_function=act, activation_dropout=dropout, disable_custom_kernels=False)
        m = D.GroundingDinoDecoderLayer(cfg)
    g = torch.Generator().manual_seed(100 + SEEDS[shape])
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((p + 0.2 * torch.randn(p.shape, generator=g)).to(torch.bfloat16).float())
    if rm_sa:
        m.rm_self_attn_modules()
    return m.eval()


def as_bf16(m, device):
    return copy.deepcopy(m).to(device).to(torch.bfloat16).eval()


def denoise_mask(Lq):
    """bool [Lq, Lq], True = may NOT attend: rows [0, dn) are two denoising groups, rows [dn, Lq) the matching queries"""
    dn = int(Lq * 0.4)
    half = dn // 2
    m = torch.zeros(Lq, Lq, dtype=torch.bool)
    m[dn:, :dn] = True
    m[:half, half:dn] = True
    m[half:dn, :half] = True
    return m


def tail_mask(B, L):
    """bool [B, L], True = padded: the last ceil((15 % + 10 % b) L) positions of image b"""
    m = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        n = min(L - 1, math.ceil(L * (0.15 + 0.10 * b) - 1e-9))
        if n > 0:
            m[b, L - n:] = True
    return m


@functools.lru_cache(maxsize=None)
def make_inputs(shape, ref_dim=2, with_pos=True, with_masks=True):
    """-> dict of CPU tensors, batch-first: tgt, pos (bf16 [B, Lq, C] or None), reference_points (fp32 [B, Lq, L, ref_dim]), memory
    [B, S, C], memory_text [B, Lt, C], spatial_shapes, level_start_index (int64) and the three masks or None: self_attn_mask (bool
    [Lq, Lq], denoise_mask), text_mask (bool [B, Lt], True = ignore) and padding_mask (bool [B, S], True = padded), both tail_mask.
    Cached: leave it unchanged."""
    c = SHAPES[shape]
    S, L, B, Lq, Lt, C = tokens(shape), len(c["maps"]), c["B"], c["Lq"], c["Lt"], c["C"]
    g = torch.Generator().manual_seed(200 + SEEDS[shape])
    tgt = torch.randn(B, Lq, C, generator=g).to(torch.bfloat16)
    pos = (0.5 * torch.randn(B, Lq, C, generator=g)).to(torch.bfloat16)
    memory = torch.randn(B, S, C, generator=g).to(torch.bfloat16)
    text = torch.randn(B, Lt, C, generator=g).to(torch.bfloat16)
    ref = torch.rand(B, Lq, L, 2, generator=g)
    if ref_dim == 4:
        ref = torch.cat([ref, 0.1 + 0.3 * torch.rand(B, Lq, L, 2, generator=g)], -1)
    return dict(tgt=tgt, pos=pos if with_pos else None, reference_points=ref, memory=memory, memory_text=text,
                spatial_shapes=torch.tensor(c["maps"], dtype=torch.int64), level_start_index=torch.from_numpy(O.level_start_index(c["maps"])),
                self_attn_mask=denoise_mask(Lq) if with_masks else None, text_mask=tail_mask(B, Lt) if with_masks else None,
                padding_mask=tail_mask(B, S) if with_masks else None)


def call(flavour, layer, t, **kw):
    """the flavour's own forward on a dict of make_inputs' tensors (any device / dtype) -> the output tensor, batch-first"""
    if flavour == "unipose":
        tr = lambda x: None if x is None else x.transpose(0, 1)
        return layer(tr(t["tgt"]), tr(t["pos"]), None, None, tr(t["reference_points"]), t["memory_text"], t["text_mask"], tr(t["memory"]),
                     t["padding_mask"], t["level_start_index"], t["spatial_shapes"], None, t["self_attn_mask"], None, **kw).transpose(0, 1)
    attention_mask = None if t["padding_mask"] is None else ~t["padding_mask"]
    out = layer(t["tgt"], t["pos"], t["reference_points"], t["spatial_shapes"], t["level_start_index"], t["memory"], attention_mask,
                t["memory_text"], t["text_mask"], t["self_attn_mask"], **kw)
    return out if kw else out[0]


def applies(flavour, layer, t, **kw):
    """the flavour's native_layer_reasons on make_inputs' tensors -> list of reasons"""
    if flavour == "unipose":
        tr = lambda x: None if x is None else x.transpose(0, 1)
        return layer.native_layer_reasons(tr(t["tgt"]), tr(t["pos"]), tr(t["reference_points"]), t["memory_text"], t["text_mask"],
                                          tr(t["memory"]), t["self_attn_mask"], **kw)
    return layer.native_layer_reasons(t["tgt"], t["pos"], t["reference_points"], t["memory"], t["memory_text"], t["text_mask"],
                                      t["self_attn_mask"], **kw)


def to(t, device, dtype=None):
    """make_inputs' dict on ``device``; floating tensors in ``dtype`` where given"""
    out = {}
    for k, v in t.items():
        if v is not None:
            v = v.to(device)
            if dtype is not None and v.is_floating_point():
                v = v.to(dtype)
        out[k] = v
    return out


@contextlib.contextmanager
def cpu_operator():
    """the operator behind the attention modules as the reference's pure-PyTorch twin, in the dtype it is given"""
    saved = A._msda_apply_fp32
    A._msda_apply_fp32 = lambda value, shapes, lsi, loc, aw, step: O.grid_sample_twin(value, shapes.tolist(), loc.to(value.dtype),
                                                                                       aw.to(value.dtype))
    try:
        yield
    finally:
        A._msda_apply_fp32 = saved


@functools.lru_cache(maxsize=None)
def reference(flavour, shape, ref_dim=2, with_pos=True, with_masks=True, variant=None):
    """-> the fp64 module's output [B, Lq, C] on the case's bf16-valued inputs.  Computed once per case on the CPU; leave it unchanged."""
    m = copy.deepcopy(make_layer(flavour, shape, **(VARIANTS[variant] if variant else {}))).double()
    t = to(make_inputs(shape, ref_dim, with_pos, with_masks), "cpu", torch.float64)
    with torch.no_grad(), cpu_operator():
        return call(flavour, m, t).contiguous()


# ---- the attention kernel alone ---------------------------------------------------------------------------------------------------------------
MHA_D = (32, 64)
# the issue's five, and (130, 132): Lk a multiple of 4 with three query blocks, so the [Lq, Lk] mask is read as 4-byte words (the path
# 900 and 1100 keys take) by every wave of several blocks, tail block included
MHA_L = ((1, 1), (37, 5), (64, 65), (130, 130), (3, 200), (130, 132))
MHA_H = (1, 3)
MHA_B = (1, 2)
MHA_PATTERNS = ("denoise", "first_tile", "full_row")


def mha_patterns(Lq, Lk):
    """the attention-mask patterns this (Lq, Lk) can carry"""
    out = []
    if Lq == Lk and Lq >= 10:
        out.append("denoise")
    if Lk > 64:
        out.append("first_tile")
    if Lk >= 5 and Lq >= 3:
        out.append("full_row")
    return out


@functools.lru_cache(maxsize=None)
def mha_inputs(D_, Lq, Lk, H, B):
    """-> (q [B, Lq, H D], k, v [B, Lk, H D]) bf16 CPU tensors.  Cached: leave them unchanged."""
    g = torch.Generator().manual_seed(D_ * 7 + Lq * 131 + Lk * 17 + H * 3 + B)
    q = torch.randn(B, Lq, H * D_, generator=g).to(torch.bfloat16)
    k = torch.randn(B, Lk, H * D_, generator=g).to(torch.bfloat16)
    v = torch.randn(B, Lk, H * D_, generator=g).to(torch.bfloat16)
    return q, k, v


@functools.lru_cache(maxsize=None)
def mha_masks(pattern, kpm, Lq, Lk, B):
    """-> (attn_mask bool [Lq, Lk] or None, key_padding_mask bool [B, Lk] or None, the row with every key masked or None)"""
    am, dead_row = None, None
    if pattern == "denoise":
        am = denoise_mask(Lq)
    elif pattern == "first_tile":
        am = torch.zeros(Lq, Lk, dtype=torch.bool)
        am[:(Lq + 1) // 2, :64] = True
    elif pattern == "full_row":
        g = torch.Generator().manual_seed(Lq * 1000 + Lk)
        am = torch.rand(Lq, Lk, generator=g) < 0.3
        am[:, Lk // 2] = False          # every other row keeps a key, whatever the padding mask hides (the tail: less than half)
        dead_row = Lq // 3
        am[dead_row] = True
    else:
        assert pattern is None
    return am, (tail_mask(B, Lk) if kpm else None), dead_row


def mha_masked_pairs(am, kp, B, Lq, Lk):
    """bool [B, Lq, Lk]: the (row, key) pairs that are masked"""
    m = torch.zeros(B, Lq, Lk, dtype=torch.bool)
    if am is not None:
        m |= am[None]
    if kp is not None:
        m |= kp[:, None, :]
    return m


@functools.lru_cache(maxsize=None)
def mha_reference(D_, Lq, Lk, H, B, pattern, kpm):
    """-> (out [B, Lq, H, D] fp64 with NaN rows where every key is masked, mag = sum_j p_j |v_j|, share of masked pairs) on the CPU"""
    q, k, v = (x.double().reshape(B, -1, H, D_).transpose(1, 2) for x in mha_inputs(D_, Lq, Lk, H, B))
    am, kp, _ = mha_masks(pattern, kpm, Lq, Lk, B)
    masked = mha_masked_pairs(am, kp, B, Lq, Lk)
    s = (q @ k.transpose(-2, -1)) * D_ ** -0.5
    s = s.masked_fill(masked[:, None], float("-inf"))
    p = torch.softmax(s, -1)          # an all -inf row: NaN, as in nn.MultiheadAttention
    out = (p @ v).transpose(1, 2)
    mag = (p @ v.abs()).transpose(1, 2)
    return out, mag, masked.float().mean().item()


def mha_conditions(D_, Lq, Lk, H, B, pattern, kpm):
    """-> share of (row, key) pairs masked on the fp64 run"""
    return mha_reference(D_, Lq, Lk, H, B, pattern, kpm)[2]
