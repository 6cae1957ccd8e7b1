"""Modules, inputs and the fp64 yardstick of the Grounding-DINO decoder's tests (test_deform_decoder_cpu.py, test_deform_decoder_gpu.py).

One model: d_model 64 / 2 heads (D 32) / 2 levels [[5, 7], [3, 4]] / 2 points / d_ffn 128 / P = 32 sine features per coordinate / 3 layers,
B 2, Lt 5 and Lq 37 or 70 (70 crosses one 64-row attention block).  ``bbox_embed`` is None, one head shared by every layer
(``decoder_bbox_embed_share``) or one head per layer.  As in deform_decoder_layer_inputs every parameter is the module's own initial value
plus 0.2 randn rounded to bf16, so that the fp64 module and the bf16 module hold the same numbers; masks are that module's denoising mask
and tail masks; ``valid_ratios`` lie in (0.5, 1] and differ per image and per level.

The yardstick (``reference``) is the mirror's own composed ``forward`` on a ``.double()`` CPU copy, the operator replaced by the
pure-PyTorch twin (deform_decoder_layer_inputs.cpu_operator).  It never calls the native library.  Nothing here touches torch.cuda at
import."""
import copy
import functools
import types

import torch

from oracle import msda as O
from visionllm_amd import deformable_decoder as D

import deform_decoder_layer_inputs as LI

C, HEADS, MAPS, POINTS, FFN, NPOS, LAYERS = 64, 2, [(5, 7), (3, 4)], 2, 128, 32, 3
B, LT, LQS = 2, 5, (37, 70)
S = sum(h * w for h, w in MAPS)
BOXES = (None, "shared", "per_layer")
# (Lq, with masks, box heads)
CASES = [(lq, m, b) for lq in LQS for m in (True, False) for b in BOXES]
IDS = [f"Lq{lq}-{'masks' if m else 'nomasks'}-box_{b}" for lq, m, b in CASES]


def config(**kw):
    c = dict(d_model=C, num_feature_levels=len(MAPS), decoder_attention_heads=HEADS, decoder_n_points=POINTS, decoder_ffn_dim=FFN,
             dropout=0.1, attention_dropout=0.1, activation_function="relu", activation_dropout=0.1, disable_custom_kernels=False,
             decoder_layers=LAYERS, query_dim=4, output_attentions=False, output_hidden_states=False, use_return_dict=False)
    c.update(kw)
    return types.SimpleNamespace(**c)


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((p + 0.2 * torch.randn(p.shape, generator=g)).to(torch.bfloat16).float())


def make_decoder(box=None, **cfg):
    """-> the decoder in fp32 (eval mode) whose parameters are bf16 values; ``box``: None, "shared" (an nn.ModuleList holding ONE head
    object in every slot, as decoder_bbox_embed_share leaves it) or "per_layer" (an nn.ModuleList of three heads)"""
    torch.manual_seed(31)
    m = D.GroundingDinoDecoder(config(**cfg))
    _perturb(m, 131)
    if box is not None:
        torch.manual_seed(32)
        heads = [D.GroundingDinoMLPPredictionHead(C, C, 4, 3) for _ in range(1 if box == "shared" else LAYERS)]
        for i, h in enumerate(heads):
            _perturb(h, 132 + i)
            with torch.no_grad():   # deltas of a few tenths of a logit, as a trained head gives: the boxes stay inside the image
                for p in h.layers[-1].parameters():
                    p.copy_((0.02 * p).to(torch.bfloat16).float())
        m.bbox_embed = torch.nn.ModuleList(heads if box == "per_layer" else [heads[0]] * LAYERS)
    return m.eval()


def as_bf16(m, device):
    return copy.deepcopy(m).to(device).to(torch.bfloat16).eval()


@functools.lru_cache(maxsize=None)
def make_inputs(Lq, with_masks=True):
    """-> dict of CPU tensors: tgt [B, Lq, C], memory [B, S, C], memory_text [B, Lt, C] (bf16), reference_points [B, Lq, 4] and
    valid_ratios [B, L, 2] (fp32), spatial_shapes, level_start_index (int64) and the three masks or None: self_attn_mask (bool [Lq, Lq],
    True = may not attend), text_mask (bool [B, Lt], True = ignore), attention_mask (bool [B, S], True = REAL, the decoder's convention).
    Cached: leave it unchanged."""
    g = torch.Generator().manual_seed(300 + Lq)
    tgt = torch.randn(B, Lq, C, generator=g).to(torch.bfloat16)
    memory = torch.randn(B, S, C, generator=g).to(torch.bfloat16)
    text = torch.randn(B, LT, C, generator=g).to(torch.bfloat16)
    ref = torch.cat([torch.rand(B, Lq, 2, generator=g), 0.1 + 0.3 * torch.rand(B, Lq, 2, generator=g)], -1)
    vr = 1.0 - 0.5 * torch.rand(B, len(MAPS), 2, generator=g)   # (0.5, 1]
    assert vr.min() > 0.5 and vr.max() <= 1.0 and len(set(vr.flatten().tolist())) == vr.numel()
    return dict(tgt=tgt, memory=memory, memory_text=text, reference_points=ref, valid_ratios=vr,
                spatial_shapes=torch.tensor(MAPS, dtype=torch.int64), level_start_index=torch.from_numpy(O.level_start_index(MAPS)),
                self_attn_mask=LI.denoise_mask(Lq) if with_masks else None, text_mask=LI.tail_mask(B, LT) if with_masks else None,
                attention_mask=~LI.tail_mask(B, S) if with_masks else None)


def to(t, device, dtype=None):
    return LI.to(t, device, dtype)


def args(t):
    """positional and keyword arguments of GroundingDinoDecoder.forward for a dict of make_inputs' tensors"""
    return (t["tgt"], t["memory"], None), dict(
        vision_encoder_attention_mask=t["attention_mask"], text_encoder_hidden_states=t["memory_text"],
        text_encoder_attention_mask=t["text_mask"], reference_points=t["reference_points"], spatial_shapes=t["spatial_shapes"],
        level_start_index=t["level_start_index"], valid_ratios=t["valid_ratios"], self_attn_mask=t["self_attn_mask"])


def call(m, t, **kw):
    """the decoder's forward -> what it returns (the tuple form unless ``return_dict`` says otherwise)"""
    a, k = args(t)
    return m(*a, **k, **kw)


def reasons(m, t, **kw):
    a, k = args(t)
    return m.native_decoder_reasons(a[0], a[1], **k, **kw)


@functools.lru_cache(maxsize=None)
def reference(Lq, with_masks=True, box=None):
    """-> (intermediate [B, n_layers, Lq, C], intermediate_reference_points [B, n_layers, Lq, 4]) of the fp64 module on the case's
    bf16-valued inputs.  Computed once per case on the CPU; leave it unchanged."""
    m = copy.deepcopy(make_decoder(box)).double()
    t = to(make_inputs(Lq, with_masks), "cpu", torch.float64)
    with torch.no_grad(), LI.cpu_operator():
        out = call(m, t)
    return out[1].contiguous(), out[2].contiguous()
