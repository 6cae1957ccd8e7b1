"""Inputs, yardstick and bounds of the deformable-attention layer's training tests (test_msda_layer_train_cpu.py,
test_msda_layer_train_gpu.py).

A torch RESTATEMENT of the reference's statements (MSDeformAttn.forward, unipose/ops/modules/ms_deform_attn.py:83-145): value_proj,
``masked_fill`` of the padded keys, the sampling_offsets / attention_weights linears, softmax over L * P, the product's own
``_sampling_locations`` (the three reference-point forms, statement for statement the reference's), the operator as the reference's
pure-PyTorch twin (``oracle.msda.grid_sample_twin``) and output_proj -- written for any floating dtype, so that the same statements give
  * the truth: torch fp64 autograd on the bf16-valued parameters, inputs and grad_out, and
  * the comparator: what a bf16 module runs -- bf16 linears, softmax and location arithmetic, the fp32 upcast around the operator
    (ms_deform_attn.py:131-139), bf16 autograd (DESIGN section 5's assembled-bf16 rule: native within 1.25 x the comparator's distance).
Both run on the CPU and never call the code under test.  test_msda_layer_train_cpu.py ties the truth's forward to
``oracle.msda.layer_forward`` on tests/golden/msda_layer.npz (the reference modules' own run).

The prep-backward kernel alone has a closed form (``prep_backward_ref``, fp64):
    d_logit  = w (g_w - sum_{L P} g_w w)                     per (row, head): the softmax's backward
    d_offset = g_loc (sx, sy)                                (sx, sy) the scale of location = ref + offset (sx, sy)
and the project's per-element bound |err| <= 1 bf16 ulp(ref) + 2^-17 mag with mag the magnitude of the terms:
    d_logit: w (|g_w| + sum |g_w| w);  d_offset: |g_loc| (sx, sy).
Nothing here touches torch.cuda at import."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from bounds import rel_rms  # noqa: F401  (re-exported)
from oracle import msda as O
from visionllm_amd.ms_deform_attn import _sampling_locations

LINEARS = ("value_proj", "sampling_offsets", "attention_weights", "output_proj")
PARAM_NAMES = tuple(f"{n}.{k}" for n in LINEARS for k in ("weight", "bias"))
ENCODER_MAPS = [(72, 64), (36, 32), (18, 16), (9, 8)]
DECODER_MAPS = [(96, 96), (48, 48), (24, 24), (12, 12)]       # the maps of test_fused_layer_decoder_shape_bf16_value
# name -> maps, Lq (None: the cells of the maps), heads, d_model, points, ref_dim, 4D normalizer, masked
CASES = {
    "a_L3_generic_pad320": dict(maps=[(12, 16), (6, 8), (3, 4)], Lq=50, M=8, C=256, P=4, ref_dim=4, four_d=False, masked=True),
    "b_4d_normalizer_pad128": dict(maps=[(12, 16), (6, 8)], Lq=64, M=4, C=128, P=4, ref_dim=4, four_d=True, masked=True),
    "c_encoder": dict(maps=ENCODER_MAPS, Lq=None, M=8, C=256, P=4, ref_dim=2, four_d=False, masked=True),
    "d_decoder_bf16_value": dict(maps=DECODER_MAPS, Lq=900, M=8, C=256, P=4, ref_dim=2, four_d=False, masked=True),
    "e_P8": dict(maps=[(12, 16), (6, 8), (3, 4), (2, 2)], Lq=50, M=8, C=256, P=8, ref_dim=4, four_d=False, masked=False),
}
B = 2
MARGIN = 1.25          # the assembled-bf16 margin of test_clip_layer_train_gpu.py / test_vit_layer_train_gpu.py


def npad(M, L, P):
    return (3 * M * L * P + 63) // 64 * 64


# ---- the reference's statements -------------------------------------------------------------------------------------------------------
def layer(p, query, reference_points, input_flatten, spatial_shapes, padding_mask, n_heads, n_points, four_d, op_dtype=None):
    """MSDeformAttn.forward on a {PARAM_NAMES: tensor} dict; ``op_dtype``: the dtype of the upcast around the operator (None: none)"""
    N, Len_q, C = query.shape
    Len_in = input_flatten.shape[1]
    L = spatial_shapes.shape[0]
    value = F.linear(input_flatten, p["value_proj.weight"], p["value_proj.bias"])
    if padding_mask is not None:
        value = value.masked_fill(padding_mask[..., None], float(0))
    value = value.view(N, Len_in, n_heads, C // n_heads)
    sampling_offsets = F.linear(query, p["sampling_offsets.weight"], p["sampling_offsets.bias"]).view(N, Len_q, n_heads, L, n_points, 2)
    attention_weights = F.linear(query, p["attention_weights.weight"], p["attention_weights.bias"]).view(N, Len_q, n_heads, L * n_points)
    attention_weights = F.softmax(attention_weights, -1).view(N, Len_q, n_heads, L, n_points)
    sampling_locations = _sampling_locations(reference_points, sampling_offsets, spatial_shapes, n_points, four_d)
    if op_dtype is not None:
        output = O.grid_sample_twin(value.to(op_dtype), spatial_shapes.tolist(), sampling_locations.to(op_dtype),
                                    attention_weights.to(op_dtype)).to(value.dtype)
    else:
        output = O.grid_sample_twin(value, spatial_shapes.tolist(), sampling_locations, attention_weights)
    return F.linear(output, p["output_proj.weight"], p["output_proj.bias"])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_params(C, M, L, P, seed=0):
    """-> {PARAM_NAMES: bf16 tensor}.  No gradient tensor degenerate: every weight randn-scaled (the modules' zero init of the two query
    linears would make the offsets and logits independent of the query), logits spread enough that the softmax is not flat."""
    g = torch.Generator().manual_seed(4000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    MLP = M * L * P
    p = {"value_proj.weight": rn(C, C) / math.sqrt(C), "value_proj.bias": 0.1 * rn(C),
         "sampling_offsets.weight": rn(2 * MLP, C) * (0.5 / math.sqrt(C)), "sampling_offsets.bias": rn(2 * MLP),
         "attention_weights.weight": rn(MLP, C) / math.sqrt(C), "attention_weights.bias": 0.5 * rn(MLP),
         "output_proj.weight": rn(C, C) / math.sqrt(C), "output_proj.bias": 0.1 * rn(C)}
    return {k: v.to(torch.bfloat16) for k, v in p.items()}


def make_reference_points(rows_shape, L, ref_dim, g):
    ref = torch.rand(*rows_shape, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = ref[..., 2:] * 0.3 + 0.05
    return ref


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict of CPU tensors: params (bf16), query, input_flatten, grad_out (bf16), reference_points (fp32), spatial_shapes,
    level_start_index (int64), padding_mask (bool or None: the last image's tail is padded) and the sizes.  Cached: leave it unchanged."""
    c = CASES[name]
    maps, M, C, P = c["maps"], c["M"], c["C"], c["P"]
    L = len(maps)
    S = sum(h * w for h, w in maps)
    Lq = S if c["Lq"] is None else c["Lq"]
    g = torch.Generator().manual_seed(5000 + sorted(CASES).index(name))
    bf = lambda t: t.to(torch.bfloat16)
    query = bf(torch.randn(B, Lq, C, generator=g))
    src = bf(torch.randn(B, S, C, generator=g))
    grad_out = bf(torch.randn(B, Lq, C, generator=g) / math.sqrt(C))
    ref = make_reference_points((B, Lq), L, c["ref_dim"], g)
    mask = None
    if c["masked"]:
        mask = torch.zeros(B, S, dtype=torch.bool)
        mask[-1, -(S // 7):] = True
    return dict(name=name, params=make_params(C, M, L, P, seed=sorted(CASES).index(name)), query=query, input_flatten=src, grad_out=grad_out,
                reference_points=ref, spatial_shapes=torch.tensor(maps, dtype=torch.int64),
                level_start_index=torch.from_numpy(O.level_start_index(maps)), padding_mask=mask, M=M, C=C, P=P, L=L, S=S, Lq=Lq,
                four_d=c["four_d"], ref_dim=c["ref_dim"])


def autograd_layer(case, dtype, op_dtype=None):
    """torch autograd of ``layer`` in ``dtype`` on copies of the case's bf16 values -> (out, {query, input_flatten, PARAM_NAMES: grad})"""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in case["params"].items()}
    q = case["query"].detach().to(dtype).requires_grad_(True)
    x = case["input_flatten"].detach().to(dtype).requires_grad_(True)
    out = layer(p, q, case["reference_points"].to(dtype), x, case["spatial_shapes"], case["padding_mask"], case["M"], case["P"],
                case["four_d"], op_dtype)
    out.backward(case["grad_out"].to(dtype))
    grads = {k: v.grad for k, v in p.items()}
    grads.update(query=q.grad, input_flatten=x.grad)
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def truth(name):
    """fp64 autograd of the reference's statements on the bf16-valued inputs (computed once per case; leave it unchanged)"""
    return autograd_layer(make_case(name), torch.float64)


@functools.lru_cache(maxsize=None)
def comparator(name):
    """the same statements as a bf16 module runs them: bf16 everywhere, fp32 around the operator, bf16 autograd"""
    return autograd_layer(make_case(name), torch.bfloat16, op_dtype=torch.float32)


# ---- the prep-backward kernel's closed form ---------------------------------------------------------------------------------------------
def offset_scale(reference_points, spatial_shapes, P, four_d):
    """(sx, sy) [R, L, 2] of location = ref + offset * (sx, sy), in the dtype of reference_points [R, L, 2|4]"""
    ref = reference_points
    wh = torch.stack([spatial_shapes[:, 1], spatial_shapes[:, 0]], -1).to(ref.dtype)
    if ref.shape[-1] == 2:
        return (1.0 / wh)[None].expand(ref.shape[0], -1, -1)
    if four_d:
        return ref[..., 2:] * 0.5 / wh[None]
    return ref[..., 2:] * 0.5 / P


def prep_backward_ref(grad_loc, grad_w, w, reference_points, spatial_shapes, P, four_d):
    """fp64: grad_loc [R, M, L, P, 2], grad_w / w [R, M, L * P], reference_points [R, L, 2|4] -> d_offset, d_logit and their magnitudes"""
    gl, gw, w = grad_loc.double(), grad_w.double(), w.double()
    s = offset_scale(reference_points.double(), spatial_shapes, P, four_d)[:, None, :, None, :]
    d_off = gl * s
    d_logit = w * (gw - (gw * w).sum(-1, keepdim=True))
    mag_logit = w.abs() * (gw.abs() + (gw * w).abs().sum(-1, keepdim=True))
    return d_off, d_logit, d_off.abs(), mag_logit


def prep_case(R, M, L, P, ref_dim, seed=0):
    """-> grad_loc, grad_w (fp32), w (fp32 softmax weights), reference_points [R, L, ref_dim], spatial_shapes [L, 2]"""
    g = torch.Generator().manual_seed(6000 + seed + 131 * R + 17 * L + P)
    gl = torch.randn(R, M, L, P, 2, generator=g) * 3
    gw = torch.randn(R, M, L * P, generator=g) * 2
    w = torch.softmax(torch.randn(R, M, L * P, generator=g) * 2, -1)
    ref = make_reference_points((R,), L, ref_dim, g)
    shapes = torch.tensor([(7 + 3 * l, 5 + 2 * l) for l in range(L)], dtype=torch.int64)
    return gl, gw, w, ref, shapes


def bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even, in integer arithmetic (NaN kept a NaN): the narrowing kernel's exact answer"""
    u = x.detach().cpu().contiguous().view(torch.int32).numpy().astype(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return torch.from_numpy(r.astype(np.int16))
