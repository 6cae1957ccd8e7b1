"""What the native one-call layers (ms_deform_attn.py, deformable_encoder.py, deformable_decoder.py, dcnv3.py) share on the host: the
attention linears' names, the descriptor writer, a call's operands, the layers' module-side conditions and activation tables."""
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

MSDA_LINEARS = tuple(n[:-2] for n in _lib.pointer_fields(_lib.VllmMsdaLayerGrads) if n.endswith("_w"))   # each a <name>_w, <name>_b pair
ACT_RELU, ACT_GELU = 0, _lib.EPI_GELU   # VllmDeformEncLayerDesc.act / VllmDeformDecLayerDesc.act


def get_activation_fn(activation, d_model=256, batch_dim=0):
    """Return an activation function given a string (unipose/utils/model_utils.py:162-175)"""
    if activation == "relu":
        return F.relu
    if activation == "gelu":
        return F.gelu
    if activation == "glu":
        return F.glu
    if activation == "prelu":
        return nn.PReLU()
    if activation == "selu":
        return F.selu
    raise RuntimeError(F"activation should be relu/gelu, not {activation}.")


def act2fn(name):
    """transformers' ACT2FN for the names a Grounding-DINO config uses (the package itself is not required)"""
    table = {"relu": F.relu, "gelu": F.gelu, "silu": F.silu, "swish": F.silu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
             "selu": F.selu}
    if name in table:
        return table[name]
    from transformers.activations import ACT2FN
    return ACT2FN[name]


def native_act(fn):
    return ACT_RELU if fn is F.relu else ACT_GELU if fn is F.gelu else None


def put(struct, keep, name, weight, bias):
    """``struct.<name>_w`` / ``<name>_b`` = pointers to 16-byte aligned weight / bias, appended to ``keep``: hold it until the call is enqueued"""
    w, b = _lib.aligned(weight.detach()), _lib.aligned(bias.detach())
    keep.extend((w, b))
    setattr(struct, name + "_w", w.data_ptr())
    setattr(struct, name + "_b", b.data_ptr())


def msda_params(attn):
    """weight and bias of each of ``attn``'s MSDA_LINEARS, in the descriptor's order"""
    return [p for n in MSDA_LINEARS for p in (getattr(attn, n).weight, getattr(attn, n).bias)]


def fill_msda_desc(desc, keep, C, n_heads, n_levels, n_points, ref_dim, use_4d, params):
    """A VllmMsdaLayerDesc, everything but ``geometry``; ``params`` as msda_params() gives them."""
    desc.d_model, desc.n_heads, desc.n_levels, desc.n_points = C, n_heads, n_levels, n_points
    desc.ref_dim, desc.use_4d_normalizer = ref_dim, int(bool(use_4d))
    for i, name in enumerate(MSDA_LINEARS):
        put(desc, keep, name, params[2 * i], params[2 * i + 1])


def opt_aligned(t):
    return None if t is None else _lib.aligned(t)


def mask_u8(mask, device):
    """a bool mask as the uint8 tensor on ``device`` that the C entries read (None stays None)"""
    return None if mask is None else mask.to(device=device).to(torch.uint8).contiguous()


def memory_operands(who, x, reference_points, memory, spatial_shapes, level_start_index, padding_mask, n_levels, ref_dim=None):
    """The operands of a native call whose activations ``x`` [B, Lq, C] attend to a multi-level ``memory`` [B, S, C] -> (x,
    reference_points, memory, spatial_shapes, level_start_index, padding_mask) as include/vllm_hip.h asks: activations 16-byte aligned (a
    view at another storage offset is copied); reference points fp32, materialised as [B, Lq, n_levels, 2 | 4] and aligned to one point;
    level tensors int64 and the mask [B, S] uint8 on ``x``'s device.  Shapes that do not fit raise RuntimeError, prefixed with ``who``.
    ``ref_dim``: the one last dimension a caller takes; ``reference_points`` None (a caller with its own) skips them."""
    B, Lq, C = x.shape
    S = memory.shape[1]
    r = reference_points
    if r is not None and (r.dim() != 4 or r.shape[0] not in (1, B) or r.shape[1] not in (1, Lq) or r.shape[2] not in (1, n_levels) or
                          (ref_dim is not None and r.shape[3] != ref_dim)):
        raise RuntimeError(f"{who}: reference_points {tuple(r.shape)} does not broadcast to ({B}, {Lq}, {n_levels}, {ref_dim or '2|4'})")
    if tuple(memory.shape) != (B, S, C):
        raise RuntimeError(f"{who}: memory {tuple(memory.shape)} vs activations {tuple(x.shape)}")
    if tuple(spatial_shapes.shape) != (n_levels, 2) or level_start_index.numel() != n_levels:
        raise RuntimeError(f"{who}: spatial_shapes {tuple(spatial_shapes.shape)} / level_start_index "
                           f"({level_start_index.numel()}) do not describe {n_levels} levels")
    if padding_mask is not None and tuple(padding_mask.shape) != (B, S):
        raise RuntimeError(f"{who}: padding mask {tuple(padding_mask.shape)} must be ({B}, {S})")
    xa = _lib.aligned(x)
    mem = xa if memory is x else _lib.aligned(memory)
    if r is not None:
        r = _lib.aligned(r.to(torch.float32).expand(B, Lq, n_levels, r.shape[3]), 16 if r.shape[3] == 4 else 8)
    shapes = spatial_shapes.to(device=xa.device, dtype=torch.int64).contiguous()
    lsi = level_start_index.to(device=xa.device, dtype=torch.int64).contiguous()
    return xa, r, mem, shapes, lsi, mask_u8(padding_mask, xa.device)


def is_gpu_bf16(t, dims=3):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == dims


def msda_layer_fused_ok(query, input_flatten, *linears, reference_points=None):
    """The fused HIP layer serves inference-dtype (bf16) modules on the GPU; anything else keeps the composed path."""
    if not (query.is_cuda and query.dtype == torch.bfloat16 and input_flatten.dtype == torch.bfloat16):
        return False
    if torch.is_grad_enabled():
        # training differentiates through the composed path (autograd Function around the operator): trainable
        # parameters, or a frozen module whose INPUTS carry gradients to upstream layers (the fused call has no grad_fn)
        if any(p.requires_grad for lin in linears for p in lin.parameters()):
            return False
        if query.requires_grad or input_flatten.requires_grad or (reference_points is not None and reference_points.requires_grad):
            return False
    d_model = query.shape[-1]
    return d_model % 64 == 0 and all(lin.weight.dtype == torch.bfloat16 and lin.bias is not None for lin in linears)


def module_reasons(training, mods, dropouts, act, attn, attn_name, query, memory, reference_points, ref_dims, grad_inputs, d_ffn):
    """The module-side reasons why a native encoder / decoder layer call does not serve, as a list of strings (empty: it does).  ``mods``:
    the modules whose parameters must be bf16 on the GPU, with biases, and frozen under grad mode; ``grad_inputs`` may not require grad
    then; ``dropouts``: what training mode would apply; ``act``: native_act(); ``attn``: the deformable attention between ``query`` and
    ``memory`` (3-d tensors); ``ref_dims``: the last dimensions of ``reference_points`` that the call takes."""
    why = []
    params = [p for m in mods for p in m.parameters()]
    if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
        why.append("parameters: bf16 on the GPU")
    if any(getattr(m, "bias", 0) is None for m in mods if not isinstance(m, nn.MultiheadAttention)):
        why.append("parameters: a Linear / LayerNorm without bias")
    if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or any(torch.is_tensor(t) and t.requires_grad for t in grad_inputs)):
        why.append("requires_grad under grad mode: there is no native backward")
    if training and any(p > 0 for p in dropouts):
        why.append("active dropout")
    if act is None:
        why.append("activation: relu or gelu")
    if not torch.is_tensor(reference_points) or reference_points.shape[-1] not in ref_dims:
        why.append("reference_points: last dim " + " or ".join(str(d) for d in ref_dims))
    elif not (is_gpu_bf16(query) and is_gpu_bf16(memory)) or not msda_layer_fused_ok(
            query, memory, *(getattr(attn, n) for n in MSDA_LINEARS), reference_points=reference_points):
        why.append(f"{attn_name}: msda_layer_fused_ok")
    C = query.shape[-1]
    if not (C % 64 == 0 and C <= 512 and d_ffn % 64 == 0 and getattr(attn, "d_model", C) == C):
        why.append("d_model a multiple of 64 up to 512, d_ffn a multiple of 64")
    return why
