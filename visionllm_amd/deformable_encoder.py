"""The deformable ENCODER layers of the detection and pose heads: module mirrors and the one-call native forward.

Same constructor arguments, parameter names and ``forward`` signatures as

* ``DeformableTransformerEncoderLayer`` -- visionllmv2/model/unipose/modeling_unipose.py:3132-3186;
* ``GroundingDinoDeformableLayer``      -- visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1105-1180,

with ``self_attn`` this package's ``MSDeformAttn`` / ``GroundingDinoMultiscaleDeformableAttention``.  With the class attribute
``native_layer = False`` (the default) ``forward`` is the reference's statements, line for line, around that attention module.  With
``native_layer = True`` the inference forward of a bf16 module is ONE native call (``vllm_deform_enc_layer_forward``,
csrc/deform_encoder_layer.hip; conditions: ``native_layer_applies``); every other call runs the composed statements unchanged.
``encoder_layers_forward`` chains layers so that each hands the next one its query (``out + pos``) from its last kernel.

Channel attention (``add_channel_attention``) and deformable box attention (``use_deformable_box_attn``) of the UniPose layer are
not mirrored: the constructor raises ``NotImplementedError`` for them.
"""
import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .ms_deform_attn import (GroundingDinoMultiscaleDeformableAttention, MSDeformAttn, known_geometry, level_pixels,
                             msda_layer_fused_ok)

_ATTN_LINEARS = ("value_proj", "sampling_offsets", "attention_weights", "output_proj")
ACT_RELU, ACT_GELU = 0, _lib.EPI_GELU   # VllmDeformEncLayerDesc.act


def _get_activation_fn(activation, d_model=256, batch_dim=0):
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


def _act2fn(name):
    """transformers' ACT2FN for the names a Grounding-DINO config uses (the package itself is not required)"""
    table = {"relu": F.relu, "gelu": F.gelu, "silu": F.silu, "swish": F.silu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
             "selu": F.selu}
    if name in table:
        return table[name]
    from transformers.activations import ACT2FN
    return ACT2FN[name]


def _native_act(fn):
    return ACT_RELU if fn is F.relu else ACT_GELU if fn is F.gelu else None


def _applies(layer, attn, norms, linears, act, dropouts, src, pos, reference_points, query_in=None):
    """The conditions of the native call that both flavours share (see the classes' ``native_layer_applies``)."""
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == torch.bfloat16 and src.dim() == 3):
        return False
    if layer.training and any(p > 0 for p in dropouts):
        return False
    if act is None or reference_points is None or reference_points.shape[-1] != 2:
        return False
    for t in (pos, query_in):
        if t is not None and not (t.is_cuda and t.dtype == torch.bfloat16 and t.shape == src.shape):
            return False
    mods = tuple(norms) + tuple(linears)
    if any(p.dtype != torch.bfloat16 or not p.is_cuda for m in mods for p in m.parameters()) or any(m.bias is None for m in mods):
        return False
    if torch.is_grad_enabled() and (any(p.requires_grad for m in mods for p in m.parameters()) or src.requires_grad or
                                    (pos is not None and pos.requires_grad) or (query_in is not None and query_in.requires_grad)):
        return False
    if not msda_layer_fused_ok(src, src, *(getattr(attn, n) for n in _ATTN_LINEARS), reference_points=reference_points):
        return False
    d_model, d_ffn = src.shape[-1], linears[0].out_features
    return d_model % 64 == 0 and d_model <= 512 and d_ffn % 64 == 0 and getattr(attn, "d_model", d_model) == d_model


def deform_enc_layer_forward(attn, norm1, linear1, act, linear2, norm2, src, pos, reference_points, spatial_shapes, level_start_index,
                             padding_mask=None, query_in=None, want_query_out=False):
    """One ``vllm_deform_enc_layer_forward`` call -> (out, query_out or None).  ``src`` [B, S, C] bf16 on the GPU, ``pos`` the same or
    None, ``reference_points`` [B, S, L, 2], ``padding_mask`` [B, S] bool (True = padded) or None, ``act`` ACT_RELU / ACT_GELU;
    ``query_in`` is the ``query_out`` of the layer in front (``src + pos`` already formed)."""
    B, S, C = src.shape
    n_levels = attn.n_levels
    if reference_points.dim() != 4 or reference_points.shape[0] not in (1, B) or reference_points.shape[1] not in (1, S) or \
            reference_points.shape[2] not in (1, n_levels) or reference_points.shape[3] != 2:
        raise RuntimeError(f"deform_enc_layer_forward: reference_points {tuple(reference_points.shape)} does not broadcast to "
                           f"({B}, {S}, {n_levels}, 2)")
    if tuple(spatial_shapes.shape) != (n_levels, 2) or level_start_index.numel() != n_levels:
        raise RuntimeError(f"deform_enc_layer_forward: spatial_shapes {tuple(spatial_shapes.shape)} / level_start_index "
                           f"({level_start_index.numel()}) do not describe {n_levels} levels")
    if padding_mask is not None and tuple(padding_mask.shape) != (B, S):
        raise RuntimeError(f"deform_enc_layer_forward: padding mask {tuple(padding_mask.shape)} must be ({B}, {S})")
    L = _lib.lib()
    desc = _lib.VllmDeformEncLayerDesc()
    a = desc.attn
    a.d_model, a.n_heads, a.n_levels, a.n_points, a.ref_dim = C, attn.n_heads, n_levels, attn.n_points, 2
    a.use_4d_normalizer = 0
    desc.d_ffn, desc.act, desc.norm1_eps, desc.norm2_eps = linear1.out_features, act, norm1.eps, norm2.eps
    keep = []

    def put(struct, name, mod):
        w, b = _lib.aligned(mod.weight.detach()), _lib.aligned(mod.bias.detach())
        keep.extend((w, b))
        setattr(struct, name + "_w", w.data_ptr())
        setattr(struct, name + "_b", b.data_ptr())
    for name in _ATTN_LINEARS:
        put(a, name, getattr(attn, name))
    for name, mod in (("norm1", norm1), ("fc1", linear1), ("fc2", linear2), ("norm2", norm2)):
        put(desc, name, mod)
    x = _lib.aligned(src)
    p = None if pos is None else _lib.aligned(pos)
    q = None if query_in is None else _lib.aligned(query_in)
    ref = _lib.aligned(reference_points.to(torch.float32).expand(B, S, n_levels, 2), 8)
    shapes = spatial_shapes.to(device=x.device, dtype=torch.int64).contiguous()
    lsi = level_start_index.to(device=x.device, dtype=torch.int64).contiguous()
    mask = None if padding_mask is None else padding_mask.to(torch.uint8).contiguous()
    a.geometry = known_geometry(spatial_shapes, S)
    ws, wsb = _lib.sized_workspace(x.device, L.vllm_deform_enc_layer_workspace_bytes(ctypes.byref(desc), B, S),
                                   "vllm_deform_enc_layer_workspace_bytes")
    out = torch.empty_like(x)
    query_out = torch.empty_like(x) if want_query_out and p is not None else None
    with torch.cuda.device(x.device):
        _lib.check(L.vllm_deform_enc_layer_forward(ctypes.byref(desc), _lib.ptr(x), _lib.ptr(p), _lib.ptr(q), _lib.ptr(ref), _lib.ptr(mask),
                                                   _lib.ptr(shapes), _lib.ptr(lsi), B, S, _lib.ptr(out), _lib.ptr(query_out), _lib.ptr(ws),
                                                   wsb, _lib.current_stream(x.device)), "vllm_deform_enc_layer_forward")
    del keep
    return out, query_out


class DeformableTransformerEncoderLayer(nn.Module):
    """UniPose / Deformable-DETR encoder layer (unipose/modeling_unipose.py:3132-3186)."""

    native_layer = False   # True: bf16 inference runs vllm_deform_enc_layer_forward where native_layer_applies() holds

    def __init__(self,
                 d_model=256, d_ffn=1024,
                 dropout=0.1, activation="relu",
                 n_levels=4, n_heads=8, n_points=4,
                 add_channel_attention=False,
                 use_deformable_box_attn=False,
                 box_attn_type='roi_align',
                 ):
        super().__init__()
        if add_channel_attention:
            raise NotImplementedError("DeformableTransformerEncoderLayer: add_channel_attention (DyReLU) is not mirrored")
        if use_deformable_box_attn:
            raise NotImplementedError("DeformableTransformerEncoderLayer: use_deformable_box_attn is not mirrored")

        # self attention
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout)
        self.norm1 = nn.LayerNorm(d_model)

        # ffn
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = _get_activation_fn(activation, d_model=d_ffn)
        self.dropout2 = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout3 = nn.Dropout(dropout)
        self.norm2 = nn.LayerNorm(d_model)

        # channel attention
        self.add_channel_attention = add_channel_attention

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, src):
        src2 = self.linear2(self.dropout2(self.activation(self.linear1(src))))
        src = src + self.dropout3(src2)
        src = self.norm2(src)
        return src

    def native_layer_applies(self, src, pos, reference_points, query_in=None):
        """What vllm_deform_enc_layer_forward serves: a bf16 module and bf16 inputs on the GPU, nothing that needs a gradient, no active
        dropout, a relu / gelu activation, 2-d reference points, the fused attention's own conditions (msda_layer_fused_ok) and d_model
        (at most 512) and d_ffn multiples of 64."""
        return _applies(self, self.self_attn, (self.norm1, self.norm2), (self.linear1, self.linear2), _native_act(self.activation),
                        (self.dropout1.p, self.dropout2.p, self.dropout3.p), src, pos, reference_points, query_in)

    def _native_forward(self, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask, query_in=None,
                        want_query_out=False):
        assert level_pixels(spatial_shapes) == src.shape[1]   # MSDeformAttn.forward's own check (ms_deform_attn.py:100)
        return deform_enc_layer_forward(self.self_attn, self.norm1, self.linear1, _native_act(self.activation), self.linear2, self.norm2,
                                        src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask, query_in,
                                        want_query_out)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask=None):
        if self.native_layer and self.native_layer_applies(src, pos, reference_points):
            return self._native_forward(src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask)[0]
        # self attention
        src2 = self.self_attn(self.with_pos_embed(src, pos), reference_points, src,
                              spatial_shapes, level_start_index, key_padding_mask)
        src = src + self.dropout1(src2)
        src = self.norm1(src)

        # ffn
        src = self.forward_ffn(src)

        return src


class GroundingDinoDeformableLayer(nn.Module):
    """HF / Grounding-DINO encoder layer (modeling_ov_grounding_dino_mask_dn.py:1105-1180).  ``config`` needs ``d_model``,
    ``num_feature_levels``, ``encoder_attention_heads``, ``encoder_n_points``, ``encoder_ffn_dim``, ``dropout``,
    ``activation_function`` and ``activation_dropout``."""

    native_layer = False   # as DeformableTransformerEncoderLayer.native_layer

    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.d_model
        self.self_attn = GroundingDinoMultiscaleDeformableAttention(
            config, num_heads=config.encoder_attention_heads, n_points=config.encoder_n_points
        )
        self.self_attn_layer_norm = nn.LayerNorm(self.embed_dim)
        self.dropout = config.dropout
        self.activation_fn = _act2fn(config.activation_function)
        self.activation_dropout = config.activation_dropout
        self.fc1 = nn.Linear(self.embed_dim, config.encoder_ffn_dim)
        self.fc2 = nn.Linear(config.encoder_ffn_dim, self.embed_dim)
        self.final_layer_norm = nn.LayerNorm(self.embed_dim)

    def native_layer_applies(self, hidden_states, position_embeddings, reference_points, output_attentions=False, query_in=None):
        """As DeformableTransformerEncoderLayer.native_layer_applies; a call with ``output_attentions`` keeps the composed path (the
        attention weights stay inside the native call)."""
        if output_attentions:
            return False
        return _applies(self, self.self_attn, (self.self_attn_layer_norm, self.final_layer_norm), (self.fc1, self.fc2),
                        _native_act(self.activation_fn), (self.dropout, self.activation_dropout), hidden_states, position_embeddings,
                        reference_points, query_in)

    def _native_forward(self, hidden_states, attention_mask, position_embeddings, reference_points, spatial_shapes, level_start_index,
                        query_in=None, want_query_out=False):
        if level_pixels(spatial_shapes) != hidden_states.shape[1]:   # the attention module's own check (...mask_dn.py:741)
            raise ValueError("Make sure to align the spatial shapes with the sequence length of the encoder hidden states")
        return deform_enc_layer_forward(self.self_attn, self.self_attn_layer_norm, self.fc1, _native_act(self.activation_fn), self.fc2,
                                        self.final_layer_norm, hidden_states, position_embeddings, reference_points, spatial_shapes,
                                        level_start_index, None if attention_mask is None else ~attention_mask, query_in, want_query_out)

    def forward(
        self,
        hidden_states: torch.Tensor,
        attention_mask: torch.Tensor,
        position_embeddings: torch.Tensor = None,
        reference_points=None,
        spatial_shapes=None,
        level_start_index=None,
        output_attentions: bool = False,
    ):
        if self.native_layer and self.native_layer_applies(hidden_states, position_embeddings, reference_points, output_attentions):
            # (the attention weights stay inside the native call, as in the fused attention: ask for output_attentions to get them)
            return self._native_forward(hidden_states, attention_mask, position_embeddings, reference_points, spatial_shapes,
                                        level_start_index)[0], None
        residual = hidden_states

        # Apply Multi-scale Deformable Attention Module on the multi-scale feature maps.
        hidden_states, attn_weights = self.self_attn(
            hidden_states=hidden_states,
            attention_mask=attention_mask,
            encoder_hidden_states=hidden_states,
            encoder_attention_mask=attention_mask,
            position_embeddings=position_embeddings,
            reference_points=reference_points,
            spatial_shapes=spatial_shapes,
            level_start_index=level_start_index,
            output_attentions=output_attentions,
        )

        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = residual + hidden_states
        hidden_states = self.self_attn_layer_norm(hidden_states)

        residual = hidden_states
        hidden_states = self.activation_fn(self.fc1(hidden_states))
        hidden_states = nn.functional.dropout(hidden_states, p=self.activation_dropout, training=self.training)

        hidden_states = self.fc2(hidden_states)
        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)

        hidden_states = residual + hidden_states
        hidden_states = self.final_layer_norm(hidden_states)

        if self.training:
            if torch.isinf(hidden_states).any() or torch.isnan(hidden_states).any():
                clamp_value = torch.finfo(hidden_states.dtype).max - 1000
                hidden_states = torch.clamp(hidden_states, min=-clamp_value, max=clamp_value)

        return hidden_states, attn_weights


def encoder_layers_forward(layers, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask=None):
    """The encoder's loop over its layers (``key_padding_mask`` [B, S], True = padded) -> the last layer's output.  Layers whose native
    call applies are chained: each writes the next one's query ``out + pos`` from its last kernel, so only the first of a run adds
    ``pos`` in a kernel of its own.  A layer that keeps the composed path is called as the plain loop calls it."""
    layers = list(layers)
    output, query = src, None
    for i, layer in enumerate(layers):
        gdino = isinstance(layer, GroundingDinoDeformableLayer)
        native = isinstance(layer, (DeformableTransformerEncoderLayer, GroundingDinoDeformableLayer)) and layer.native_layer and \
            (layer.native_layer_applies(output, pos, reference_points, query_in=query))
        if native:
            more = i + 1 < len(layers)
            if gdino:
                output, query = layer._native_forward(output, None if key_padding_mask is None else ~key_padding_mask, pos, reference_points,
                                                      spatial_shapes, level_start_index, query, more)
            else:
                output, query = layer._native_forward(output, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask,
                                                      query, more)
            continue
        query = None
        if gdino:
            output = layer(output, None if key_padding_mask is None else ~key_padding_mask, pos, reference_points, spatial_shapes,
                           level_start_index)[0]
        else:
            output = layer(output, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask)
    return output
