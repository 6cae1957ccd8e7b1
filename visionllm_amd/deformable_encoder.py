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
from torch import nn

from . import _lib
from ._native_call import (act2fn, fill_msda_desc, get_activation_fn, is_gpu_bf16, memory_operands, module_reasons, msda_params,
                           native_act, opt_aligned, put)
from .ms_deform_attn import GroundingDinoMultiscaleDeformableAttention, MSDeformAttn, known_geometry, level_pixels


def _reasons(layer, attn, norms, linears, act, dropouts, src, pos, reference_points, query_in=None):
    """Every reason why ``vllm_deform_enc_layer_forward`` does not serve this call, as a list of strings (empty: it does): the inputs'
    own, then the module's (module_reasons, the decoder layers' words).  Only the layer's norms and FFN linears are asked for bf16 GPU
    parameters here; the attention linears answer through msda_layer_fused_ok."""
    why = []
    if not is_gpu_bf16(src):
        why.append("src: a bf16 CUDA tensor [B, S, C]")
        if not (torch.is_tensor(src) and src.dim() == 3):
            return why
    if any(t is not None and not (is_gpu_bf16(t) and t.shape == src.shape) for t in (pos, query_in)):
        why.append("pos / query_in: bf16 CUDA tensors of src's shape")
    return why + module_reasons(layer.training, tuple(norms) + tuple(linears), dropouts, act, attn, "self-attention", src, src,
                                reference_points, (2,), (src, pos, query_in), linears[0].out_features)


def deform_enc_layer_forward(attn, norm1, linear1, act, linear2, norm2, src, pos, reference_points, spatial_shapes, level_start_index,
                             padding_mask=None, query_in=None, want_query_out=False):
    """One ``vllm_deform_enc_layer_forward`` call -> (out, query_out or None).  ``src`` [B, S, C] bf16 on the GPU, ``pos`` the same or
    None, ``reference_points`` [B, S, L, 2], ``padding_mask`` [B, S] bool (True = padded) or None, ``act`` ACT_RELU / ACT_GELU;
    ``query_in`` is the ``query_out`` of the layer in front (``src + pos`` already formed)."""
    B, S, C = src.shape
    x, ref, _, shapes, lsi, mask = memory_operands("deform_enc_layer_forward", src, reference_points, src, spatial_shapes, level_start_index,
                                                   padding_mask, attn.n_levels, ref_dim=2)
    p, q = opt_aligned(pos), opt_aligned(query_in)
    L = _lib.lib()
    desc = _lib.VllmDeformEncLayerDesc()
    desc.d_ffn, desc.act, desc.norm1_eps, desc.norm2_eps = linear1.out_features, act, norm1.eps, norm2.eps
    keep = []
    fill_msda_desc(desc.attn, keep, C, attn.n_heads, attn.n_levels, attn.n_points, 2, False, msda_params(attn))
    for name, mod in (("norm1", norm1), ("fc1", linear1), ("fc2", linear2), ("norm2", norm2)):
        put(desc, keep, name, mod.weight, mod.bias)
    desc.attn.geometry = known_geometry(spatial_shapes, S)
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
        self.activation = get_activation_fn(activation, d_model=d_ffn)
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

    def native_layer_reasons(self, src, pos, reference_points, query_in=None):
        """why this call keeps the composed path, as a list of strings (empty: the native call serves it)"""
        return _reasons(self, self.self_attn, (self.norm1, self.norm2), (self.linear1, self.linear2), native_act(self.activation),
                        (self.dropout1.p, self.dropout2.p, self.dropout3.p), src, pos, reference_points, query_in)

    def native_layer_applies(self, src, pos, reference_points, query_in=None):
        """What vllm_deform_enc_layer_forward serves: a bf16 module and bf16 inputs on the GPU, nothing that needs a gradient, no active
        dropout, a relu / gelu activation, 2-d reference points, the fused attention's own conditions (msda_layer_fused_ok) and d_model
        (at most 512) and d_ffn multiples of 64."""
        return not self.native_layer_reasons(src, pos, reference_points, query_in)

    def _native_forward(self, src, pos, reference_points, spatial_shapes, level_start_index, key_padding_mask, query_in=None,
                        want_query_out=False):
        assert level_pixels(spatial_shapes) == src.shape[1]   # MSDeformAttn.forward's own check (ms_deform_attn.py:100)
        return deform_enc_layer_forward(self.self_attn, self.norm1, self.linear1, native_act(self.activation), self.linear2, self.norm2,
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
        self.activation_fn = act2fn(config.activation_function)
        self.activation_dropout = config.activation_dropout
        self.fc1 = nn.Linear(self.embed_dim, config.encoder_ffn_dim)
        self.fc2 = nn.Linear(config.encoder_ffn_dim, self.embed_dim)
        self.final_layer_norm = nn.LayerNorm(self.embed_dim)

    def native_layer_reasons(self, hidden_states, position_embeddings, reference_points, output_attentions=False, query_in=None):
        """why this call keeps the composed path, as a list of strings (empty: the native call serves it)"""
        why = _reasons(self, self.self_attn, (self.self_attn_layer_norm, self.final_layer_norm), (self.fc1, self.fc2),
                       native_act(self.activation_fn), (self.dropout, self.activation_dropout), hidden_states, position_embeddings,
                       reference_points, query_in)
        if output_attentions:
            why.append("output_attentions: the attention weights stay inside the native call")
        return why

    def native_layer_applies(self, hidden_states, position_embeddings, reference_points, output_attentions=False, query_in=None):
        """As DeformableTransformerEncoderLayer.native_layer_applies; a call with ``output_attentions`` keeps the composed path."""
        return not self.native_layer_reasons(hidden_states, position_embeddings, reference_points, output_attentions, query_in)

    def _native_forward(self, hidden_states, attention_mask, position_embeddings, reference_points, spatial_shapes, level_start_index,
                        query_in=None, want_query_out=False):
        if level_pixels(spatial_shapes) != hidden_states.shape[1]:   # the attention module's own check (...mask_dn.py:741)
            raise ValueError("Make sure to align the spatial shapes with the sequence length of the encoder hidden states")
        return deform_enc_layer_forward(self.self_attn, self.self_attn_layer_norm, self.fc1, native_act(self.activation_fn), self.fc2,
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
