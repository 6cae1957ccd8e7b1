"""The deformable DECODER layers of the detection and pose heads: module mirrors and the one-call native forward.

Same constructor arguments, parameter names and ``forward`` signatures as

* ``DeformableTransformerDecoderLayer`` -- visionllmv2/model/unipose/modeling_unipose.py:3188-3323;
* ``GroundingDinoDecoderLayer``         -- visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1292-1407,

with ``self_attn`` / ``ca_text`` / ``encoder_attn_text`` torch's own ``nn.MultiheadAttention`` (state-dicts load) and ``cross_attn`` /
``encoder_attn`` this package's ``MSDeformAttn`` / ``GroundingDinoMultiscaleDeformableAttention``.  With the class attribute
``native_layer = False`` (the default) ``forward`` is the reference's statements, line for line.  With ``native_layer = True`` the
inference forward of a bf16 module is ONE native call (``vllm_deform_dec_layer_forward``, csrc/deform_decoder_layer.hip; conditions:
``native_layer_applies``); every other call runs the composed statements unchanged.

The UniPose layer is sequence-first (``tgt`` [nq, bs, C]) and the native entry batch-first: its mirror transposes ``tgt``,
``tgt_query_pos``, the reference points and ``memory`` on entry and the result on exit -- views where bs == 1, copies otherwise (the
composed path's attention module makes the same copy of ``memory``).

``GroundingDinoDecoder`` (...mask_dn.py:1725-1981) is the loop around the Grounding-DINO layers -- reference points times
``valid_ratios``, the sine embedding and its MLP, ``layer_norm``, ``bbox_embed`` and the iterative box refinement -- with the same
arrangement one level up: ``native_decoder = False`` (the default) runs the reference's statements, ``native_decoder = True`` makes the
inference forward of a bf16 module ONE native call (``vllm_deform_decoder_forward``, csrc/deform_decoder.hip) wherever
``native_decoder_reasons`` is empty.
"""
import ctypes
import dataclasses
import math
import weakref

import torch
from torch import nn

from . import _lib
from ._native_call import (MSDA_LINEARS, act2fn, fill_msda_desc, get_activation_fn, is_gpu_bf16, mask_u8, memory_operands, module_reasons,
                           msda_params, native_act, opt_aligned, put)
from .ms_deform_attn import GroundingDinoMultiscaleDeformableAttention, MSDeformAttn, known_geometry, level_pixels


def _mha_reasons(name, mha, d_model):
    """why the native attention kernel cannot stand in for this nn.MultiheadAttention (empty: it can)"""
    out = []
    if not getattr(mha, "_qkv_same_embed_dim", False) or mha.in_proj_weight is None:
        out.append(f"{name}: separate q / k / v projection weights")
        return out
    if mha.in_proj_bias is None or mha.out_proj.bias is None:
        out.append(f"{name}: no bias")
    if mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
        out.append(f"{name}: bias_k / add_zero_attn")
    if mha.embed_dim != d_model or mha.head_dim not in (32, 64):
        out.append(f"{name}: head dim {mha.head_dim} (32 or 64)")
    return out


def native_layer_reasons(layer, parts, tgt, pos, reference_points, memory_text, text_mask, memory, self_attn_mask, batch_first):
    """Every reason why ``vllm_deform_dec_layer_forward`` does not serve this call, as a list of strings (empty: it does).  ``parts`` is
    the layer's ``_parts()``; tensors as the layer's ``forward`` receives them (``batch_first`` tells the layout of tgt / pos / memory)."""
    why = []
    if not (is_gpu_bf16(tgt) and is_gpu_bf16(memory)):
        why.append("tgt / memory: bf16 CUDA tensors [., ., C]")
        if not (torch.is_tensor(tgt) and tgt.dim() == 3 and torch.is_tensor(memory) and memory.dim() == 3):
            return why
    if pos is not None and not (is_gpu_bf16(pos) and pos.shape == tgt.shape):
        why.append("query_pos: a bf16 CUDA tensor of tgt's shape")
    bdim, qdim = (0, 1) if batch_first else (1, 0)
    B, Lq, C = tgt.shape[bdim], tgt.shape[qdim], tgt.shape[2]
    sa, ta = parts["self_attn"], parts["text_attn"]
    mods = [parts["ca_norm"], parts["fc1"], parts["fc2"], parts["ffn_norm"]] + [getattr(parts["cross_attn"], n) for n in MSDA_LINEARS]
    if sa is not None:
        mods += [sa, parts["sa_norm"]]
    if ta is not None:
        mods += [ta, parts["text_norm"]]
    why += module_reasons(layer.training, mods, parts["dropouts"], parts["act"], parts["cross_attn"], "cross-attention", tgt, memory,
                          reference_points, (2, 4), (tgt, pos, memory, memory_text, reference_points), parts["fc1"].out_features)
    if sa is not None:
        why += _mha_reasons("self_attn", sa, C)
        if self_attn_mask is not None and not (torch.is_tensor(self_attn_mask) and self_attn_mask.dtype == torch.bool and
                                               tuple(self_attn_mask.shape) == (Lq, Lq)):
            why.append("self_attn_mask: None or a 2-d bool [Lq, Lq] (float and per-head masks keep the composed path)")
    if ta is not None:
        why += _mha_reasons("text attention", ta, C)
        if not (torch.is_tensor(memory_text) and memory_text.dim() == 3 and memory_text.shape[0] == B and memory_text.shape[2] == C and
                memory_text.shape[1] > 0 and memory_text.dtype == torch.bfloat16 and memory_text.is_cuda):
            why.append("memory_text: a bf16 CUDA tensor [B, Lt, C]")
        if text_mask is not None and not (torch.is_tensor(text_mask) and text_mask.dtype == torch.bool and torch.is_tensor(memory_text) and
                                          memory_text.dim() == 3 and tuple(text_mask.shape) == (B, memory_text.shape[1])):
            why.append("text mask: None or bool [B, Lt]")
    return why


def _fill_layer_desc(desc, parts, C, ref_dim, keep):
    """``desc`` (a VllmDeformDecLayerDesc) from a layer's ``_parts()``, everything but ``cross_attn.geometry``; the tensors whose
    pointers it holds are appended to ``keep``"""
    attn = parts["cross_attn"]
    fill_msda_desc(desc.cross_attn, keep, C, attn.n_heads, attn.n_levels, attn.n_points, ref_dim, getattr(attn, "use_4D_normalizer", False),
                   msda_params(attn))
    sa, ta = parts["self_attn"], parts["text_attn"]
    desc.d_ffn, desc.act = parts["fc1"].out_features, parts["act"]
    desc.has_self_attn, desc.has_text_attn = int(sa is not None), int(ta is not None)
    desc.n_heads_sa = sa.num_heads if sa is not None else ta.num_heads if ta is not None else 0
    desc.ca_norm_eps, desc.ffn_norm_eps = parts["ca_norm"].eps, parts["ffn_norm"].eps
    for name in ("ca_norm", "fc1", "fc2", "ffn_norm"):
        put(desc, keep, name, parts[name].weight, parts[name].bias)
    for pre, mha, norm in (("sa", sa, parts["sa_norm"]), ("text", ta, parts["text_norm"])):
        if mha is not None:
            put(desc, keep, pre + "_in_proj", mha.in_proj_weight, mha.in_proj_bias)
            put(desc, keep, pre + "_out_proj", mha.out_proj.weight, mha.out_proj.bias)
            put(desc, keep, pre + "_norm", norm.weight, norm.bias)
            setattr(desc, pre + "_norm_eps", norm.eps)


def deform_dec_layer_forward(parts, tgt, pos, reference_points, self_attn_mask, memory_text, text_mask, memory, memory_padding_mask,
                             spatial_shapes, level_start_index):
    """One ``vllm_deform_dec_layer_forward`` call -> out [B, Lq, C].  Batch-first: ``tgt`` [B, Lq, C] bf16 on the GPU, ``pos`` the same or
    None, ``reference_points`` [B, Lq, L, 2 | 4], ``self_attn_mask`` bool [Lq, Lq] (True = may not attend) or None, ``memory_text``
    [B, Lt, C], ``text_mask`` bool [B, Lt] (True = ignore) or None, ``memory`` [B, S, C], ``memory_padding_mask`` bool [B, S] (True =
    padded) or None."""
    B, Lq, C = tgt.shape
    S = memory.shape[1]
    x, ref, mem, shapes, lsi, pmask = memory_operands("deform_dec_layer_forward", tgt, reference_points, memory, spatial_shapes,
                                                      level_start_index, memory_padding_mask, parts["cross_attn"].n_levels)
    p = opt_aligned(pos)
    L = _lib.lib()
    desc = _lib.VllmDeformDecLayerDesc()
    keep = []
    _fill_layer_desc(desc, parts, C, ref.shape[-1], keep)
    sam = mask_u8(self_attn_mask, x.device) if parts["self_attn"] is not None else None
    text, tmask, Lt = None, None, 0
    if parts["text_attn"] is not None:
        text, tmask, Lt = _lib.aligned(memory_text), mask_u8(text_mask, x.device), memory_text.shape[1]
    desc.cross_attn.geometry = known_geometry(spatial_shapes, Lq)
    ws, wsb = _lib.sized_workspace(x.device, L.vllm_deform_dec_layer_workspace_bytes(ctypes.byref(desc), B, Lq, Lt, S),
                                   "vllm_deform_dec_layer_workspace_bytes")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(L.vllm_deform_dec_layer_forward(ctypes.byref(desc), _lib.ptr(x), _lib.ptr(p), _lib.ptr(ref), _lib.ptr(sam), _lib.ptr(text),
                                                   _lib.ptr(tmask), _lib.ptr(mem), _lib.ptr(pmask), _lib.ptr(shapes), _lib.ptr(lsi), B, Lq, Lt, S,
                                                   _lib.ptr(out), _lib.ptr(ws), wsb, _lib.current_stream(x.device)),
                   "vllm_deform_dec_layer_forward")
    del keep
    return out


class DeformableTransformerDecoderLayer(nn.Module):
    """UniPose / DINO decoder layer (unipose/modeling_unipose.py:3188-3323)."""

    native_layer = False   # True: bf16 inference runs vllm_deform_dec_layer_forward where native_layer_applies() holds

    def __init__(self, d_model=256, d_ffn=1024,
                 dropout=0.1, activation="relu",
                 n_levels=4, n_heads=8, n_points=4,
                 use_text_feat_guide=False,
                 use_text_cross_attention=False,
                 ffn_extra_layernorm=False
                 ):
        super().__init__()

        # cross attention
        self.cross_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.dropout1 = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.norm1 = nn.LayerNorm(d_model)

        # cross attention text
        if use_text_cross_attention:
            self.ca_text = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
            self.catext_dropout = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
            self.catext_norm = nn.LayerNorm(d_model)

        # self attention
        self.self_attn = nn.MultiheadAttention(d_model, n_heads, dropout=dropout)
        self.dropout2 = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.norm2 = nn.LayerNorm(d_model)

        # ffn
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.activation = get_activation_fn(activation, d_model=d_ffn, batch_dim=1)
        self.dropout3 = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.dropout4 = nn.Dropout(dropout) if dropout > 0 else nn.Identity()
        self.norm3 = nn.LayerNorm(d_model)
        if ffn_extra_layernorm:
            raise NotImplementedError('ffn_extra_layernorm not implemented')
        else:
            self.norm_ext = None

        self.key_aware_proj = None
        self.use_text_feat_guide = use_text_feat_guide
        assert not use_text_feat_guide
        self.use_text_cross_attention = use_text_cross_attention

    def rm_self_attn_modules(self):
        self.self_attn = None
        self.dropout2 = None
        self.norm2 = None

    @staticmethod
    def with_pos_embed(tensor, pos):
        return tensor if pos is None else tensor + pos

    def forward_ffn(self, tgt, ipdb_flag=False):

        with torch.amp.autocast("cuda", enabled=False):   # (the reference spells it torch.cuda.amp.autocast, which newer torch deprecates)
            tgt2 = self.linear2(self.dropout3(self.activation(self.linear1(tgt))))

        tgt = tgt + self.dropout4(tgt2)
        tgt = self.norm3(tgt)
        return tgt

    def _parts(self):
        text = self.ca_text if self.use_text_cross_attention else None
        drops = [getattr(m, "p", 0.0) for m in (self.dropout1, self.dropout3, self.dropout4)]
        if self.self_attn is not None:
            drops += [getattr(self.dropout2, "p", 0.0), self.self_attn.dropout]
        if text is not None:
            drops += [getattr(self.catext_dropout, "p", 0.0), text.dropout]
        return dict(cross_attn=self.cross_attn, self_attn=self.self_attn, sa_norm=self.norm2, text_attn=text,
                    text_norm=self.catext_norm if text is not None else None, ca_norm=self.norm1, fc1=self.linear1, fc2=self.linear2,
                    ffn_norm=self.norm3, act=native_act(self.activation), dropouts=drops)

    def native_layer_reasons(self, tgt, tgt_query_pos=None, tgt_reference_points=None, memory_text=None, text_attention_mask=None,
                             memory=None, self_attn_mask=None, cross_attn_mask=None):
        """why this call keeps the composed path, as a list of strings (empty: the native call serves it)"""
        why = native_layer_reasons(self, self._parts(), tgt, tgt_query_pos, tgt_reference_points, memory_text, text_attention_mask, memory,
                                   self_attn_mask, batch_first=False)
        if cross_attn_mask is not None:
            why.append("cross_attn_mask")
        return why

    def native_layer_applies(self, *args, **kwargs):
        """What vllm_deform_dec_layer_forward serves: bf16 CUDA inputs; every parameter bf16, with biases; nothing that needs a gradient
        under grad mode; no active dropout (the attention modules' own included); a relu / gelu activation; the fused cross-attention's
        conditions (msda_layer_fused_ok); packed in_proj weights, no bias_k / add_zero_attn, head dim 32 or 64; ``self_attn_mask`` None or
        a 2-d bool [Lq, Lq]; the text mask None or bool [B, Lt]; no ``cross_attn_mask``; d_model (at most 512) and d_ffn multiples of 64."""
        return not self.native_layer_reasons(*args, **kwargs)

    def _native_forward(self, tgt, tgt_query_pos, tgt_reference_points, memory_text, text_attention_mask, memory, memory_key_padding_mask,
                        memory_level_start_index, memory_spatial_shapes, self_attn_mask):
        assert level_pixels(memory_spatial_shapes) == memory.shape[0]   # MSDeformAttn.forward's own check (ms_deform_attn.py:100)
        out = deform_dec_layer_forward(self._parts(), tgt.transpose(0, 1), None if tgt_query_pos is None else tgt_query_pos.transpose(0, 1),
                                       tgt_reference_points.transpose(0, 1), self_attn_mask, memory_text, text_attention_mask,
                                       memory.transpose(0, 1), memory_key_padding_mask, memory_spatial_shapes, memory_level_start_index)
        return out.transpose(0, 1)

    def forward(self,
                # for tgt
                tgt,  # nq, bs, d_model
                tgt_query_pos=None,  # pos for query. MLP(Sine(pos))
                tgt_query_sine_embed=None,  # pos for query. Sine(pos)
                tgt_key_padding_mask=None,
                tgt_reference_points=None,  # nq, bs, 4

                memory_text=None,  # bs, num_token, d_model
                text_attention_mask=None,  # bs, num_token

                # for memory
                memory=None,  # hw, bs, d_model
                memory_key_padding_mask=None,
                memory_level_start_index=None,  # num_levels
                memory_spatial_shapes=None,  # bs, num_levels, 2
                memory_pos=None,  # pos for memory

                # sa
                self_attn_mask=None,  # mask used for self-attention
                cross_attn_mask=None,  # mask used for cross-attention
                ):
        """
        Input:
            - tgt/tgt_query_pos: nq, bs, d_model
            -
        """
        assert cross_attn_mask is None

        if self.native_layer and self.native_layer_applies(tgt, tgt_query_pos, tgt_reference_points, memory_text, text_attention_mask, memory,
                                                           self_attn_mask, cross_attn_mask):
            return self._native_forward(tgt, tgt_query_pos, tgt_reference_points, memory_text, text_attention_mask, memory,
                                        memory_key_padding_mask, memory_level_start_index, memory_spatial_shapes, self_attn_mask)

        # self attention
        if self.self_attn is not None:
            q = k = self.with_pos_embed(tgt, tgt_query_pos)
            tgt2 = self.self_attn(q, k, tgt, attn_mask=self_attn_mask)[0]
            tgt = tgt + self.dropout2(tgt2)
            tgt = self.norm2(tgt)

        if self.use_text_cross_attention:
            tgt2 = self.ca_text(self.with_pos_embed(tgt, tgt_query_pos), memory_text.transpose(0, 1),
                                memory_text.transpose(0, 1), key_padding_mask=text_attention_mask)[0]
            tgt = tgt + self.catext_dropout(tgt2)
            tgt = self.catext_norm(tgt)

        tgt2 = self.cross_attn(self.with_pos_embed(tgt, tgt_query_pos).transpose(0, 1),
                               tgt_reference_points.transpose(0, 1).contiguous(),
                               memory.transpose(0, 1),
                               memory_spatial_shapes, memory_level_start_index,
                               memory_key_padding_mask).transpose(0, 1)
        tgt = tgt + self.dropout1(tgt2)
        tgt = self.norm1(tgt)

        # ffn
        tgt = self.forward_ffn(tgt)

        return tgt


class GroundingDinoDecoderLayer(nn.Module):
    """HF / Grounding-DINO decoder layer (modeling_ov_grounding_dino_mask_dn.py:1292-1407).  ``config`` needs ``d_model``,
    ``num_feature_levels``, ``decoder_attention_heads``, ``decoder_n_points``, ``decoder_ffn_dim``, ``dropout``, ``attention_dropout``,
    ``activation_function`` and ``activation_dropout``."""

    native_layer = False   # as DeformableTransformerDecoderLayer.native_layer

    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.d_model

        # self-attention
        self.self_attn = nn.MultiheadAttention(
            embed_dim=self.embed_dim,
            num_heads=config.decoder_attention_heads,
            dropout=config.attention_dropout,
            batch_first=True,
        )
        self.dropout = config.dropout
        self.activation_fn = act2fn(config.activation_function)
        self.activation_dropout = config.activation_dropout

        self.self_attn_layer_norm = nn.LayerNorm(self.embed_dim)
        # cross-attention text
        self.encoder_attn_text = nn.MultiheadAttention(
            embed_dim=self.embed_dim,
            num_heads=config.decoder_attention_heads,
            dropout=config.attention_dropout,
            batch_first=True,
        )
        self.encoder_attn_text_layer_norm = nn.LayerNorm(self.embed_dim)
        # cross-attention
        self.encoder_attn = GroundingDinoMultiscaleDeformableAttention(
            config,
            num_heads=config.decoder_attention_heads,
            n_points=config.decoder_n_points,
        )
        self.encoder_attn_layer_norm = nn.LayerNorm(self.embed_dim)
        # feedforward neural networks
        self.fc1 = nn.Linear(self.embed_dim, config.decoder_ffn_dim)
        self.fc2 = nn.Linear(config.decoder_ffn_dim, self.embed_dim)
        self.final_layer_norm = nn.LayerNorm(self.embed_dim)

    def with_pos_embed(self, tensor, position_embeddings):
        return tensor if position_embeddings is None else tensor + position_embeddings

    def _parts(self):
        return dict(cross_attn=self.encoder_attn, self_attn=self.self_attn, sa_norm=self.self_attn_layer_norm,
                    text_attn=self.encoder_attn_text, text_norm=self.encoder_attn_text_layer_norm, ca_norm=self.encoder_attn_layer_norm,
                    fc1=self.fc1, fc2=self.fc2, ffn_norm=self.final_layer_norm, act=native_act(self.activation_fn),
                    dropouts=[self.dropout, self.activation_dropout, self.self_attn.dropout, self.encoder_attn_text.dropout])

    def native_layer_reasons(self, hidden_states, position_embeddings=None, reference_points=None, vision_encoder_hidden_states=None,
                             text_encoder_hidden_states=None, text_encoder_attention_mask=None, self_attn_mask=None,
                             output_attentions=False):
        """why this call keeps the composed path, as a list of strings (empty: the native call serves it)"""
        why = native_layer_reasons(self, self._parts(), hidden_states, position_embeddings, reference_points, text_encoder_hidden_states,
                                   text_encoder_attention_mask, vision_encoder_hidden_states, self_attn_mask, batch_first=True)
        if output_attentions:
            why.append("output_attentions: the attention weights stay inside the native call")
        return why

    def native_layer_applies(self, *args, **kwargs):
        """As DeformableTransformerDecoderLayer.native_layer_applies; a call with ``output_attentions`` keeps the composed path."""
        return not self.native_layer_reasons(*args, **kwargs)

    def forward(
        self,
        hidden_states: torch.Tensor,
        position_embeddings=None,
        reference_points=None,
        spatial_shapes=None,
        level_start_index=None,
        vision_encoder_hidden_states=None,
        vision_encoder_attention_mask=None,
        text_encoder_hidden_states=None,
        text_encoder_attention_mask=None,
        self_attn_mask=None,
        output_attentions=False,
    ):
        if self.native_layer and self.native_layer_applies(hidden_states, position_embeddings, reference_points, vision_encoder_hidden_states,
                                                           text_encoder_hidden_states, text_encoder_attention_mask, self_attn_mask,
                                                           output_attentions):
            if level_pixels(spatial_shapes) != vision_encoder_hidden_states.shape[1]:   # the attention module's own check (...mask_dn.py:741)
                raise ValueError("Make sure to align the spatial shapes with the sequence length of the encoder hidden states")
            return (deform_dec_layer_forward(self._parts(), hidden_states, position_embeddings, reference_points, self_attn_mask,
                                             text_encoder_hidden_states, text_encoder_attention_mask, vision_encoder_hidden_states,
                                             None if vision_encoder_attention_mask is None else ~vision_encoder_attention_mask,
                                             spatial_shapes, level_start_index),)
        residual = hidden_states

        # Self Attention
        q = k = self.with_pos_embed(hidden_states, position_embeddings)
        hidden_states, self_attn_weights = self.self_attn(
            query=q, key=k, value=hidden_states, attn_mask=self_attn_mask, average_attn_weights=False
        )

        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = residual + hidden_states
        hidden_states = self.self_attn_layer_norm(hidden_states)

        second_residual = hidden_states

        # Cross-Attention Text
        hidden_states, text_cross_attn_weights = self.encoder_attn_text(
            query=self.with_pos_embed(hidden_states, position_embeddings),
            key=text_encoder_hidden_states,
            value=text_encoder_hidden_states,
            key_padding_mask=text_encoder_attention_mask,
            average_attn_weights=False,
        )

        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = second_residual + hidden_states
        hidden_states = self.encoder_attn_text_layer_norm(hidden_states)

        third_residual = hidden_states

        # Cross-Attention
        cross_attn_weights = None
        hidden_states, cross_attn_weights = self.encoder_attn(
            hidden_states=hidden_states,
            attention_mask=vision_encoder_attention_mask,
            encoder_hidden_states=vision_encoder_hidden_states,
            encoder_attention_mask=vision_encoder_attention_mask,
            position_embeddings=position_embeddings,
            reference_points=reference_points,
            spatial_shapes=spatial_shapes,
            level_start_index=level_start_index,
            output_attentions=output_attentions,
        )

        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = third_residual + hidden_states
        hidden_states = self.encoder_attn_layer_norm(hidden_states)

        # Fully Connected
        residual = hidden_states
        hidden_states = self.activation_fn(self.fc1(hidden_states))
        hidden_states = nn.functional.dropout(hidden_states, p=self.activation_dropout, training=self.training)
        hidden_states = self.fc2(hidden_states)
        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = residual + hidden_states
        hidden_states = self.final_layer_norm(hidden_states)

        outputs = (hidden_states,)

        if output_attentions:
            outputs += (self_attn_weights, text_cross_attn_weights, cross_attn_weights)

        return outputs


# ---- the Grounding-DINO decoder around the layer (modeling_ov_grounding_dino_mask_dn.py:1725-1981) ---------------------------------------
def inverse_sigmoid(x, eps=1e-5):
    """modeling_ov_grounding_dino_mask_dn.py:401-405"""
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


class GroundingDinoMLPPredictionHead(nn.Module):
    """The DETR MLP head (modeling_ov_grounding_dino_mask_dn.py:3704-3720): ``layers.N`` are Linears, ReLU between them."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = nn.functional.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


@dataclasses.dataclass
class GroundingDinoDecoderOutput:
    """The fields of the reference's ModelOutput of the same name (:183-211), as a plain dataclass."""
    last_hidden_state: torch.Tensor = None
    intermediate_hidden_states: torch.Tensor = None
    intermediate_reference_points: torch.Tensor = None
    hidden_states: tuple = None
    attentions: tuple = None


def _box_heads(bbox_embed, n_layers, d_model):
    """``bbox_embed`` as a list of n_layers three-layer heads of width d_model (entries may be one shared module), or None where it is
    anything else"""
    try:
        heads = list(bbox_embed)
    except TypeError:
        return None
    if len(heads) != n_layers:
        return None
    for h in heads:
        lin = list(getattr(h, "layers", ()))
        if getattr(h, "num_layers", None) != 3 or len(lin) != 3 or not all(isinstance(m, nn.Linear) and m.bias is not None for m in lin):
            return None
        if [tuple(m.weight.shape) for m in lin] != [(d_model, d_model), (d_model, d_model), (4, d_model)]:
            return None
    return heads


_NATIVE_STATE = weakref.WeakKeyDictionary()   # GroundingDinoDecoder -> {device: (signature, descriptors and what they point to)}


class GroundingDinoDecoder(nn.Module):
    """The Grounding-DINO decoder (modeling_ov_grounding_dino_mask_dn.py:1725-1981): parameter names ``layer_norm``, ``layers.N.*`` and
    ``reference_points_head.layers.{0,1}``; ``bbox_embed``, ``class_embed`` and ``query_scale`` are assigned from outside, as there.
    ``config`` needs what GroundingDinoDecoderLayer needs, and ``decoder_layers`` and ``query_dim``; ``output_attentions``,
    ``output_hidden_states`` and ``use_return_dict`` are read where ``forward`` is not told (defaults False, False, True).

    With the class attribute ``native_decoder = False`` (the default) ``forward`` is the reference's statements, line for line, and every
    layer honours its own ``native_layer``.  With ``native_decoder = True`` a call for which ``native_decoder_reasons`` is empty is ONE
    ``vllm_deform_decoder_forward`` (csrc/deform_decoder.hip); every other call runs the composed statements unchanged.

    The native call writes layer-major buffers, so ``intermediate_hidden_states`` [B, n_layers, Lq, C] and
    ``intermediate_reference_points`` [B, n_layers, Lq, 4] come back as ``.transpose(0, 1)`` VIEWS of them: the shapes and values of the
    reference's ``torch.stack(dim=1)``, but not contiguous.  ``last_hidden_state`` is ``intermediate_hidden_states[:, -1]``.  Reference
    points may be fp32 or bf16: they are widened once on entry, kept fp32 through every layer and returned in the caller's dtype.
    Descriptors and the ``dim_t`` table are remembered per device (and rebuilt when a parameter's storage changes); no weight is copied."""

    native_decoder = False   # True: bf16 inference runs vllm_deform_decoder_forward where native_decoder_reasons() is empty

    def __init__(self, config):
        super().__init__()
        self.config = config

        self.dropout = config.dropout
        self.layer_norm = nn.LayerNorm(config.d_model)
        self.layers = nn.ModuleList([GroundingDinoDecoderLayer(config) for _ in range(config.decoder_layers)])
        self.reference_points_head = GroundingDinoMLPPredictionHead(
            config.query_dim // 2 * config.d_model, config.d_model, config.d_model, 2
        )
        self.gradient_checkpointing = False

        # hack implementation for iterative bounding box refinement and two-stage Deformable DETR
        self.bbox_embed = None
        self.class_embed = None
        self.query_scale = None

    @staticmethod
    def _dim_t(num_pos_feats, device):
        temperature = 10000
        dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=device)
        dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
        return dim_t

    def get_proposal_pos_embed(self, proposals):
        """Get the position embedding of the proposals."""
        num_pos_feats = self.config.d_model // 2
        scale = 2 * math.pi

        dim_t = self._dim_t(num_pos_feats, proposals.device)
        # batch_size, num_queries
        pos_x = proposals[:, :, 0] * scale
        pos_y = proposals[:, :, 1] * scale
        # batch_size, num_queries, num_pos_feats
        pos_x = pos_x[:, :, None] / dim_t
        pos_y = pos_y[:, :, None] / dim_t
        # batch_size, num_queries, num_pos_feats
        pos_x = torch.stack((pos_x[:, :, 0::2].sin(), pos_x[:, :, 1::2].cos()), dim=3).flatten(2)
        pos_y = torch.stack((pos_y[:, :, 0::2].sin(), pos_y[:, :, 1::2].cos()), dim=3).flatten(2)

        if proposals.size(-1) == 2:
            # batch_size, num_queries, num_pos_feats * 2
            pos = torch.cat((pos_y, pos_x), dim=2)
        elif proposals.size(-1) == 4:
            w_embed = proposals[:, :, 2] * scale
            pos_w = w_embed[:, :, None] / dim_t
            # batch_size, num_queries, num_pos_feats
            pos_w = torch.stack((pos_w[:, :, 0::2].sin(), pos_w[:, :, 1::2].cos()), dim=3).flatten(2)

            h_embed = proposals[:, :, 3] * scale
            pos_h = h_embed[:, :, None] / dim_t
            # batch_size, num_queries, num_pos_feats
            pos_h = torch.stack((pos_h[:, :, 0::2].sin(), pos_h[:, :, 1::2].cos()), dim=3).flatten(2)
            # batch_size, num_queries, num_pos_feats * 4
            pos = torch.cat((pos_y, pos_x, pos_w, pos_h), dim=2)
        else:
            raise ValueError("Unknown proposals shape(-1):{}".format(proposals.size(-1)))
        return pos

    def _own_params(self):
        heads = _box_heads(self.bbox_embed, len(self.layers), self.config.d_model) if self.bbox_embed is not None else None
        mods = [self.layer_norm] + list(self.reference_points_head.layers) + [m for h in (heads or ()) for m in h.layers]
        return heads, [p for m in mods for p in m.parameters()]

    def native_decoder_reasons(self, inputs_embeds, vision_encoder_hidden_states, vision_encoder_attention_mask=None,
                               text_encoder_hidden_states=None, text_encoder_attention_mask=None, reference_points=None, spatial_shapes=None,
                               level_start_index=None, valid_ratios=None, self_attn_mask=None, output_attentions=False,
                               output_hidden_states=False):
        """Every reason why ``vllm_deform_decoder_forward`` does not serve this call, as a list of strings (empty: it does): training mode;
        something that requires grad under grad mode; ``output_attentions`` / ``output_hidden_states``; reference points that are not 4-d
        (2-d ones turn 4-d after the first refinement: that loop stays composed); non-bf16 parameters or inputs, or CPU tensors;
        ``query_scale``; a ``bbox_embed`` that is not None and not n_layers three-layer heads of width d_model; ``query_dim`` other than 4
        or d_model / 2 not a multiple of 16; and, prefixed with the layer's name, every reason a layer gives."""
        why = []
        x, mem, ref, vr = inputs_embeds, vision_encoder_hidden_states, reference_points, valid_ratios
        C, n_layers = self.config.d_model, len(self.layers)
        if self.training:
            why.append("training mode")
        if output_attentions:
            why.append("output_attentions: the attention weights stay inside the native call")
        if output_hidden_states:
            why.append("output_hidden_states: the un-normed hidden states stay inside the native call")
        if self.query_scale is not None:
            why.append("query_scale")
        heads, params = self._own_params()
        if self.bbox_embed is not None and heads is None:
            why.append(f"bbox_embed: None or {n_layers} three-layer heads of width d_model")
        if n_layers < 1 or self.config.query_dim != 4 or (C // 2) % 16 or C % 2:
            why.append("query_dim 4, d_model / 2 a multiple of 16, at least one layer")
        if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
            why.append("parameters: bf16 on the GPU")
        elif any(p.data_ptr() % 16 for p in params if p.numel() > 4) or any(p.data_ptr() % 16 for l in self.layers for p in l.parameters()):
            why.append("parameters: 16-byte aligned storage")
        if any(m.bias is None for m in self.reference_points_head.layers):
            why.append("parameters: a Linear without bias")
        if not (is_gpu_bf16(x) and is_gpu_bf16(mem)):
            why.append("inputs_embeds / vision_encoder_hidden_states: bf16 CUDA tensors [B, ., C]")
        if not (torch.is_tensor(ref) and ref.dim() == 3 and ref.shape[-1] == 4):
            why.append("reference_points: [B, Lq, 4] (2-d reference points keep the composed path)")
        elif not (ref.is_cuda and ref.dtype in (torch.float32, torch.bfloat16) and torch.is_tensor(x) and ref.shape[:2] == x.shape[:2]):
            why.append("reference_points: an fp32 or bf16 CUDA tensor [B, Lq, 4]")
        n_levels = getattr(self.layers[0].encoder_attn, "n_levels", 0) if n_layers else 0
        if not (torch.is_tensor(vr) and vr.is_cuda and vr.dtype in (torch.float32, torch.bfloat16) and torch.is_tensor(x) and
                tuple(vr.shape) == (x.shape[0], n_levels, 2)):
            why.append("valid_ratios: an fp32 or bf16 CUDA tensor [B, n_levels, 2]")
        if vision_encoder_attention_mask is not None and not (torch.is_tensor(vision_encoder_attention_mask) and
                                                              vision_encoder_attention_mask.dtype == torch.bool):
            why.append("vision_encoder_attention_mask: None or bool [B, S]")
        if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or
                                        any(torch.is_tensor(t) and t.requires_grad for t in (x, mem, ref, vr, text_encoder_hidden_states))):
            why.append("requires_grad under grad mode: there is no native backward")
        if torch.is_tensor(x) and x.dim() == 3 and torch.is_tensor(mem) and mem.dim() == 3 and torch.is_tensor(ref) and ref.dim() == 3:
            ref_in = ref[:, :, None].expand(-1, -1, max(n_levels, 1), -1)
            for i, layer in enumerate(self.layers):   # (query_pos has inputs_embeds' shape and dtype)
                why += [f"layers.{i}: {r}" for r in layer.native_layer_reasons(x, x, ref_in, mem, text_encoder_hidden_states,
                                                                                text_encoder_attention_mask, self_attn_mask, False)]
        return why

    def _native_state(self, device, heads, params):
        """descriptors of this module on ``device``: built once, rebuilt when a parameter's storage has moved"""
        sig = (tuple(p.data_ptr() for p in params), tuple(p.data_ptr() for l in self.layers for p in l.parameters()))
        cache = _NATIVE_STATE.setdefault(self, {})
        ent = cache.get(device)
        if ent is not None and ent[0] == sig:
            return ent[1]
        C, n = self.config.d_model, len(self.layers)
        keep = []
        descs = (_lib.VllmDeformDecLayerDesc * n)()
        for i, layer in enumerate(self.layers):
            _fill_layer_desc(descs[i], layer._parts(), C, 4, keep)
        d = _lib.VllmDeformDecoderDesc()
        d.n_layers, d.n_pos_feats = n, C // 2
        d.layer_norm_eps, d.inverse_sigmoid_eps = self.layer_norm.eps, 1e-5
        d.layers = descs
        l0, l1 = self.reference_points_head.layers
        dim_t = self._dim_t(C // 2, device).contiguous()
        d.ref_head_w0, d.ref_head_b0, d.ref_head_w1, d.ref_head_b1 = (t.data_ptr() for t in (l0.weight, l0.bias, l1.weight, l1.bias))
        d.layer_norm_w, d.layer_norm_b, d.dim_t = self.layer_norm.weight.data_ptr(), self.layer_norm.bias.data_ptr(), dim_t.data_ptr()
        boxes = None
        if heads is not None:
            boxes = (_lib.VllmBoxHead * n)()
            for i, h in enumerate(heads):
                (boxes[i].w0, boxes[i].b0, boxes[i].w1, boxes[i].b1, boxes[i].w2, boxes[i].b2) = (
                    t.data_ptr() for m in h.layers for t in (m.weight, m.bias))
            d.box_heads = boxes
        state = dict(desc=d, layers=descs, boxes=boxes, dim_t=dim_t, keep=keep)
        cache[device] = (sig, state)
        return state

    def _native_forward(self, x, mem, attention_mask, text, text_mask, reference_points, spatial_shapes, level_start_index, valid_ratios,
                        self_attn_mask):
        if level_pixels(spatial_shapes) != mem.shape[1]:   # the attention module's own check (...mask_dn.py:741)
            raise ValueError("Make sure to align the spatial shapes with the sequence length of the encoder hidden states")
        B, Lq, C = x.shape
        S, Lt, n = mem.shape[1], text.shape[1], len(self.layers)
        # (the decoder's reference points are [B, Lq, 4], one per query: the call multiplies them by valid_ratios itself)
        xa, _, mema, shapes, lsi, pmask = memory_operands("GroundingDinoDecoder", x, None, mem, spatial_shapes, level_start_index,
                                                          None if attention_mask is None else ~attention_mask, valid_ratios.shape[1])
        L = _lib.lib()
        heads, params = self._own_params()
        st = self._native_state(x.device, heads, params)
        geo = known_geometry(spatial_shapes, Lq)
        for ld in st["layers"]:
            ld.cross_attn.geometry = geo
        texta = _lib.aligned(text)
        ref = _lib.aligned(reference_points.to(torch.float32))
        vr = _lib.aligned(valid_ratios.to(torch.float32))
        sam, tmask = mask_u8(self_attn_mask, x.device), mask_u8(text_mask, x.device)
        ws, wsb = _lib.sized_workspace(x.device, L.vllm_deform_decoder_workspace_bytes(ctypes.byref(st["desc"]), B, Lq, Lt, S),
                                       "vllm_deform_decoder_workspace_bytes")
        inter = torch.empty((n, B, Lq, C), dtype=torch.bfloat16, device=x.device)
        irp = torch.empty((n, B, Lq, 4), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.vllm_deform_decoder_forward(ctypes.byref(st["desc"]), _lib.ptr(xa), _lib.ptr(ref), _lib.ptr(vr), _lib.ptr(sam),
                                                     _lib.ptr(texta), _lib.ptr(tmask), _lib.ptr(mema), _lib.ptr(pmask), _lib.ptr(shapes),
                                                     _lib.ptr(lsi), B, Lq, Lt, S, _lib.ptr(inter), _lib.ptr(irp), _lib.ptr(ws), wsb,
                                                     _lib.current_stream(x.device)),
                       "vllm_deform_decoder_forward")
        return inter[-1], inter.transpose(0, 1), irp.to(reference_points.dtype).transpose(0, 1)

    def forward(
        self,
        inputs_embeds,
        vision_encoder_hidden_states,
        mask_features,
        vision_encoder_attention_mask=None,
        text_encoder_hidden_states=None,
        text_encoder_attention_mask=None,
        reference_points=None,
        spatial_shapes=None,
        level_start_index=None,
        valid_ratios=None,
        self_attn_mask=None,
        output_attentions=None,
        output_hidden_states=None,
        return_dict=None,
    ):
        """The reference's ``forward`` (:1792-1981; ``mask_features`` is not read there either).  Returns the reference's tuple
        (last_hidden_state, intermediate_hidden_states, intermediate_reference_points[, hidden_states][, attentions]) or, with
        ``return_dict``, a GroundingDinoDecoderOutput.  On the native route the two stacked tensors are non-contiguous views (class
        docstring)."""
        output_attentions = output_attentions if output_attentions is not None else getattr(self.config, "output_attentions", False)
        output_hidden_states = (
            output_hidden_states if output_hidden_states is not None else getattr(self.config, "output_hidden_states", False)
        )
        return_dict = return_dict if return_dict is not None else getattr(self.config, "use_return_dict", True)

        if inputs_embeds is not None:
            hidden_states = inputs_embeds

        if self.native_decoder and not self.native_decoder_reasons(
                inputs_embeds, vision_encoder_hidden_states, vision_encoder_attention_mask, text_encoder_hidden_states,
                text_encoder_attention_mask, reference_points, spatial_shapes, level_start_index, valid_ratios, self_attn_mask,
                output_attentions, output_hidden_states):
            hidden_states, intermediate, intermediate_reference_points = self._native_forward(
                inputs_embeds, vision_encoder_hidden_states, vision_encoder_attention_mask, text_encoder_hidden_states,
                text_encoder_attention_mask, reference_points, spatial_shapes, level_start_index, valid_ratios, self_attn_mask)
            if not return_dict:
                return (hidden_states, intermediate, intermediate_reference_points)
            return GroundingDinoDecoderOutput(
                last_hidden_state=hidden_states,
                intermediate_hidden_states=intermediate,
                intermediate_reference_points=intermediate_reference_points,
                hidden_states=None,
                attentions=None,
            )

        # decoder layers
        all_hidden_states = () if output_hidden_states else None
        all_self_attns = () if output_attentions else None
        all_attns = () if output_attentions else None
        all_cross_attns_vision = () if (output_attentions and vision_encoder_hidden_states is not None) else None
        all_cross_attns_text = () if (output_attentions and text_encoder_hidden_states is not None) else None
        intermediate = ()
        intermediate_reference_points = ()

        for idx, decoder_layer in enumerate(self.layers):
            if reference_points.shape[-1] == 4:
                reference_points_input = (
                    reference_points[:, :, None] * torch.cat([valid_ratios, valid_ratios], -1)[:, None]
                )
            else:
                if reference_points.shape[-1] != 2:
                    raise ValueError("Reference points' last dimension must be of size 2")
                reference_points_input = reference_points[:, :, None] * valid_ratios[:, None]
            query_pos = self.get_proposal_pos_embed(reference_points_input[:, :, 0, :]).to(hidden_states.dtype)
            query_pos = self.reference_points_head(query_pos)

            # In original implementation they apply layer norm before outputting intermediate hidden states
            # Though that's not through between layers so the layers use as input the output of the previous layer
            # withtout layer norm
            if output_hidden_states:
                all_hidden_states += (self.layer_norm(hidden_states),)

            layer_outputs = decoder_layer(
                hidden_states=hidden_states,
                position_embeddings=query_pos,
                reference_points=reference_points_input,
                spatial_shapes=spatial_shapes,
                level_start_index=level_start_index,
                vision_encoder_hidden_states=vision_encoder_hidden_states,
                vision_encoder_attention_mask=vision_encoder_attention_mask,
                text_encoder_hidden_states=text_encoder_hidden_states,
                text_encoder_attention_mask=text_encoder_attention_mask,
                self_attn_mask=self_attn_mask,
                output_attentions=output_attentions,
            )

            hidden_states = layer_outputs[0]

            # hack implementation for iterative bounding box refinement
            if self.bbox_embed is not None:
                tmp = self.bbox_embed[idx](hidden_states)
                if reference_points.shape[-1] == 4:
                    new_reference_points = tmp + inverse_sigmoid(reference_points)
                    new_reference_points = new_reference_points.sigmoid()
                else:
                    if reference_points.shape[-1] != 2:
                        raise ValueError(
                            f"Reference points' last dimension must be of size 2, but is {reference_points.shape[-1]}"
                        )
                    new_reference_points = tmp
                    new_reference_points[..., :2] = tmp[..., :2] + inverse_sigmoid(reference_points)
                    new_reference_points = new_reference_points.sigmoid()
                reference_points = new_reference_points.detach()

            intermediate += (self.layer_norm(hidden_states),)
            intermediate_reference_points += (reference_points,)

            if output_attentions:
                all_self_attns += (layer_outputs[1],)

                if text_encoder_hidden_states is not None:
                    all_cross_attns_text += (layer_outputs[2],)

                if vision_encoder_hidden_states is not None:
                    all_cross_attns_vision += (layer_outputs[3],)

        # Keep batch_size as first dimension
        intermediate = torch.stack(intermediate, dim=1)
        intermediate_reference_points = torch.stack(intermediate_reference_points, dim=1)
        hidden_states = self.layer_norm(hidden_states)

        # add hidden states from the last decoder layer
        if output_hidden_states:
            all_hidden_states += (hidden_states,)

        if output_attentions:
            all_attns += (all_self_attns, all_cross_attns_text, all_cross_attns_vision)

        if not return_dict:
            return tuple(
                v
                for v in [
                    hidden_states,
                    intermediate,
                    intermediate_reference_points,
                    all_hidden_states,
                    all_attns,
                ]
                if v is not None
            )
        return GroundingDinoDecoderOutput(
            last_hidden_state=hidden_states,
            intermediate_hidden_states=intermediate,
            intermediate_reference_points=intermediate_reference_points,
            hidden_states=all_hidden_states,
            attentions=all_attns,
        )
