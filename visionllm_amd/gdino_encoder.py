"""The Grounding-DINO ENCODER: ``get_sine_pos_embed``, ``GroundingDinoTextEnhancerLayer``, ``GroundingDinoEncoderLayer`` and
``GroundingDinoEncoder`` of visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:787-857, :1185-1290, :1560-1722, under the
reference's constructor arguments and parameter names: the ``encoder.*`` slice of an ``OVGroundingDinoModel`` state-dict loads.  The
config is read by attribute; ``transformers`` is not needed.

The arrangement of the other mirrors, at two levels:

* ``GroundingDinoTextEnhancerLayer.native_layer = False`` (the default) runs the reference's statements; ``True`` makes a forward for
  which ``native_layer_reasons`` is empty ONE ``vllm_text_enhancer_forward`` (csrc/gdino_encoder.hip), and the weight slot is None.
* ``GroundingDinoEncoderLayer.forward`` is the reference's statements around its three members -- the package's
  ``GroundingDinoFusionLayer``, the enhancer and ``GroundingDinoDeformableLayer`` -- each of which honours its own switch.
* ``GroundingDinoEncoder.native_encoder = False`` (the default) runs the reference's loop; ``True`` makes a forward for which
  ``native_encoder_reasons`` is empty ONE ``vllm_gdino_encoder_forward`` for all layers (include/vllm_hip.h, section f2g).

One departure from the reference: the text position embedding that ``get_text_position_embeddings`` returns is cast to
``text_features.dtype`` (the reference builds it in fp32 and relies on autocast; without autocast a bf16 ``nn.MultiheadAttention`` fed an
fp32 query raises).  For fp32 and fp64 modules the cast changes no value.  Masks that are None are passed on as None where the reference
would fail on ``~None``.

THE MASK QUIRK.  ``GroundingDinoTextEnhancerLayer.forward`` turns a ``[B, Lt, Lt]`` mask into ``[H B, Lt, Lt]`` with
``attention_masks.repeat(self.num_heads, 1, 1)``, and ``nn.MultiheadAttention`` indexes a 3-d mask by ``b * H + h``: image ``b``, head
``h`` attends under the mask of image ``(b * H + h) % B``, not of image ``b`` (harmless for B = 1 or equal masks).  That is the
reference's behaviour; the composed statements keep it and the native routes reproduce it exactly (``n_masks = B``)."""
import ctypes
import dataclasses
import math
import weakref
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import _lib
from ._native_call import act2fn, fill_msda_desc, is_gpu_bf16, mask_u8, msda_params, native_act, opt_aligned, put
from .deformable_encoder import GroundingDinoDeformableLayer
from .fusion_layer import GroundingDinoFusionLayer
from .ms_deform_attn import known_geometry, level_pixels

HEAD_DIMS = (32, 64)   # vllm_mha_fwd_masks_bf16


def get_sine_pos_embed(
    pos_tensor: torch.Tensor,
    num_pos_feats: int = 128,
    temperature: int = 10000,
    exchange_xy: bool = True,
) -> Tensor:
    """generate sine position embedding from a position tensor (:1185-1214)
    Args:
        pos_tensor (torch.Tensor): shape: [..., n].
        num_pos_feats (int): projected shape for each float in the tensor.
        temperature (int): temperature in the sine/cosine function.
        exchange_xy (bool, optional): exchange pos x and pos y. \
            For example, input tensor is [x,y], the results will be [pos(y), pos(x)]. Defaults to True.
    Returns:
        pos_embed (torch.Tensor): shape: [..., n*num_pos_feats].
    """
    scale = 2 * math.pi
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos_tensor.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)

    def sine_func(x: torch.Tensor):
        sin_x = x * scale / dim_t
        sin_x = torch.stack((sin_x[..., 0::2].sin(), sin_x[..., 1::2].cos()), dim=3).flatten(2)
        return sin_x

    pos_res = [sine_func(x) for x in pos_tensor.split([1] * pos_tensor.shape[-1], dim=-1)]
    if exchange_xy:
        pos_res[0], pos_res[1] = pos_res[1], pos_res[0]
    pos_res = torch.cat(pos_res, dim=-1)
    return pos_res


def sine_dim_t(num_pos_feats, device, temperature=10000):
    """get_sine_pos_embed's own table (its first two statements), as the fp32 tensor the native calls read"""
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=device)
    return temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)


def _n_masks(mask, B, H, Lt):
    """slabs of an enhancer mask as the native call reads it: 1 for [Lt, Lt], B for [B, Lt, Lt] (the reference's repeat, module
    docstring), B H for [B H, Lt, Lt]; None for any other shape"""
    if mask.dim() == 2 and tuple(mask.shape) == (Lt, Lt):
        return 1
    if mask.dim() == 3 and tuple(mask.shape[1:]) == (Lt, Lt) and mask.shape[0] in (B, B * H):
        return int(mask.shape[0])
    return None


class GroundingDinoTextEnhancerLayer(nn.Module):
    """Vanilla Transformer with text embeddings as input (:787-857).  ``config`` needs ``d_model``, ``encoder_attention_heads``,
    ``encoder_ffn_dim``, ``text_enhancer_dropout`` and ``activation_function``.

    ``forward(hidden_states [B, Lt, C], attention_masks, position_embeddings)`` -> ``(hidden_states, attention_weights)``; the bool mask
    (True = may NOT attend) is [Lt, Lt], [B H, Lt, Lt] or [B, Lt, Lt], the last repeated as the reference repeats it (module docstring:
    the mask quirk).  With ``native_layer = True`` a call for which ``native_layer_reasons`` is empty is ONE
    ``vllm_text_enhancer_forward`` and returns ``(hidden_states, None)``: the ``[B, H, Lt, Lt]`` weights are never built.  A caller who
    needs them leaves the switch off."""

    native_layer = False   # True: bf16 inference runs vllm_text_enhancer_forward where native_layer_reasons() is empty

    def __init__(self, config):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(
            embed_dim=config.d_model,
            num_heads=config.encoder_attention_heads // 2,
            dropout=config.text_enhancer_dropout,
            batch_first=True,
        )
        # Implementation of Feedforward model
        self.fc1 = nn.Linear(config.d_model, config.encoder_ffn_dim // 2)
        self.fc2 = nn.Linear(config.encoder_ffn_dim // 2, config.d_model)

        self.layer_norm_before = nn.LayerNorm(config.d_model)
        self.layer_norm_after = nn.LayerNorm(config.d_model)

        self.activation = act2fn(config.activation_function)
        self.num_heads = config.encoder_attention_heads // 2
        self.dropout = config.text_enhancer_dropout

    def with_pos_embed(self, hidden_state: Tensor, position_embeddings: Optional[Tensor]):
        return hidden_state if position_embeddings is None else hidden_state + position_embeddings

    def native_layer_reasons(self, hidden_states, attention_masks=None, position_embeddings=None):
        """why this call keeps the composed path, as a list of strings (empty: the native call serves it)"""
        why = []
        x, pos, mha = hidden_states, position_embeddings, self.self_attn
        if self.training:
            why.append("training mode")
        params = list(self.parameters())
        if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
            why.append("parameters: bf16 on the GPU")
        if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or any(torch.is_tensor(v) and v.requires_grad for v in (x, pos))):
            why.append("requires_grad under grad mode: there is no native backward")
        if not getattr(mha, "_qkv_same_embed_dim", False) or mha.in_proj_weight is None:
            why.append("self_attn: separate q / k / v projection weights")
        elif mha.in_proj_bias is None or mha.out_proj.bias is None:
            why.append("self_attn: no bias")
        if mha.bias_k is not None or mha.bias_v is not None or mha.add_zero_attn:
            why.append("self_attn: bias_k / add_zero_attn")
        C, F = mha.embed_dim, self.fc1.out_features
        if mha.head_dim not in HEAD_DIMS:
            why.append(f"self_attn: head dim {mha.head_dim} (32 or 64)")
        if not (C % 64 == 0 and 64 <= C <= 512 and F % 64 == 0):
            why.append("d_model a multiple of 64 in 64 .. 512, d_ffn a multiple of 64")
        if native_act(self.activation) is None:
            why.append("activation: relu or gelu")
        if not is_gpu_bf16(x):
            why.append("hidden_states: a bf16 CUDA tensor [B, Lt, d_model]")
        if pos is not None and not (is_gpu_bf16(pos) and torch.is_tensor(x) and pos.shape == x.shape):
            why.append("position_embeddings: None or a bf16 CUDA tensor of hidden_states' shape")
        if not (torch.is_tensor(x) and x.dim() == 3):
            return why
        if x.stride(-1) != 1 or (torch.is_tensor(pos) and pos.dim() == 3 and pos.stride(-1) != 1):
            why.append("hidden_states / position_embeddings: a contiguous last dim")
        B, Lt, Cx = x.shape
        if Cx != C or B * Lt * max(F, 2 * C) * 2 >= 2 ** 31:
            why.append("shapes: [B, Lt, d_model], B Lt rows of the widest intermediate under 2^31 bytes")
        m = attention_masks
        if m is not None and not (torch.is_tensor(m) and m.dtype == torch.bool and _n_masks(m, B, self.num_heads, Lt) is not None):
            why.append("attention_masks: None or bool [Lt, Lt], [B, Lt, Lt] or [B H, Lt, Lt] (a float mask keeps the composed path)")
        return why

    def native_layer_applies(self, hidden_states, attention_masks=None, position_embeddings=None):
        return not self.native_layer_reasons(hidden_states, attention_masks, position_embeddings)

    def _fill_desc(self, keep):
        mha = self.self_attn
        d = _lib.VllmTextEnhancerDesc()
        d.d_model, d.n_heads, d.d_ffn, d.act = mha.embed_dim, mha.num_heads, self.fc1.out_features, native_act(self.activation)
        d.norm_before_eps, d.norm_after_eps = self.layer_norm_before.eps, self.layer_norm_after.eps
        put(d, keep, "in_proj", mha.in_proj_weight, mha.in_proj_bias)   # the packed parameter: the call slices it by pointer offset
        put(d, keep, "out_proj", mha.out_proj.weight, mha.out_proj.bias)
        for name, mod in (("norm_before", self.layer_norm_before), ("fc1", self.fc1), ("fc2", self.fc2), ("norm_after", self.layer_norm_after)):
            put(d, keep, name, mod.weight, mod.bias)
        return d

    def _native_forward(self, hidden_states, attention_masks=None, position_embeddings=None):
        B, Lt, C = hidden_states.shape
        L = _lib.lib()
        dev = hidden_states.device
        keep = []
        d = self._fill_desc(keep)
        x, pos = _lib.aligned(hidden_states), opt_aligned(position_embeddings)
        mask = mask_u8(attention_masks, dev)
        n_masks = 1 if attention_masks is None else _n_masks(attention_masks, B, self.num_heads, Lt)
        out = torch.empty((B, Lt, C), dtype=torch.bfloat16, device=dev)
        ws, wsb = _lib.sized_workspace(dev, L.vllm_text_enhancer_workspace_bytes(ctypes.byref(d), B, Lt), "vllm_text_enhancer_workspace_bytes")
        with torch.cuda.device(dev):
            _lib.check(L.vllm_text_enhancer_forward(ctypes.byref(d), _lib.ptr(x), _lib.ptr(pos), _lib.ptr(mask), n_masks, B, Lt, _lib.ptr(out),
                                                    _lib.ptr(ws), wsb, _lib.current_stream(dev)), "vllm_text_enhancer_forward")
        del keep
        return out, None

    def forward(
        self,
        hidden_states: torch.FloatTensor,
        attention_masks: Optional[torch.BoolTensor] = None,
        position_embeddings: Optional[torch.FloatTensor] = None,
    ) -> Tuple[torch.FloatTensor, torch.FloatTensor]:
        """Text self-attention to enhance projection of text features generated by the text encoder within
        GroundingDinoEncoderLayer (:812-857) -> (hidden_states [B, Lt, C], attention_weights [B, H, Lt, Lt])."""
        if self.native_layer and self.native_layer_applies(hidden_states, attention_masks, position_embeddings):
            return self._native_forward(hidden_states, attention_masks, position_embeddings)

        # repeat attn mask
        if attention_masks is not None and attention_masks.dim() == 3 and attention_masks.shape[0] == hidden_states.shape[0]:
            # bs, num_q, num_k
            attention_masks = attention_masks.repeat(self.num_heads, 1, 1)

        queries = keys = self.with_pos_embed(hidden_states, position_embeddings)
        attention_output, attention_weights = self.self_attn(
            query=queries, key=keys, value=hidden_states, attn_mask=attention_masks, average_attn_weights=False
        )
        attention_output = nn.functional.dropout(attention_output, p=self.dropout, training=self.training)
        hidden_states = hidden_states + attention_output
        hidden_states = self.layer_norm_before(hidden_states)

        residual = hidden_states
        hidden_states = self.activation(self.fc1(hidden_states))
        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = self.fc2(hidden_states)
        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        hidden_states = hidden_states + residual
        hidden_states = self.layer_norm_after(hidden_states)

        return hidden_states, attention_weights


class GroundingDinoEncoderLayer(nn.Module):
    """One encoder layer (:1217-1290): fusion layer, text enhancer, deformable layer.  ``config`` needs what the three members need."""

    def __init__(self, config) -> None:
        super().__init__()

        self.d_model = config.d_model

        self.text_enhancer_layer = GroundingDinoTextEnhancerLayer(config)
        self.fusion_layer = GroundingDinoFusionLayer(config)
        self.deformable_layer = GroundingDinoDeformableLayer(config)

    def get_text_position_embeddings(
        self, text_features: Tensor, text_position_embedding: Tensor, text_position_ids: Tensor
    ) -> Tensor:
        batch_size, seq_length, _ = text_features.shape
        if text_position_embedding is None and text_position_ids is None:
            text_position_embedding = torch.arange(seq_length, device=text_features.device)
            text_position_embedding = text_position_embedding.float()
            text_position_embedding = text_position_embedding.unsqueeze(0).unsqueeze(-1)
            text_position_embedding = text_position_embedding.repeat(batch_size, 1, 1)
            text_position_embedding = get_sine_pos_embed(
                text_position_embedding, num_pos_feats=self.d_model, exchange_xy=False
            )
        if text_position_ids is not None:
            text_position_embedding = get_sine_pos_embed(
                text_position_ids[..., None], num_pos_feats=self.d_model, exchange_xy=False
            )

        return text_position_embedding

    def forward(
        self,
        vision_features: Tensor,
        vision_position_embedding: Tensor,
        spatial_shapes: Tensor,
        level_start_index: Tensor,
        key_padding_mask: Tensor,
        reference_points: Tensor,
        text_features: Optional[Tensor] = None,
        text_attention_mask: Optional[Tensor] = None,
        text_position_embedding: Optional[Tensor] = None,
        text_self_attention_masks: Optional[Tensor] = None,
        text_position_ids: Optional[Tensor] = None,
    ):
        # (the stated departure: the reference's cast is to vision_features.dtype under autocast; module docstring)
        text_position_embedding = self.get_text_position_embeddings(
            text_features, text_position_embedding, text_position_ids
        ).to(text_features.dtype)

        (vision_features, vision_fused_attn), (text_features, text_fused_attn) = self.fusion_layer(
            vision_features=vision_features,
            text_features=text_features,
            attention_mask_vision=key_padding_mask,
            attention_mask_text=text_attention_mask,
        )

        (text_features, text_enhanced_attn) = self.text_enhancer_layer(
            hidden_states=text_features,
            attention_masks=None if text_self_attention_masks is None else ~text_self_attention_masks,  # note we use ~ for mask here
            position_embeddings=(text_position_embedding if text_position_embedding is not None else None),
        )

        (vision_features, vision_deformable_attn) = self.deformable_layer(
            hidden_states=vision_features,
            attention_mask=None if key_padding_mask is None else ~key_padding_mask,
            position_embeddings=vision_position_embedding,
            reference_points=reference_points,
            spatial_shapes=spatial_shapes,
            level_start_index=level_start_index,
        )

        return (
            (vision_features, text_features),
            (vision_fused_attn, text_fused_attn, text_enhanced_attn, vision_deformable_attn),
        )


@dataclasses.dataclass
class GroundingDinoEncoderOutput:
    """The fields of the reference's ModelOutput of the same name, as a plain dataclass."""
    last_hidden_state_vision: torch.Tensor = None
    last_hidden_state_text: torch.Tensor = None
    hidden_states_vision: tuple = None
    hidden_states_text: tuple = None
    attentions: tuple = None


def _fill_deformable_desc(desc, layer, keep):
    """``desc`` (a VllmDeformEncLayerDesc) from a GroundingDinoDeformableLayer, everything but ``attn.geometry``"""
    attn = layer.self_attn
    desc.d_ffn, desc.act = layer.fc1.out_features, native_act(layer.activation_fn)
    desc.norm1_eps, desc.norm2_eps = layer.self_attn_layer_norm.eps, layer.final_layer_norm.eps
    fill_msda_desc(desc.attn, keep, layer.embed_dim, attn.n_heads, attn.n_levels, attn.n_points, 2, False, msda_params(attn))
    for name, mod in (("norm1", layer.self_attn_layer_norm), ("fc1", layer.fc1), ("fc2", layer.fc2), ("norm2", layer.final_layer_norm)):
        put(desc, keep, name, mod.weight, mod.bias)


_NATIVE_STATE = weakref.WeakKeyDictionary()   # GroundingDinoEncoder -> {device: (signature, descriptors and what they point to)}


class GroundingDinoEncoder(nn.Module):
    """The Grounding-DINO encoder (:1560-1722): parameter names ``layers.N.{text_enhancer_layer,fusion_layer,deformable_layer}.*``.
    ``config`` needs what GroundingDinoEncoderLayer needs, and ``encoder_layers`` and ``dropout``; ``output_attentions``,
    ``output_hidden_states`` and ``use_return_dict`` are read where ``forward`` is not told (defaults False, False, True).

    With the class attribute ``native_encoder = False`` (the default) ``forward`` is the reference's statements and every member honours
    its own ``native_layer``.  With ``native_encoder = True`` a call for which ``native_encoder_reasons`` is empty is ONE
    ``vllm_gdino_encoder_forward`` (csrc/gdino_encoder.hip): the reference points and the text position embedding once, then per layer
    the launches of the three members' native calls.  Descriptors and the ``dim_t`` table are remembered per device (and rebuilt when a
    parameter's storage changes); no weight is copied.  ``valid_ratios`` may be fp32 or bf16 (widened once)."""

    native_encoder = False   # True: bf16 inference runs vllm_gdino_encoder_forward where native_encoder_reasons() is empty

    def __init__(self, config):
        super().__init__()
        self.config = config

        self.dropout = config.dropout
        self.layers = nn.ModuleList([GroundingDinoEncoderLayer(config) for _ in range(config.encoder_layers)])

    @staticmethod
    def get_reference_points(spatial_shapes, valid_ratios, device):
        """
        Get reference points for each feature map. Used in decoder.
        Args:
            spatial_shapes (`torch.LongTensor` of shape `(num_feature_levels, 2)`):
                Spatial shapes of each feature map.
            valid_ratios (`torch.FloatTensor` of shape `(batch_size, num_feature_levels, 2)`):
                Valid ratios of each feature map.
            device (`torch.device`):
                Device on which to create the tensors.
        Returns:
            `torch.FloatTensor` of shape `(batch_size, num_queries, num_feature_levels, 2)`
        """
        reference_points_list = []
        for level, (height, width) in enumerate(spatial_shapes):
            ref_y, ref_x = torch.meshgrid(
                torch.linspace(0.5, height - 0.5, height, dtype=torch.float32, device=device),
                torch.linspace(0.5, width - 0.5, width, dtype=torch.float32, device=device),
                indexing="ij",
            )
            # TODO: valid_ratios could be useless here. check https://github.com/fundamentalvision/Deformable-DETR/issues/36
            ref_y = ref_y.reshape(-1)[None] / (valid_ratios[:, None, level, 1] * height)
            ref_x = ref_x.reshape(-1)[None] / (valid_ratios[:, None, level, 0] * width)
            ref = torch.stack((ref_x, ref_y), -1)
            reference_points_list.append(ref)
        reference_points = torch.cat(reference_points_list, 1)
        reference_points = reference_points[:, :, None] * valid_ratios[:, None]
        return reference_points

    def native_encoder_reasons(self, vision_features, vision_attention_mask=None, vision_position_embedding=None, spatial_shapes=None,
                               level_start_index=None, valid_ratios=None, text_features=None, text_attention_mask=None,
                               text_position_embedding=None, text_self_attention_masks=None, text_position_ids=None,
                               output_attentions=False, output_hidden_states=False):
        """Every reason why ``vllm_gdino_encoder_forward`` does not serve this call, as a list of strings (empty: it does): training mode;
        ``output_attentions`` / ``output_hidden_states``; a missing ``text_self_attention_masks``; ``valid_ratios`` that is not an fp32
        or bf16 CUDA tensor [B, n_levels, 2]; a text position embedding or position ids of another kind than the call takes; parameters
        whose storage is not 16-byte aligned; and, prefixed ``layers.N.<member>:``, every reason a member gives."""
        why = []
        x, t, vr = vision_features, text_features, valid_ratios
        n_layers = len(self.layers)
        if self.training:
            why.append("training mode")
        if output_attentions:
            why.append("output_attentions: the attention weights stay inside the native call")
        if output_hidden_states:
            why.append("output_hidden_states: the hidden states between two layers stay inside the native call")
        if n_layers < 1:
            why.append("at least one layer")
        if text_self_attention_masks is None:
            why.append("text_self_attention_masks: missing")
        if not (is_gpu_bf16(x) and is_gpu_bf16(t) and x.shape[0] == t.shape[0]):
            why.append("vision_features / text_features: bf16 CUDA tensors [B, ., d_model] of one batch")
            return why
        if not (is_gpu_bf16(vision_position_embedding) and vision_position_embedding.shape == x.shape):
            why.append("vision_position_embedding: a bf16 CUDA tensor of vision_features' shape")
        B, Lt = t.shape[0], t.shape[1]
        n_levels = getattr(self.layers[0].deformable_layer.self_attn, "n_levels", 0) if n_layers else 0
        if not (torch.is_tensor(vr) and vr.is_cuda and vr.dtype in (torch.float32, torch.bfloat16) and tuple(vr.shape) == (B, n_levels, 2)):
            why.append("valid_ratios: an fp32 or bf16 CUDA tensor [B, n_levels, 2]")
            return why
        if torch.is_grad_enabled() and vr.requires_grad:
            why.append("requires_grad under grad mode: there is no native backward")
        if not (torch.is_tensor(spatial_shapes) and tuple(spatial_shapes.shape) == (n_levels, 2) and torch.is_tensor(level_start_index) and
                level_start_index.numel() == n_levels):
            why.append("spatial_shapes [n_levels, 2] / level_start_index [n_levels]")
        ids, emb = text_position_ids, text_position_embedding
        if ids is not None and not (torch.is_tensor(ids) and ids.is_cuda and tuple(ids.shape) == (B, Lt)):
            why.append("text_position_ids: None or a CUDA tensor [B, Lt]")
        if ids is None and emb is not None and not (is_gpu_bf16(emb) and emb.shape == t.shape):
            why.append("text_position_embedding: None or a bf16 CUDA tensor of text_features' shape")
        if any(p.is_cuda and p.data_ptr() % 16 for p in self.parameters()):
            why.append("parameters: 16-byte aligned storage")
        masks = text_self_attention_masks
        for i, layer in enumerate(self.layers):   # (the position embeddings have the features' shapes and dtype)
            for member, reasons in (
                    ("fusion_layer", layer.fusion_layer.native_layer_reasons(x, t, vision_attention_mask, text_attention_mask)),
                    ("text_enhancer_layer", layer.text_enhancer_layer.native_layer_reasons(t, masks, t)),
                    ("deformable_layer", layer.deformable_layer.native_layer_reasons(x, vision_position_embedding, vr))):
                why += [f"layers.{i}.{member}: {r}" for r in reasons]
        return why

    def _native_state(self, device):
        """descriptors of this module on ``device``: built once, rebuilt when a parameter's storage has moved"""
        sig = tuple(p.data_ptr() for p in self.parameters())
        cache = _NATIVE_STATE.setdefault(self, {})
        ent = cache.get(device)
        if ent is not None and ent[0] == sig:
            return ent[1]
        n = len(self.layers)
        keep = []
        fusion, enhancer, deformable = (_lib.VllmFusionLayerDesc * n)(), (_lib.VllmTextEnhancerDesc * n)(), (_lib.VllmDeformEncLayerDesc * n)()
        for i, layer in enumerate(self.layers):
            fusion[i] = layer.fusion_layer._fill_desc(keep)
            enhancer[i] = layer.text_enhancer_layer._fill_desc(keep)
            _fill_deformable_desc(deformable[i], layer.deformable_layer, keep)
        dim_t = sine_dim_t(self.layers[0].d_model, device).contiguous()
        d = _lib.VllmGdinoEncoderDesc()
        d.n_layers, d.reserved = n, 0
        d.fusion, d.enhancer, d.deformable, d.dim_t = fusion, enhancer, deformable, dim_t.data_ptr()
        state = dict(desc=d, fusion=fusion, enhancer=enhancer, deformable=deformable, dim_t=dim_t, keep=keep)
        cache[device] = (sig, state)
        return state

    def _native_forward(self, vision_features, vision_attention_mask, vision_position_embedding, spatial_shapes, level_start_index, valid_ratios,
                        text_features, text_attention_mask, text_position_embedding, text_self_attention_masks, text_position_ids):
        B, S, C = vision_features.shape
        Lt = text_features.shape[1]
        if level_pixels(spatial_shapes) != S:   # the attention module's own check (...mask_dn.py:741)
            raise ValueError("Make sure to align the spatial shapes with the sequence length of the encoder hidden states")
        dev = vision_features.device
        L = _lib.lib()
        st = self._native_state(dev)
        geo = known_geometry(spatial_shapes, S)
        for ld in st["deformable"]:
            ld.attn.geometry = geo
        x, xpos, t = _lib.aligned(vision_features), _lib.aligned(vision_position_embedding), _lib.aligned(text_features)
        vr = _lib.aligned(valid_ratios.to(torch.float32))
        shapes = spatial_shapes.to(device=dev, dtype=torch.int64).contiguous()
        lsi = level_start_index.to(device=dev, dtype=torch.int64).contiguous()
        vmask, tmask = mask_u8(vision_attention_mask, dev), mask_u8(text_attention_mask, dev)
        # the reference's `~` (:1273), once per call instead of once per layer
        inv = ~text_self_attention_masks
        n_masks = _n_masks(inv, B, self.layers[0].text_enhancer_layer.num_heads, Lt)
        sam = mask_u8(inv, dev)
        # the reference's precedence (:1231-1242): position ids, else the caller's embedding, else 0 .. Lt - 1
        positions = emb = None
        if text_position_ids is not None:
            positions = text_position_ids.to(torch.float32).contiguous()
        elif text_position_embedding is not None:
            emb = _lib.aligned(text_position_embedding)
        out_v, out_t = torch.empty((B, S, C), dtype=torch.bfloat16, device=dev), torch.empty((B, Lt, C), dtype=torch.bfloat16, device=dev)
        ws, wsb = _lib.sized_workspace(dev, L.vllm_gdino_encoder_workspace_bytes(ctypes.byref(st["desc"]), B, S, Lt),
                                       "vllm_gdino_encoder_workspace_bytes")
        with torch.cuda.device(dev):
            _lib.check(L.vllm_gdino_encoder_forward(ctypes.byref(st["desc"]), _lib.ptr(x), _lib.ptr(xpos), _lib.ptr(vmask), _lib.ptr(vr),
                                                    _lib.ptr(shapes), _lib.ptr(lsi), _lib.ptr(t), _lib.ptr(tmask), _lib.ptr(sam), n_masks,
                                                    _lib.ptr(positions), _lib.ptr(emb), B, S, Lt, _lib.ptr(out_v), _lib.ptr(out_t),
                                                    _lib.ptr(ws), wsb, _lib.current_stream(dev)), "vllm_gdino_encoder_forward")
        return out_v, out_t

    def forward(
        self,
        vision_features: Tensor,
        vision_attention_mask: Tensor,
        vision_position_embedding: Tensor,
        spatial_shapes: Tensor,
        level_start_index: Tensor,
        valid_ratios=None,
        text_features: Optional[Tensor] = None,
        text_attention_mask: Optional[Tensor] = None,
        text_position_embedding: Optional[Tensor] = None,
        text_self_attention_masks: Optional[Tensor] = None,
        text_position_ids: Optional[Tensor] = None,
        output_attentions=None,
        output_hidden_states=None,
        return_dict=None,
    ):
        """The reference's ``forward`` (:1608-1722): vision_features / vision_position_embedding [B, S, C]; vision_attention_mask [B, S]
        and text_attention_mask [B, Lt], True = padding; text_self_attention_masks [B, Lt, Lt], True = may attend (it is inverted for
        the enhancer).  Returns the reference's tuple (vision, text[, hidden states][, attentions]) or, with ``return_dict``, a
        GroundingDinoEncoderOutput."""
        output_attentions = output_attentions if output_attentions is not None else getattr(self.config, "output_attentions", False)
        output_hidden_states = (
            output_hidden_states if output_hidden_states is not None else getattr(self.config, "output_hidden_states", False)
        )
        return_dict = return_dict if return_dict is not None else getattr(self.config, "use_return_dict", True)

        if self.native_encoder and not self.native_encoder_reasons(
                vision_features, vision_attention_mask, vision_position_embedding, spatial_shapes, level_start_index, valid_ratios,
                text_features, text_attention_mask, text_position_embedding, text_self_attention_masks, text_position_ids, output_attentions,
                output_hidden_states):
            vision_features, text_features = self._native_forward(
                vision_features, vision_attention_mask, vision_position_embedding, spatial_shapes, level_start_index, valid_ratios,
                text_features, text_attention_mask, text_position_embedding, text_self_attention_masks, text_position_ids)
            if not return_dict:
                return (vision_features, text_features)
            return GroundingDinoEncoderOutput(last_hidden_state_vision=vision_features, last_hidden_state_text=text_features,
                                              hidden_states_vision=None, hidden_states_text=None, attentions=None)

        reference_points = self.get_reference_points(spatial_shapes, valid_ratios, device=vision_features.device)

        encoder_vision_states = () if output_hidden_states else None
        encoder_text_states = () if output_hidden_states else None
        all_attns = () if output_attentions else None
        all_attn_fused_text = () if output_attentions else None
        all_attn_fused_vision = () if output_attentions else None
        all_attn_enhanced_text = () if output_attentions else None
        all_attn_deformable = () if output_attentions else None
        for i, encoder_layer in enumerate(self.layers):
            if output_hidden_states:
                encoder_vision_states += (vision_features,)
                encoder_text_states += (text_features,)

            (vision_features, text_features), attentions = encoder_layer(
                vision_features=vision_features,
                vision_position_embedding=vision_position_embedding,
                spatial_shapes=spatial_shapes,
                level_start_index=level_start_index,
                key_padding_mask=vision_attention_mask,
                reference_points=reference_points,
                text_features=text_features,
                text_attention_mask=text_attention_mask,
                text_position_embedding=text_position_embedding,
                text_self_attention_masks=text_self_attention_masks,
                text_position_ids=text_position_ids,
            )

            if output_attentions:
                all_attn_fused_vision += (attentions[0],)
                all_attn_fused_text += (attentions[1],)
                all_attn_enhanced_text += (attentions[2],)
                all_attn_deformable += (attentions[3],)

        if output_hidden_states:
            encoder_vision_states += (vision_features,)
            encoder_text_states += (text_features,)

        if output_attentions:
            all_attns = (all_attn_fused_vision, all_attn_fused_text, all_attn_enhanced_text, all_attn_deformable)

        if not return_dict:
            enc_outputs = [vision_features, text_features, encoder_vision_states, encoder_text_states, all_attns]
            return tuple(v for v in enc_outputs if v is not None)
        return GroundingDinoEncoderOutput(
            last_hidden_state_vision=vision_features,
            last_hidden_state_text=text_features,
            hidden_states_vision=encoder_vision_states,
            hidden_states_text=encoder_text_states,
            attentions=all_attns,
        )
