"""The fusion layer of Grounding-DINO, which ``GroundingDinoEncoderLayer`` runs in front of every deformable encoder layer
(deformable_encoder.py): ``GroundingDinoDropPath``, ``GroundingDinoBiMultiHeadAttention`` and ``GroundingDinoFusionLayer`` of
visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:860-1101 (modeling_grounding_dino.py has the same classes), under
the reference's constructor arguments and parameter names: the matching slice of an ``OVGroundingDinoModel`` state-dict loads.

``GroundingDinoFusionLayer`` follows the arrangement of the other mirrors: ``native_layer = False`` (the default) runs the reference's
statements; ``native_layer = True`` makes a forward for which ``native_layer_reasons`` is empty ONE ``vllm_fusion_layer_forward``
(csrc/fusion_layer.cpp, csrc/xattn.hip; include/vllm_hip.h section f2f, which also states where the exact masked softmax of the native
call departs from the reference's clamped one)."""
import ctypes
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._native_call import is_gpu_bf16, mask_u8, opt_aligned, put

HEAD_DIMS = (128, 256)   # vllm_xattn_fwd_bf16


class GroundingDinoBiMultiHeadAttention(nn.Module):
    def __init__(self, config):
        super().__init__()

        vision_dim = text_dim = config.d_model
        embed_dim = config.encoder_ffn_dim // 2
        num_heads = config.encoder_attention_heads // 2
        dropout = config.fusion_dropout

        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.vision_dim = vision_dim
        self.text_dim = text_dim

        if self.head_dim * self.num_heads != self.embed_dim:
            raise ValueError(
                f"`embed_dim` must be divisible by `num_heads` (got `embed_dim`: {self.embed_dim} and `num_heads`: {self.num_heads})."
            )
        self.scale = self.head_dim ** (-0.5)
        self.dropout = dropout

        self.vision_proj = nn.Linear(self.vision_dim, self.embed_dim)
        self.text_proj = nn.Linear(self.text_dim, self.embed_dim)
        self.values_vision_proj = nn.Linear(self.vision_dim, self.embed_dim)
        self.values_text_proj = nn.Linear(self.text_dim, self.embed_dim)

        self.out_vision_proj = nn.Linear(self.embed_dim, self.vision_dim)
        self.out_text_proj = nn.Linear(self.embed_dim, self.text_dim)

    def _shape(self, tensor: torch.Tensor, seq_len: int, batch_size: int):
        return tensor.view(batch_size, seq_len, self.num_heads, self.head_dim).transpose(1, 2).contiguous()

    def forward(
        self,
        vision_features: torch.FloatTensor,
        text_features: torch.FloatTensor,
        vision_attention_mask: Optional[torch.BoolTensor] = None,
        text_attention_mask: Optional[torch.BoolTensor] = None,
    ) -> Tuple[Tuple[torch.FloatTensor, torch.FloatTensor], Tuple[torch.FloatTensor, torch.FloatTensor]]:
        """Image-to-text and text-to-image cross-attention (:893-1006) -> ((vision_attn_output, vision_attn_weights),
        (text_attn_output, text_attn_weights)); the masks are True at padding tokens."""
        batch_size, tgt_len, _ = vision_features.size()

        vision_query_states = self.vision_proj(vision_features) * self.scale
        vision_query_states = self._shape(vision_query_states, tgt_len, batch_size)

        text_key_states = self.text_proj(text_features)
        text_key_states = self._shape(text_key_states, -1, batch_size)

        vision_value_states = self.values_vision_proj(vision_features)
        vision_value_states = self._shape(vision_value_states, -1, batch_size)

        text_value_states = self.values_text_proj(text_features)
        text_value_states = self._shape(text_value_states, -1, batch_size)

        proj_shape = (batch_size * self.num_heads, -1, self.head_dim)

        vision_query_states = vision_query_states.view(*proj_shape)
        text_key_states = text_key_states.view(*proj_shape)
        vision_value_states = vision_value_states.view(*proj_shape)
        text_value_states = text_value_states.view(*proj_shape)

        src_len = text_key_states.size(1)
        attn_weights = torch.bmm(vision_query_states, text_key_states.transpose(1, 2))  # bs*nhead, nimg, ntxt

        if attn_weights.size() != (batch_size * self.num_heads, tgt_len, src_len):
            raise ValueError(
                f"Attention weights should be of size {(batch_size * self.num_heads, tgt_len, src_len)}, but is {attn_weights.size()}"
            )

        attn_weights = attn_weights - attn_weights.max()
        # Do not increase -50000/50000, data type half has quite limited range
        attn_weights = torch.clamp(attn_weights, min=-50000, max=50000)

        attn_weights_transposed = attn_weights.transpose(1, 2)
        text_attn_weights = attn_weights_transposed - torch.max(attn_weights_transposed, dim=-1, keepdim=True)[0]

        # Do not increase -50000/50000, data type half has quite limited range
        text_attn_weights = torch.clamp(text_attn_weights, min=-50000, max=50000)

        # mask vision for language
        if vision_attention_mask is not None:
            vision_attention_mask = (
                vision_attention_mask[:, None, None, :].repeat(1, self.num_heads, 1, 1).flatten(0, 1)
            )
            text_attn_weights.masked_fill_(vision_attention_mask, float("-inf"))

        text_attn_weights = text_attn_weights.softmax(dim=-1)

        # mask language for vision
        if text_attention_mask is not None:
            text_attention_mask = text_attention_mask[:, None, None, :].repeat(1, self.num_heads, 1, 1).flatten(0, 1)
            attn_weights.masked_fill_(text_attention_mask, float("-inf"))
        vision_attn_weights = attn_weights.softmax(dim=-1)

        vision_attn_probs = F.dropout(vision_attn_weights, p=self.dropout, training=self.training)
        text_attn_probs = F.dropout(text_attn_weights, p=self.dropout, training=self.training)

        vision_attn_output = torch.bmm(vision_attn_probs, text_value_states)
        text_attn_output = torch.bmm(text_attn_probs, vision_value_states)

        if vision_attn_output.size() != (batch_size * self.num_heads, tgt_len, self.head_dim):
            raise ValueError(
                f"`vision_attn_output` should be of size {(batch_size, self.num_heads, tgt_len, self.head_dim)}, but is {vision_attn_output.size()}"
            )

        if text_attn_output.size() != (batch_size * self.num_heads, src_len, self.head_dim):
            raise ValueError(
                f"`text_attn_output` should be of size {(batch_size, self.num_heads, src_len, self.head_dim)}, but is {text_attn_output.size()}"
            )

        vision_attn_output = vision_attn_output.view(batch_size, self.num_heads, tgt_len, self.head_dim)
        vision_attn_output = vision_attn_output.transpose(1, 2)
        vision_attn_output = vision_attn_output.reshape(batch_size, tgt_len, self.embed_dim)

        text_attn_output = text_attn_output.view(batch_size, self.num_heads, src_len, self.head_dim)
        text_attn_output = text_attn_output.transpose(1, 2)
        text_attn_output = text_attn_output.reshape(batch_size, src_len, self.embed_dim)

        vision_attn_output = self.out_vision_proj(vision_attn_output)
        text_attn_output = self.out_text_proj(text_attn_output)

        return (vision_attn_output, vision_attn_weights), (text_attn_output, text_attn_weights)


def drop_path(input: torch.Tensor, drop_prob: float = 0.0, training: bool = False) -> torch.Tensor:
    """Stochastic depth per sample (:1010-1026)"""
    if drop_prob == 0.0 or not training:
        return input
    keep_prob = 1 - drop_prob
    shape = (input.shape[0],) + (1,) * (input.ndim - 1)  # work with diff dim tensors, not just 2D ConvNets
    random_tensor = keep_prob + torch.rand(shape, dtype=input.dtype, device=input.device)
    random_tensor.floor_()  # binarize
    output = input.div(keep_prob) * random_tensor
    return output


class GroundingDinoDropPath(nn.Module):
    """Drop paths (Stochastic Depth) per sample (when applied in main path of residual blocks)."""

    def __init__(self, drop_prob: Optional[float] = None) -> None:
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return drop_path(hidden_states, self.drop_prob, self.training)

    def extra_repr(self) -> str:
        return "p={}".format(self.drop_prob)


class GroundingDinoFusionLayer(nn.Module):
    """``config`` needs ``d_model``, ``encoder_ffn_dim``, ``encoder_attention_heads``, ``fusion_dropout`` and ``fusion_droppath``.

    ``forward(vision_features [B, S, C], text_features [B, Lt, C], attention_mask_vision, attention_mask_text)`` with bool masks [B, S] /
    [B, Lt], True = a padding token, -> ``((vision_features, vision_attn_weights), (text_features, text_attn_weights))``.

    With ``native_layer = False`` (the default) it is the reference's statements.  With ``native_layer = True`` a call for which
    ``native_layer_reasons`` is empty is ONE ``vllm_fusion_layer_forward``, and BOTH WEIGHT SLOTS ARE None: the native route returns
    ``((vision_features, None), (text_features, None))``, because the ``[B H, S, Lt]`` weight tensors are never built (not building
    them is the point; ``GroundingDinoEncoderLayer`` only hands them on to ``output_attentions``).  A caller who needs them leaves the
    switch off.  The native call computes the exact masked softmax; where that departs from the reference's clamped one is stated in
    include/vllm_hip.h, section f2f."""

    native_layer = False   # True: bf16 inference runs vllm_fusion_layer_forward where native_layer_reasons() is empty

    def __init__(self, config, init_values=1e-4):
        super().__init__()
        drop_path = config.fusion_droppath

        # pre layer norm
        self.layer_norm_vision = nn.LayerNorm(config.d_model)
        self.layer_norm_text = nn.LayerNorm(config.d_model)
        self.attn = GroundingDinoBiMultiHeadAttention(config)

        # add layer scale for training stability
        self.drop_path = GroundingDinoDropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.vision_param = nn.Parameter(init_values * torch.ones((config.d_model)), requires_grad=True)
        self.text_param = nn.Parameter(init_values * torch.ones((config.d_model)), requires_grad=True)

    def native_layer_reasons(self, vision_features, text_features, attention_mask_vision=None, attention_mask_text=None):
        """why this call keeps the composed path, as a list of strings (empty: the native call serves it)"""
        why = []
        x, t, a = vision_features, text_features, self.attn
        if self.training:
            why.append("training mode")
        params = list(self.parameters())
        if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
            why.append("parameters: bf16 on the GPU")
        if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or any(torch.is_tensor(v) and v.requires_grad for v in (x, t))):
            why.append("requires_grad under grad mode: there is no native backward")
        if not (is_gpu_bf16(x) and is_gpu_bf16(t)):
            why.append("vision_features / text_features: bf16 CUDA tensors [B, ., d_model]")
        if not (torch.is_tensor(x) and torch.is_tensor(t) and x.dim() == 3 and t.dim() == 3):
            return why
        if x.stride(-1) != 1 or t.stride(-1) != 1:
            why.append("vision_features / text_features: a contiguous last dim")
        C = a.vision_dim
        B, S, _ = x.shape
        Lt = t.shape[1]
        if not (C % 64 == 0 and 64 <= C <= 512 and a.head_dim in HEAD_DIMS and x.shape[-1] == C and tuple(t.shape) == (B, Lt, C) and Lt >= 1 and
                B * max(S, Lt) * a.embed_dim * 2 < 2 ** 31):
            why.append("shapes: d_model a multiple of 64 in 64 .. 512, head dim 128 or 256, [B, S, d_model] and [B, Lt >= 1, d_model] of one "
                       "batch, B max(S, Lt) embed_dim under 2^30")
        for name, m, n, dim in (("attention_mask_vision", attention_mask_vision, S, "S"), ("attention_mask_text", attention_mask_text, Lt, "Lt")):
            if m is not None and not (torch.is_tensor(m) and m.dtype == torch.bool and tuple(m.shape) == (B, n)):
                why.append(f"{name}: bool [B, {dim}] or None")
        return why

    def native_layer_applies(self, vision_features, text_features, attention_mask_vision=None, attention_mask_text=None):
        return not self.native_layer_reasons(vision_features, text_features, attention_mask_vision, attention_mask_text)

    def _fill_desc(self, keep):
        a = self.attn
        d = _lib.VllmFusionLayerDesc()
        d.d_model, d.embed_dim, d.n_heads = a.vision_dim, a.embed_dim, a.num_heads
        d.vision_norm_eps, d.text_norm_eps = self.layer_norm_vision.eps, self.layer_norm_text.eps
        put(d, keep, "vision_norm", self.layer_norm_vision.weight, self.layer_norm_vision.bias)
        put(d, keep, "text_norm", self.layer_norm_text.weight, self.layer_norm_text.bias)
        for name in ("vision_proj", "text_proj", "values_vision_proj", "values_text_proj", "out_vision_proj", "out_text_proj"):
            lin = getattr(a, name)
            put(d, keep, name, lin.weight, lin.bias)
        for name in ("vision_param", "text_param"):
            p = _lib.aligned(getattr(self, name).detach())
            keep.append(p)
            setattr(d, name, p.data_ptr())
        return d

    def _native_forward(self, vision_features, text_features, attention_mask_vision=None, attention_mask_text=None):
        B, S, C = vision_features.shape
        Lt = text_features.shape[1]
        L = _lib.lib()
        dev = vision_features.device
        keep = []
        d = self._fill_desc(keep)
        x, t = _lib.aligned(vision_features), _lib.aligned(text_features)
        vmask, tmask = opt_aligned(mask_u8(attention_mask_vision, dev)), opt_aligned(mask_u8(attention_mask_text, dev))
        out_v, out_t = torch.empty((B, S, C), dtype=torch.bfloat16, device=dev), torch.empty((B, Lt, C), dtype=torch.bfloat16, device=dev)
        ws, wsb = _lib.sized_workspace(dev, L.vllm_fusion_layer_workspace_bytes(ctypes.byref(d), B, S, Lt), "vllm_fusion_layer_workspace_bytes")
        with torch.cuda.device(dev):
            _lib.check(L.vllm_fusion_layer_forward(ctypes.byref(d), _lib.ptr(x), _lib.ptr(t), _lib.ptr(vmask), _lib.ptr(tmask), B, S, Lt,
                                                   _lib.ptr(out_v), _lib.ptr(out_t), _lib.ptr(ws), wsb, _lib.current_stream(dev)),
                       "vllm_fusion_layer_forward")
        return (out_v, None), (out_t, None)

    def forward(
        self,
        vision_features: torch.FloatTensor,
        text_features: torch.FloatTensor,
        attention_mask_vision: Optional[torch.BoolTensor] = None,
        attention_mask_text: Optional[torch.BoolTensor] = None,
    ) -> Tuple[Tuple[torch.FloatTensor, torch.FloatTensor], Tuple[torch.FloatTensor, torch.FloatTensor]]:
        """Image and text features fusion (:1059-1101)"""
        if self.native_layer and self.native_layer_applies(vision_features, text_features, attention_mask_vision, attention_mask_text):
            return self._native_forward(vision_features, text_features, attention_mask_vision, attention_mask_text)
        vision_features = self.layer_norm_vision(vision_features)
        text_features = self.layer_norm_text(text_features)
        (delta_v, vision_attn), (delta_t, text_attn) = self.attn(
            vision_features,
            text_features,
            vision_attention_mask=attention_mask_vision,
            text_attention_mask=attention_mask_text,
        )
        vision_features = vision_features + self.drop_path(self.vision_param * delta_v)
        text_features = text_features + self.drop_path(self.text_param * delta_t)

        return (vision_features, vision_attn), (text_features, text_attn)
