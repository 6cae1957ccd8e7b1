"""The INPUTS of the Grounding-DINO encoder: the step of ``OVGroundingDinoModel`` between the backbone's feature maps and
``GroundingDinoEncoder`` (visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:2080-2111, :2164, :2200-2209, :2388-2439),
with ``GroundingDinoSinePositionEmbedding`` (:529-564), ``GroundingDinoLearnedPositionEmbedding`` (:567-588) and the mask down-sampling
of the backbone (:502) and of the extra levels (:2406), under the reference's parameter names: the ``input_proj_vision.*`` and
``level_embed`` slice of an ``OVGroundingDinoModel`` state-dict loads with ``strict=True``.  The config is read by attribute;
``transformers`` is not needed.

``GroundingDinoEncoderInputs.native_inputs = False`` (the default) runs the reference's statements; ``True`` makes a forward for which
``native_inputs_reasons`` is empty ONE ``vllm_gdino_inputs_forward`` (include/vllm_hip.h, section f2h; csrc/gdino_inputs.hip), whose
outputs ``GroundingDinoEncoder.native_encoder`` takes as they are.

One departure of the native call, stated in the header: the reference rounds the position embedding to bf16 and then adds
``level_embed`` with a second rounding; the native call adds in fp32 and rounds once."""
import ctypes
import dataclasses
import math
import weakref

import torch
from torch import nn

from . import _lib

GN_GROUPS = 32
MAX_LEVELS = 8   # struct VllmGdinoInputsDesc's arrays


class GroundingDinoSinePositionEmbedding(nn.Module):
    """
    This is a more standard version of the position embedding, very similar to the one used by the Attention is all you
    need paper, generalized to work on images. (:529-564)
    """

    def __init__(self, embedding_dim=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.temperature = temperature
        self.normalize = normalize
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        if scale is None:
            scale = 2 * math.pi
        self.scale = scale

    def dim_t(self, device):
        """the temperature table, by the two statements of ``forward``: the fp32 tensor the native call reads"""
        dim_t = torch.arange(self.embedding_dim, dtype=torch.float32, device=device)
        dim_t = self.temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / self.embedding_dim)
        return dim_t

    def forward(self, pixel_values, pixel_mask):
        if pixel_mask is None:
            raise ValueError("No pixel mask provided")
        y_embed = pixel_mask.cumsum(1, dtype=torch.float32)
        x_embed = pixel_mask.cumsum(2, dtype=torch.float32)
        if self.normalize:
            eps = 1e-6
            y_embed = y_embed / (y_embed[:, -1:, :] + eps) * self.scale
            x_embed = x_embed / (x_embed[:, :, -1:] + eps) * self.scale

        dim_t = torch.arange(self.embedding_dim, dtype=torch.float32, device=pixel_values.device)
        dim_t = self.temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / self.embedding_dim)

        pos_x = x_embed[:, :, :, None] / dim_t
        pos_y = y_embed[:, :, :, None] / dim_t
        pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos = torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)
        return pos


class GroundingDinoLearnedPositionEmbedding(nn.Module):
    """
    This module learns positional embeddings up to a fixed maximum size. (:567-588; the composed path only)
    """

    def __init__(self, embedding_dim=256):
        super().__init__()
        self.row_embeddings = nn.Embedding(50, embedding_dim)
        self.column_embeddings = nn.Embedding(50, embedding_dim)

    def forward(self, pixel_values, pixel_mask=None):
        height, width = pixel_values.shape[-2:]
        width_values = torch.arange(width, device=pixel_values.device)
        height_values = torch.arange(height, device=pixel_values.device)
        x_emb = self.column_embeddings(width_values)
        y_emb = self.row_embeddings(height_values)
        pos = torch.cat([x_emb.unsqueeze(0).repeat(height, 1, 1), y_emb.unsqueeze(1).repeat(1, width, 1)], dim=-1)
        pos = pos.permute(2, 0, 1)
        pos = pos.unsqueeze(0)
        pos = pos.repeat(pixel_values.shape[0], 1, 1, 1)
        return pos


def build_position_encoding(config):
    """:591-603; ``position_embedding_type`` defaults to "sine" """
    n_steps = config.d_model // 2
    kind = getattr(config, "position_embedding_type", "sine")
    if kind == "sine":
        position_embedding = GroundingDinoSinePositionEmbedding(n_steps, config.positional_embedding_temperature, normalize=True)
    elif kind == "learned":
        position_embedding = GroundingDinoLearnedPositionEmbedding(n_steps)
    else:
        raise ValueError(f"Not supported {kind}")

    return position_embedding


@dataclasses.dataclass
class GroundingDinoEncoderInputsOutput:
    """What ``forward`` (:2388-2439) hands to the encoder.  ``mask_flatten`` is True at a REAL cell: the model passes ``~mask_flatten`` on as
    ``vision_attention_mask``."""
    source_flatten: torch.Tensor = None          # [B, S, C]
    mask_flatten: torch.Tensor = None            # [B, S] bool
    lvl_pos_embed_flatten: torch.Tensor = None   # [B, S, C]
    spatial_shapes: torch.Tensor = None          # [L, 2] int64
    level_start_index: torch.Tensor = None       # [L] int64
    valid_ratios: torch.Tensor = None            # [B, L, 2] fp32


def _map_format(t):
    """0: contiguous NCHW, 1: torch.channels_last, None: neither (a view at a storage offset of either is one of them)"""
    if t.is_contiguous():
        return 0
    if t.is_contiguous(memory_format=torch.channels_last):
        return 1
    return None


_NATIVE_STATE = weakref.WeakKeyDictionary()   # GroundingDinoEncoderInputs -> {device: (signature, descriptor and what it points to)}


class GroundingDinoEncoderInputs(nn.Module):
    """``input_proj_vision``, ``level_embed`` and the position embedding of ``OVGroundingDinoModel`` (:2080-2111, :2164, :2077).
    ``config`` needs ``d_model``, ``num_feature_levels`` and ``positional_embedding_temperature`` (``position_embedding_type`` where it is
    not "sine"); ``in_channels``: the channels of the backbone's last maps (the reference's ``intermediate_channel_sizes[-3:]``).

    ``forward(feature_maps, pixel_mask)``: the backbone's last ``len(in_channels)`` maps ``[B, Cin_l, H_l, W_l]`` and the pixel mask
    ``[B, H, W]`` (bool / uint8 / int64, non-zero = a real pixel) -> GroundingDinoEncoderInputsOutput.  The module down-samples the mask
    itself for every level, with the reference's statement.  With ``native_inputs = True`` a call for which ``native_inputs_reasons`` is
    empty is ONE ``vllm_gdino_inputs_forward``.  The descriptor, the ``dim_t`` table and the 3 x 3 weights permuted to ``[C, 3, 3, Cin]``
    (a pure permutation in bf16) are remembered per device and rebuilt when a parameter's storage or version changes."""

    native_inputs = False   # True: bf16 inference runs vllm_gdino_inputs_forward where native_inputs_reasons() is empty

    def __init__(self, config, in_channels):
        super().__init__()
        self.config = config
        in_channels = list(in_channels)
        self.num_feature_levels = config.num_feature_levels
        self.position_embedding = build_position_encoding(config)

        # Create input projection layers (:2081-2111)
        if config.num_feature_levels > 1:
            num_backbone_outs = len(in_channels)
            input_proj_list = []
            for _ in range(num_backbone_outs):
                in_ch = in_channels[_]
                input_proj_list.append(
                    nn.Sequential(
                        nn.Conv2d(in_ch, config.d_model, kernel_size=1),
                        nn.GroupNorm(32, config.d_model),
                    )
                )
            for _ in range(config.num_feature_levels - num_backbone_outs):
                input_proj_list.append(
                    nn.Sequential(
                        nn.Conv2d(in_ch, config.d_model, kernel_size=3, stride=2, padding=1),
                        nn.GroupNorm(32, config.d_model),
                    )
                )
                in_ch = config.d_model
            self.input_proj_vision = nn.ModuleList(input_proj_list)
        else:
            self.input_proj_vision = nn.ModuleList(
                [
                    nn.Sequential(
                        nn.Conv2d(in_channels[-1], config.d_model, kernel_size=1),
                        nn.GroupNorm(32, config.d_model),
                    )
                ]
            )
        self.num_backbone_outs = len(in_channels) if config.num_feature_levels > 1 else 1

        self.level_embed = nn.Parameter(torch.Tensor(config.num_feature_levels, config.d_model))
        # GroundingDinoPreTrainedModel._init_weights
        nn.init.normal_(self.level_embed)
        for proj in self.input_proj_vision:
            nn.init.xavier_uniform_(proj[0].weight, gain=1)
            nn.init.constant_(proj[0].bias, 0)

    @staticmethod
    def downsample_mask(pixel_mask, size):
        """the reference's one statement (:502, :2406)"""
        return nn.functional.interpolate(pixel_mask[None].float(), size=size).to(torch.bool)[0]

    def get_valid_ratio(self, mask):
        """Get the valid ratio of all feature maps. (:2200-2209)"""

        _, height, width = mask.shape
        valid_height = torch.sum(mask[:, :, 0], 1)
        valid_width = torch.sum(mask[:, 0, :], 1)
        valid_ratio_heigth = valid_height.float() / height
        valid_ratio_width = valid_width.float() / width
        valid_ratio = torch.stack([valid_ratio_width, valid_ratio_heigth], -1)
        return valid_ratio

    # ---- the native call ------------------------------------------------------------------------------------------------------------------
    def native_inputs_reasons(self, feature_maps, pixel_mask):
        """Every reason why ``vllm_gdino_inputs_forward`` does not serve this call, as a list of strings (empty: it does)."""
        why = []
        if self.training:
            why.append("training mode")
        params = list(self.parameters())
        if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
            why.append("parameters: bf16 on the GPU")
        maps = list(feature_maps) if isinstance(feature_maps, (list, tuple)) else None
        if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or any(torch.is_tensor(m) and m.requires_grad for m in maps or ())):
            why.append("requires_grad under grad mode: there is no native backward")
        pe = self.position_embedding
        if not (isinstance(pe, GroundingDinoSinePositionEmbedding) and pe.normalize and pe.scale == 2 * math.pi):
            why.append("position_embedding: the sine embedding with normalize=True and scale 2 pi (a learned or un-normalised one keeps the composed path)")
        C = self.level_embed.shape[1]
        if not (C % 64 == 0 and 64 <= C <= 512):
            why.append("d_model a multiple of 64 in 64 .. 512")
        elif isinstance(pe, GroundingDinoSinePositionEmbedding) and pe.embedding_dim * 2 != C:
            why.append("position_embedding: embedding_dim d_model / 2")
        n_levels, n_maps = len(self.input_proj_vision), self.num_backbone_outs
        if not (1 <= n_maps <= n_levels <= MAX_LEVELS and self.level_embed.shape[0] == n_levels):
            why.append(f"levels: 1 <= backbone maps <= levels <= {MAX_LEVELS}, one level_embed row per level")
        for i, proj in enumerate(self.input_proj_vision):
            conv, gn = proj[0], proj[1]
            k = (1, 1) if i < n_maps else (3, 3)
            geometry = ((1, 1), (0, 0)) if i < n_maps else ((2, 2), (1, 1))
            if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == k and (conv.stride, conv.padding) == geometry and conv.out_channels == C
                    and conv.padding_mode == "zeros"):
                why.append(f"input_proj_vision.{i}.0: a 1 x 1 Conv2d (backbone levels) or a 3 x 3 / stride 2 / padding 1 Conv2d (extra levels) to d_model")
                continue
            if conv.groups != 1 or conv.dilation != (1, 1):
                why.append(f"input_proj_vision.{i}.0: a conv with groups or dilation")
            if conv.bias is None:
                why.append(f"input_proj_vision.{i}.0: a conv without bias")
            if conv.in_channels % 64:
                why.append(f"input_proj_vision.{i}.0: Cin {conv.in_channels} (a multiple of 64)")
            if i > n_maps and conv.in_channels != C or i == n_maps and conv.in_channels != self.input_proj_vision[n_maps - 1][0].in_channels:
                why.append(f"input_proj_vision.{i}.0: an extra level reads the last map's or d_model channels")
            if not (isinstance(gn, nn.GroupNorm) and gn.num_groups == GN_GROUPS and gn.num_channels == C):
                why.append(f"input_proj_vision.{i}.1: GroupNorm({GN_GROUPS}, d_model)")
            elif not gn.affine:
                why.append(f"input_proj_vision.{i}.1: GroupNorm without affine")
        if maps is None or len(maps) != n_maps or not all(torch.is_tensor(m) and m.is_cuda and m.dtype == torch.bfloat16 and m.dim() == 4 for m in maps):
            why.append(f"feature_maps: a list of {n_maps} bf16 CUDA tensors [B, Cin, H, W]")
            return why
        if any(_map_format(m) is None for m in maps):
            why.append("feature_maps: contiguous NCHW or torch.channels_last (offset views of either are served; arbitrary strides are not)")
        pm = pixel_mask
        if not (torch.is_tensor(pm) and pm.is_cuda and pm.dim() == 3 and pm.dtype in (torch.bool, torch.uint8, torch.int64)):
            why.append("pixel_mask: a bool / uint8 / int64 CUDA tensor [B, H, W]")
            return why
        B = pm.shape[0]
        if B < 1 or pm.shape[1] < 1 or pm.shape[2] < 1 or any(
                m.shape[0] != B or m.shape[1] != self.input_proj_vision[i][0].in_channels or m.shape[2] < 1 or m.shape[3] < 1
                for i, m in enumerate(maps)):
            why.append("shapes: the mask's and every map's batch agree, map l has input_proj_vision.l's input channels, no empty extent")
        elif any(B * m.shape[2] * m.shape[3] * max(9 * m.shape[1] if i == n_maps - 1 and n_levels > n_maps else m.shape[1], C) * 2 >= 2 ** 31
                 for i, m in enumerate(maps)):
            why.append("shapes: B H W rows of the widest GEMM operand under 2^31 bytes")
        return why

    def native_inputs_applies(self, feature_maps, pixel_mask):
        return not self.native_inputs_reasons(feature_maps, pixel_mask)

    def _native_state(self, device):
        """the descriptor of this module on ``device``: built once, rebuilt when a parameter's storage or version has changed"""
        sig = tuple((p.data_ptr(), p._version) for p in self.parameters())
        cache = _NATIVE_STATE.setdefault(self, {})
        ent = cache.get(device)
        if ent is not None and ent[0] == sig:
            return ent[1]
        keep = []

        def held(t):
            t = _lib.aligned(t.detach())
            keep.append(t)
            return t.data_ptr()

        d = _lib.VllmGdinoInputsDesc()
        d.d_model, d.n_levels, d.n_maps, d.reserved = self.level_embed.shape[1], len(self.input_proj_vision), self.num_backbone_outs, 0
        for i, proj in enumerate(self.input_proj_vision):
            conv, gn = proj[0], proj[1]
            d.c_in[i], d.gn_eps[i] = conv.in_channels, gn.eps
            w = conv.weight.detach()
            # 1 x 1: [C, Cin, 1, 1] is [C, Cin] as stored; 3 x 3: [C, Cin, 3, 3] -> [C, 3, 3, Cin], the patch matrix's (ky, kx, c) order
            d.conv_w[i] = held(w.reshape(w.shape[0], -1) if i < d.n_maps else w.permute(0, 2, 3, 1).contiguous())
            d.conv_b[i], d.gn_w[i], d.gn_b[i] = held(conv.bias), held(gn.weight), held(gn.bias)
        d.level_embed = held(self.level_embed)
        d.dim_t = held(self.position_embedding.dim_t(device).contiguous())
        state = dict(desc=d, keep=keep)
        cache[device] = (sig, state)
        return state

    def _native_forward(self, feature_maps, pixel_mask):
        dev = pixel_mask.device
        L = _lib.lib()
        st = self._native_state(dev)
        d = st["desc"]
        n = d.n_maps
        B, H, W = pixel_mask.shape
        maps, fmt = [], []
        for m in feature_maps:
            if m.data_ptr() % 16:   # a view at an unaligned storage offset: one copy in its own memory format
                m = m.clone(memory_format=torch.preserve_format)
            maps.append(m)
            fmt.append(_map_format(m))
        pm = pixel_mask.contiguous()
        IntN = ctypes.c_int * n
        map_h, map_w, map_fmt = IntN(*(m.shape[2] for m in maps)), IntN(*(m.shape[3] for m in maps)), IntN(*fmt)
        ptrs = (ctypes.c_void_p * n)(*(m.data_ptr() for m in maps))
        shapes = [(m.shape[2], m.shape[3]) for m in maps]
        for _ in range(d.n_levels - n):
            shapes.append(((shapes[-1][0] - 1) // 2 + 1, (shapes[-1][1] - 1) // 2 + 1))
        S, C = sum(h * w for h, w in shapes), d.d_model
        source = torch.empty((B, S, C), dtype=torch.bfloat16, device=dev)
        pos = torch.empty((B, S, C), dtype=torch.bfloat16, device=dev)
        mask = torch.empty((B, S), dtype=torch.bool, device=dev)
        valid_ratios = torch.empty((B, d.n_levels, 2), dtype=torch.float32, device=dev)
        ws, wsb = _lib.sized_workspace(dev, L.vllm_gdino_inputs_workspace_bytes(ctypes.byref(d), B, map_h, map_w, map_fmt),
                                       "vllm_gdino_inputs_workspace_bytes")
        with torch.cuda.device(dev):
            _lib.check(L.vllm_gdino_inputs_forward(ctypes.byref(d), ptrs, map_h, map_w, map_fmt, _lib.ptr(pm), pm.element_size(), B, H, W,
                                                   _lib.ptr(source), _lib.ptr(pos), _lib.ptr(mask), _lib.ptr(valid_ratios), _lib.ptr(ws), wsb,
                                                   _lib.current_stream(dev)), "vllm_gdino_inputs_forward")
        spatial_shapes = torch.as_tensor(shapes, dtype=torch.long, device=dev)
        level_start_index = torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1]))
        return GroundingDinoEncoderInputsOutput(source, mask, pos, spatial_shapes, level_start_index, valid_ratios)

    def forward(self, feature_maps, pixel_mask):
        if self.native_inputs and self.native_inputs_applies(feature_maps, pixel_mask):
            return self._native_forward(feature_maps, pixel_mask)

        # the backbone's statement per map (:500-503) and GroundingDinoConvModel's (:522-524)
        vision_features_input = []
        position_embeddings_list_input = []
        for feature_map in feature_maps:
            # downsample pixel_mask to match shape of corresponding feature_map
            mask = nn.functional.interpolate(pixel_mask[None].float(), size=feature_map.shape[-2:]).to(torch.bool)[0]
            vision_features_input.append((feature_map, mask))
            # position encoding
            position_embeddings_list_input.append(self.position_embedding(feature_map, mask).to(feature_map.dtype))

        # :2390-2410
        sources = []
        masks = []
        for level, (source, mask) in enumerate(vision_features_input):
            sources.append(self.input_proj_vision[level](source))
            masks.append(mask)
            if mask is None:
                raise ValueError("No attention mask was provided")

        # Lowest resolution feature maps are obtained via 3x3 stride 2 convolutions on the final stage
        if self.num_feature_levels > len(sources):
            _len_sources = len(sources)
            for level in range(_len_sources, self.num_feature_levels):
                if level == _len_sources:
                    source = self.input_proj_vision[level](vision_features_input[-1][0])
                else:
                    source = self.input_proj_vision[level](sources[-1])
                mask = nn.functional.interpolate(pixel_mask[None].float(), size=source.shape[-2:]).to(torch.bool)[0]
                pos_l = self.position_embedding(source, mask).to(source.dtype)
                sources.append(source)
                masks.append(mask)
                position_embeddings_list_input.append(pos_l)

        # Prepare encoder inputs (by flattening) (:2418-2439)
        source_flatten = []
        mask_flatten = []
        lvl_pos_embed_flatten = []
        spatial_shapes = []
        for level, (source, mask, pos_embed) in enumerate(zip(sources, masks, position_embeddings_list_input)):
            batch_size, num_channels, height, width = source.shape
            spatial_shape = (height, width)
            spatial_shapes.append(spatial_shape)
            source = source.flatten(2).transpose(1, 2)
            mask = mask.flatten(1)
            pos_embed = pos_embed.flatten(2).transpose(1, 2)
            lvl_pos_embed = pos_embed + self.level_embed[level].view(1, 1, -1)
            lvl_pos_embed_flatten.append(lvl_pos_embed)
            source_flatten.append(source)
            mask_flatten.append(mask)
        source_flatten = torch.cat(source_flatten, 1)
        mask_flatten = torch.cat(mask_flatten, 1)
        lvl_pos_embed_flatten = torch.cat(lvl_pos_embed_flatten, 1)
        spatial_shapes = torch.as_tensor(spatial_shapes, dtype=torch.long, device=source_flatten.device)
        level_start_index = torch.cat((spatial_shapes.new_zeros((1,)), spatial_shapes.prod(1).cumsum(0)[:-1]))
        valid_ratios = torch.stack([self.get_valid_ratio(m) for m in masks], 1)
        valid_ratios = valid_ratios.float()

        return GroundingDinoEncoderInputsOutput(source_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index,
                                                valid_ratios)
