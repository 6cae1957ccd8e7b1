"""The two-stage query selection of Grounding-DINO, between the deformable encoder (deformable_encoder.py) and the decoder
(deformable_decoder.py): ``gen_encoder_output_proposals`` and the ``two_stage`` statements of ``OVGroundingDinoModel.forward``
(visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:2228-2276, :2503-2543) with ``GroundingDinoContrastiveEmbedding``
(:1410-1428).  The mask heads (``forward_seg_heads``) are not part of it: the caller runs them on ``target_undetach`` or on its
``query_embeds``, as the reference does.

``GroundingDinoQuerySelection`` follows the arrangement of the other mirrors: ``native_selection = False`` (the default) runs the reference's
statements; ``native_selection = True`` makes a forward for which ``native_selection_reasons`` is empty ONE ``vllm_query_select_forward``
(csrc/query_select.hip)."""
import ctypes
import dataclasses

import torch
from torch import nn

from . import _lib
from ._native_call import is_gpu_bf16, mask_u8, put
from .deformable_decoder import GroundingDinoMLPPredictionHead, _box_heads
from .ms_deform_attn import level_pixels

MAX_QUERIES = 2048   # vllm_topk_rows_f32 sorts its survivors in LDS


class GroundingDinoContrastiveEmbedding(nn.Module):
    """modeling_ov_grounding_dino_mask_dn.py:1410-1428: vision . text^T, -inf at masked tokens, padded with -inf to ``max_text_len``
    columns.  The padded tensor is fp32 whatever the operands are, because ``torch.full`` is."""

    def __init__(self, config=None, max_text_len=None):
        super().__init__()
        self.max_text_len = max_text_len if max_text_len is not None else config.max_text_len

    def forward(self, vision_hidden_state, text_hidden_state, text_token_mask):
        output = vision_hidden_state @ text_hidden_state.transpose(-1, -2)
        output.masked_fill_(~text_token_mask[:, None, :], float("-inf"))

        # padding to max_text_len
        new_output = torch.full((*output.shape[:-1], self.max_text_len), float("-inf"), device=output.device)
        new_output[..., : output.shape[-1]] = output

        return new_output


@dataclasses.dataclass
class QuerySelectionOutput:
    """What the reference has computed at :2543.  On the native route the three full tensors are None (not building them is the point)."""
    target: torch.Tensor = None
    target_undetach: torch.Tensor = None            # None where ``query_embeds`` was given (the reference does not gather it then)
    reference_points: torch.Tensor = None
    init_reference_points: torch.Tensor = None
    enc_topk_coords_logits: torch.Tensor = None
    enc_topk_class_logits: torch.Tensor = None
    topk_proposals: torch.Tensor = None             # [B, num_queries] int64
    enc_outputs_class: torch.Tensor = None          # [B, S, max_text_len] fp32
    enc_outputs_coord_logits: torch.Tensor = None   # [B, S, 4] fp32
    object_query_embedding: torch.Tensor = None     # [B, S, C]


class GroundingDinoQuerySelection(nn.Module):
    """The members ``enc_output``, ``enc_output_norm``, ``encoder_output_bbox_embed`` and ``encoder_output_class_embed`` under the
    reference's names: the matching slice of an ``OVGroundingDinoModel`` state-dict loads.  ``bbox_embed`` may be given: the decoder's
    shared head object (``decoder_bbox_embed_share``), as the reference assigns it.

    ``forward(vision_features, text_features, mask_flatten, text_token_mask, spatial_shapes, num_queries, query_embeds=None)``:
    ``vision_features`` [B, S, C] is ``encoder_outputs[0]``, ``text_features`` [B, Lt, C] ``encoder_outputs[1]``, ``mask_flatten`` bool
    [B, S] with True = a REAL cell (the model's convention: it passes ``~mask_flatten`` on), ``text_token_mask`` bool [B, Lt] with True = a
    real token.

    With ``native_selection = False`` (the default) it is the reference's statements.  With ``native_selection = True`` a call for which
    ``native_selection_reasons`` is empty is ONE ``vllm_query_select_forward``.  The native route selects by the documented order -- score
    descending, ties by ascending index, NaN greatest, i.e. ``torch.sort(stable=True, descending=True)`` -- where ``torch.topk`` leaves
    ties unspecified, and it leaves ``enc_outputs_class``, ``enc_outputs_coord_logits`` and ``object_query_embedding`` None: they are
    never built.  A caller who needs them passes ``full_outputs=True``, which keeps the composed path.  On the native route
    ``reference_points`` and ``enc_topk_coords_logits`` are fp32 with the box delta never rounded to bf16."""

    native_selection = False   # True: bf16 inference runs vllm_query_select_forward where native_selection_reasons() is empty

    def __init__(self, d_model=256, max_text_len=256, bbox_embed=None):
        super().__init__()
        self.d_model = d_model
        self.enc_output = nn.Linear(d_model, d_model)
        self.enc_output_norm = nn.LayerNorm(d_model)
        self.encoder_output_bbox_embed = bbox_embed if bbox_embed is not None else GroundingDinoMLPPredictionHead(d_model, d_model, 4, 3)
        self.encoder_output_class_embed = GroundingDinoContrastiveEmbedding(max_text_len=max_text_len)

    def gen_encoder_output_proposals(self, enc_output, padding_mask, spatial_shapes):
        """modeling_ov_grounding_dino_mask_dn.py:2228-2276 -> (object_query [B, S, C], output_proposals [B, S, 4] fp32, after an inverse
        sigmoid; +inf at padded rows and invalid proposals)"""
        batch_size = enc_output.shape[0]
        proposals = []
        current_position = 0
        for level, (height, width) in enumerate(spatial_shapes):
            height, width = int(height), int(width)
            mask_flatten_ = padding_mask[:, current_position : (current_position + height * width)].view(
                batch_size, height, width, 1
            )
            valid_height = torch.sum(~mask_flatten_[:, :, 0, 0], 1)
            valid_width = torch.sum(~mask_flatten_[:, 0, :, 0], 1)

            grid_y, grid_x = torch.meshgrid(
                torch.linspace(0, height - 1, height, dtype=torch.float32, device=enc_output.device),
                torch.linspace(0, width - 1, width, dtype=torch.float32, device=enc_output.device),
                indexing="ij",
            )
            grid = torch.cat([grid_x.unsqueeze(-1), grid_y.unsqueeze(-1)], -1)

            scale = torch.cat([valid_width.unsqueeze(-1), valid_height.unsqueeze(-1)], 1).view(batch_size, 1, 1, 2)
            grid = (grid.unsqueeze(0).expand(batch_size, -1, -1, -1) + 0.5) / scale
            width_heigth = torch.ones_like(grid) * 0.05 * (2.0**level)
            proposal = torch.cat((grid, width_heigth), -1).view(batch_size, -1, 4)
            proposals.append(proposal)
            current_position += height * width

        output_proposals = torch.cat(proposals, 1)
        output_proposals_valid = ((output_proposals > 0.01) & (output_proposals < 0.99)).all(-1, keepdim=True)
        output_proposals = torch.log(output_proposals / (1 - output_proposals))  # inverse sigmoid
        output_proposals = output_proposals.masked_fill(padding_mask.unsqueeze(-1), float("inf"))
        output_proposals = output_proposals.masked_fill(~output_proposals_valid, float("inf"))

        # assign each pixel as an object query
        object_query = enc_output
        object_query = object_query.masked_fill(padding_mask.unsqueeze(-1), float(0))
        object_query = object_query.masked_fill(~output_proposals_valid, float(0))
        object_query = self.enc_output_norm(self.enc_output(object_query))
        return object_query, output_proposals

    def _mods(self):
        head = self.encoder_output_bbox_embed
        return [self.enc_output, self.enc_output_norm] + [m for m in getattr(head, "layers", ()) if isinstance(m, nn.Linear)]

    def native_selection_reasons(self, vision_features, text_features, mask_flatten, text_token_mask, spatial_shapes, num_queries,
                                 query_embeds=None, full_outputs=False):
        """Every reason why ``vllm_query_select_forward`` does not serve this call, as a list of strings (empty: it does)."""
        why = []
        x, text = vision_features, text_features
        C = self.d_model
        if self.training:
            why.append("training mode")
        if full_outputs:
            why.append("full_outputs: the native call never builds enc_outputs_class / enc_outputs_coord_logits / object_query_embedding")
        params = [p for m in self._mods() for p in m.parameters()]
        if any(p.dtype != torch.bfloat16 or not p.is_cuda for p in params):
            why.append("parameters: bf16 on the GPU")
        if any(getattr(m, "bias", 0) is None for m in self._mods()):
            why.append("parameters: a Linear / LayerNorm without bias")
        if torch.is_grad_enabled() and (any(p.requires_grad for p in params) or
                                        any(torch.is_tensor(t) and t.requires_grad for t in (x, text, query_embeds))):
            why.append("requires_grad under grad mode: there is no native backward")
        if not (C % 64 == 0 and 64 <= C <= 512 and tuple(self.enc_output.weight.shape) == (C, C) and
                tuple(self.enc_output_norm.weight.shape) == (C,)):
            why.append("d_model a multiple of 64 in 64 .. 512")
        if _box_heads([self.encoder_output_bbox_embed], 1, C) is None:
            why.append("encoder_output_bbox_embed: a three-layer head of width d_model")
        if not (is_gpu_bf16(x) and is_gpu_bf16(text)):
            why.append("vision_features / text_features: bf16 CUDA tensors [B, ., d_model]")
        if not (torch.is_tensor(x) and torch.is_tensor(text) and x.dim() == 3 and text.dim() == 3 and x.shape[-1] == C and
                text.shape[-1] == C and x.shape[0] == text.shape[0]):
            why.append("vision_features [B, S, d_model] and text_features [B, Lt, d_model] of one batch")
            return why
        B, S, _ = x.shape
        Lt = text.shape[1]
        mtl = getattr(self.encoder_output_class_embed, "max_text_len", 0)
        if not (1 <= Lt <= mtl <= 256):
            why.append("text: 1 <= Lt <= max_text_len <= 256")
        if not (isinstance(num_queries, int) and 1 <= num_queries <= min(S, MAX_QUERIES)):
            why.append(f"num_queries: 1 .. min(S, {MAX_QUERIES})")
        if not (torch.is_tensor(mask_flatten) and mask_flatten.dtype == torch.bool and tuple(mask_flatten.shape) == (B, S)):
            why.append("mask_flatten: bool [B, S]")
        if not (torch.is_tensor(text_token_mask) and text_token_mask.dtype == torch.bool and tuple(text_token_mask.shape) == (B, Lt)):
            why.append("text_token_mask: bool [B, Lt]")
        if not (torch.is_tensor(spatial_shapes) and spatial_shapes.dim() == 2 and spatial_shapes.shape[1] == 2 and
                1 <= spatial_shapes.shape[0] <= 16 and level_pixels(spatial_shapes) == S):
            why.append("spatial_shapes: [1 .. 16 levels, 2] describing the S rows")
        if B * S * C * 2 >= 2 ** 31:
            why.append("B S d_model: under 2^31 bytes")
        return why

    def _native_forward(self, x, text, mask_flatten, text_token_mask, spatial_shapes, k, query_embeds, scores_out=None):
        B, S, C = x.shape
        Lt = text.shape[1]
        mtl = self.encoder_output_class_embed.max_text_len
        L = _lib.lib()
        dev = x.device
        keep = []
        d = _lib.VllmQuerySelectDesc()
        d.d_model, d.max_text_len, d.n_levels, d.layer_norm_eps = C, mtl, spatial_shapes.shape[0], self.enc_output_norm.eps
        put(d, keep, "enc_output", self.enc_output.weight, self.enc_output.bias)
        put(d, keep, "enc_output_norm", self.enc_output_norm.weight, self.enc_output_norm.bias)
        for i, lin in enumerate(self.encoder_output_bbox_embed.layers):
            w, b = _lib.aligned(lin.weight.detach()), _lib.aligned(lin.bias.detach())
            keep.extend((w, b))
            setattr(d.box_head, f"w{i}", w.data_ptr())
            setattr(d.box_head, f"b{i}", b.data_ptr())
        xa, texta = _lib.aligned(x), _lib.aligned(text)
        pmask, tmask = mask_u8(~mask_flatten, dev), mask_u8(text_token_mask, dev)
        shapes = spatial_shapes.to(device=dev, dtype=torch.int64).contiguous()
        hw = shapes[:, 0] * shapes[:, 1]
        lsi = (torch.cumsum(hw, 0) - hw).contiguous()
        ws, wsb = _lib.sized_workspace(dev, L.vllm_query_select_workspace_bytes(ctypes.byref(d), B, S, Lt, k), "vllm_query_select_workspace_bytes")
        idx = torch.empty((B, k), dtype=torch.int64, device=dev)
        target = torch.empty((B, k, C), dtype=torch.bfloat16, device=dev)
        coords = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
        ref = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
        cls = torch.empty((B, k, mtl), dtype=torch.float32, device=dev)
        if scores_out is not None and not (scores_out.is_cuda and scores_out.dtype == torch.float32 and scores_out.is_contiguous() and
                                           tuple(scores_out.shape) == (B, S)):
            raise ValueError(f"scores_out: a contiguous fp32 CUDA tensor ({B}, {S})")
        with torch.cuda.device(dev):
            _lib.check(L.vllm_query_select_forward(ctypes.byref(d), _lib.ptr(xa), _lib.ptr(pmask), _lib.ptr(texta), _lib.ptr(tmask), _lib.ptr(shapes),
                                                   _lib.ptr(lsi), B, S, Lt, k, _lib.ptr(idx), _lib.ptr(target), _lib.ptr(coords), _lib.ptr(ref),
                                                   _lib.ptr(cls), _lib.ptr(scores_out), _lib.ptr(ws), wsb, _lib.current_stream(dev)),
                       "vllm_query_select_forward")
        out = QuerySelectionOutput(reference_points=ref, init_reference_points=ref, enc_topk_coords_logits=coords, enc_topk_class_logits=cls,
                                   topk_proposals=idx)
        if query_embeds is not None:
            out.target = query_embeds.unsqueeze(0).repeat(B, 1, 1)
        else:
            out.target_undetach = target
            out.target = target.detach()
        return out

    def forward(self, vision_features, text_features, mask_flatten, text_token_mask, spatial_shapes, num_queries, query_embeds=None,
                full_outputs=False, scores_out=None):
        """-> QuerySelectionOutput.  ``full_outputs=True`` asks for ``enc_outputs_class``, ``enc_outputs_coord_logits`` and
        ``object_query_embedding`` and therefore keeps the composed path, which always fills them.  ``scores_out`` (an fp32 CUDA tensor
        [B, S], native route only) receives the scores the selection was made from."""
        if self.native_selection and not self.native_selection_reasons(vision_features, text_features, mask_flatten, text_token_mask,
                                                                       spatial_shapes, num_queries, query_embeds, full_outputs):
            return self._native_forward(vision_features, text_features, mask_flatten, text_token_mask, spatial_shapes, num_queries,
                                        query_embeds, scores_out)
        batch_size = vision_features.shape[0]
        object_query_embedding, output_proposals = self.gen_encoder_output_proposals(
            vision_features, ~mask_flatten, spatial_shapes
        )

        # hack implementation for two-stage Deformable DETR
        # apply a detection head to each pixel (A.4 in paper)
        # linear projection for bounding box binary classification (i.e. foreground and background)
        enc_outputs_class = self.encoder_output_class_embed(
            object_query_embedding, text_features, text_token_mask
        )  # [bs, \sum(hw), K]
        # 3-layer FFN to predict bounding boxes coordinates (bbox regression branch)
        delta_bbox = self.encoder_output_bbox_embed(object_query_embedding)
        enc_outputs_coord_logits = delta_bbox + output_proposals  # [bs, \sum(hw), 4], unsigmoid

        # only keep top scoring `config.num_queries` proposals
        topk = num_queries
        topk_logits = enc_outputs_class.max(-1)[0]
        topk_proposals = torch.topk(topk_logits, topk, dim=1)[1]
        topk_coords_logits = torch.gather(
            enc_outputs_coord_logits, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, 4)
        )

        topk_coords_logits = topk_coords_logits.detach()
        reference_points = topk_coords_logits.sigmoid()
        init_reference_points = reference_points
        enc_topk_coords_logits = torch.gather(
            enc_outputs_coord_logits, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, 4)
        )
        enc_topk_class_logits = torch.gather(
            enc_outputs_class, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, enc_outputs_class.shape[-1])
        )
        target_undetach = None
        if query_embeds is not None:
            target = query_embeds.unsqueeze(0).repeat(batch_size, 1, 1)  # [num_queries, C] -> [bs, num_queries, c]
        else:
            target_undetach = torch.gather(object_query_embedding, 1, topk_proposals.unsqueeze(-1).repeat(1, 1, self.d_model))
            target = target_undetach.detach()
        return QuerySelectionOutput(target=target, target_undetach=target_undetach, reference_points=reference_points,
                                    init_reference_points=init_reference_points, enc_topk_coords_logits=enc_topk_coords_logits,
                                    enc_topk_class_logits=enc_topk_class_logits, topk_proposals=topk_proposals,
                                    enc_outputs_class=enc_outputs_class, enc_outputs_coord_logits=enc_outputs_coord_logits,
                                    object_query_embedding=object_query_embedding)
