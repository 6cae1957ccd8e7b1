"""visionllm_amd -- MI355X (gfx950) native image -> visual-token hot path of VisionLLMv2.

Host-side mirror of the reference's operator/module interfaces for that path only:

* ``ms_deform_attn``  -- ``ms_deform_attn_forward/backward``, ``MSDeformAttnFunction``, ``MSDeformAttn``,
  ``MultiScaleDeformableAttention`` (mmcv) and ``GroundingDinoMultiscaleDeformableAttention`` (HF) mirrors.
* ``intern_vit`` / ``clip_vit`` -- drop-in ``vis_encoder`` modules (same parameter names as the reference).
* ``bridge``          -- ``pixel_shuffle`` + ``vl_bridge`` projector.
* ``dist``            -- data-parallel sharding of images and the RCCL all-gather of visual tokens.
* ``deformable_encoder`` -- ``DeformableTransformerEncoderLayer`` (UniPose) and ``GroundingDinoDeformableLayer`` (HF) mirrors with the
  one-call native forward, and ``encoder_layers_forward``; the three names are also attributes of this package.
* ``deformable_decoder`` -- ``DeformableTransformerDecoderLayer`` (UniPose) and ``GroundingDinoDecoderLayer`` (HF) mirrors with the
  one-call native forward, and ``GroundingDinoDecoder`` (with ``GroundingDinoMLPPredictionHead``), the whole decoder loop as one native
  call; the four names are also attributes of this package.
* ``query_selection`` -- ``GroundingDinoQuerySelection``: the two-stage query selection between that encoder and that decoder
  (``gen_encoder_output_proposals``, the contrastive class head, the top-k and the gathers) with the one-call native forward; also an
  attribute of this package.
* ``fusion_layer`` -- ``GroundingDinoFusionLayer`` (with ``GroundingDinoBiMultiHeadAttention`` and ``GroundingDinoDropPath``): the
  bi-directional image <-> text attention in front of every Grounding-DINO encoder layer, with the one-call native forward; the three
  names are also attributes of this package.
* ``gdino_encoder`` -- ``GroundingDinoTextEnhancerLayer``, ``GroundingDinoEncoderLayer`` and ``GroundingDinoEncoder`` (with
  ``get_sine_pos_embed`` and ``GroundingDinoEncoderOutput``): the text enhancer with its one-call native forward, the layer that chains
  fusion layer, enhancer and deformable layer, and the whole encoder loop as one native call; the five names are also attributes of
  this package.
* ``gdino_inputs`` -- ``GroundingDinoEncoderInputs`` (with ``GroundingDinoSinePositionEmbedding`` and
  ``GroundingDinoEncoderInputsOutput``): the step between the backbone's feature maps and that encoder -- input projections with
  GroupNorm, the mask pyramid, the sine position embedding + level embedding, valid ratios -- with the one-call native forward; the
  three names are also attributes of this package.

All compute goes through ``libvllm_hip.so`` (hand-written HIP, C ABI in ``include/vllm_hip.h``).  There is NO
CPU fallback: calling an op without the built extension, or with CPU tensors, raises.
"""
from ._lib import build, lib, lib_path  # noqa: F401

__version__ = "0.1.0"

_ENCODER_EXPORTS = ("DeformableTransformerEncoderLayer", "GroundingDinoDeformableLayer", "encoder_layers_forward")
_DECODER_EXPORTS = ("DeformableTransformerDecoderLayer", "GroundingDinoDecoderLayer", "GroundingDinoDecoder", "GroundingDinoMLPPredictionHead")
_SELECTION_EXPORTS = ("GroundingDinoQuerySelection",)
_FUSION_EXPORTS = ("GroundingDinoFusionLayer", "GroundingDinoBiMultiHeadAttention", "GroundingDinoDropPath")
_GDINO_ENCODER_EXPORTS = ("GroundingDinoTextEnhancerLayer", "GroundingDinoEncoderLayer", "GroundingDinoEncoder", "GroundingDinoEncoderOutput",
                          "get_sine_pos_embed")
_GDINO_INPUTS_EXPORTS = ("GroundingDinoEncoderInputs", "GroundingDinoSinePositionEmbedding", "GroundingDinoEncoderInputsOutput")
__all__ = ["build", "lib", "lib_path", *_ENCODER_EXPORTS, *_DECODER_EXPORTS, *_SELECTION_EXPORTS, *_FUSION_EXPORTS, *_GDINO_ENCODER_EXPORTS,
           *_GDINO_INPUTS_EXPORTS]


def __getattr__(name):
    # resolved on first use: importing the package itself stays free of torch
    if name in _ENCODER_EXPORTS:
        from . import deformable_encoder
        return getattr(deformable_encoder, name)
    if name in _DECODER_EXPORTS:
        from . import deformable_decoder
        return getattr(deformable_decoder, name)
    if name in _SELECTION_EXPORTS:
        from . import query_selection
        return getattr(query_selection, name)
    if name in _FUSION_EXPORTS:
        from . import fusion_layer
        return getattr(fusion_layer, name)
    if name in _GDINO_ENCODER_EXPORTS:
        from . import gdino_encoder
        return getattr(gdino_encoder, name)
    if name in _GDINO_INPUTS_EXPORTS:
        from . import gdino_inputs
        return getattr(gdino_inputs, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
