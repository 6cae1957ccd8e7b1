// What the Grounding-DINO encoder (gdino_encoder.hip) strings together from the fusion layer (fusion_layer.cpp) and the deformable
// encoder layer (deform_encoder_layer.hip): each entry's refusals, workspace size and launches as functions that take a carved
// workspace, so that the public entries and the encoder run the same statements.  Host code only.
#pragma once
#include "kernels.hpp"

namespace vllm {

// fusion_layer.cpp.  check_desc / check_sizes: the descriptor's and the sizes' refusals; ws_bytes: for a checked descriptor and sizes,
// B S > 0; check_call: every other refusal of vllm_fusion_layer_forward, on the operands the launches will get; run: the launches.
int fusion_check_desc(const VllmFusionLayerDesc *d);
int fusion_check_sizes(const VllmFusionLayerDesc *d, int B, int S, int Lt);
long fusion_ws_bytes(const VllmFusionLayerDesc *d, int B, int S, int Lt);
int fusion_check_call(const VllmFusionLayerDesc *d, const uint16_t *vision, const uint16_t *text, int B, int S, int Lt, const uint16_t *out_vision,
                      const uint16_t *out_text, const void *workspace, long workspace_bytes);
int fusion_run(const VllmFusionLayerDesc *d, const uint16_t *vision, const uint16_t *text, const uint8_t *vision_padding_mask,
               const uint8_t *text_padding_mask, int B, int S, int Lt, uint16_t *out_vision, uint16_t *out_text, void *workspace, hipStream_t st);

// deform_encoder_layer.hip, in the same arrangement (B S > 0 for ws_bytes, check_call and run).
int enc_layer_check_desc(const VllmDeformEncLayerDesc *d);
long enc_layer_ws_bytes(const VllmDeformEncLayerDesc *d, int B, int S);
int enc_layer_check_call(const VllmDeformEncLayerDesc *d, const uint16_t *src, const uint16_t *pos, const uint16_t *query_in,
                         const float *reference_points, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int S,
                         const uint16_t *out, const uint16_t *query_out, const void *workspace, long workspace_bytes);
int enc_layer_run(const VllmDeformEncLayerDesc *d, const uint16_t *src, const uint16_t *pos, const uint16_t *query_in, const float *reference_points,
                  const uint8_t *padding_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int S, uint16_t *out,
                  uint16_t *query_out, void *workspace, hipStream_t st);

}  // namespace vllm
