// What the decoder layer's entry (deform_decoder_layer.hip) shares with the decoder loop around it (deform_decoder.hip).  Host code only.
#pragma once
#include "kernels.hpp"

namespace vllm {

int dec_layer_check_desc(const VllmDeformDecLayerDesc *d);
int dec_layer_check_sizes(const VllmDeformDecLayerDesc *d, int B, int Lq, int Lt, int S);
// vllm_deform_dec_layer_forward's workspace for a checked descriptor and checked sizes
long dec_layer_ws_bytes(const VllmDeformDecLayerDesc *d, int B, int Lq, int Lt, int S);
// Every refusal of vllm_deform_dec_layer_forward behind the descriptor and the sizes (B Lq > 0), in its order; host-only, enqueues nothing.
int dec_layer_check_call(const VllmDeformDecLayerDesc *d, const uint16_t *tgt, const uint16_t *query_pos, const float *reference_points,
                         const uint16_t *memory_text, const uint16_t *memory, const int64_t *spatial_shapes, const int64_t *level_start_index,
                         int B, int Lq, int Lt, int S, const uint16_t *out, const void *workspace, long workspace_bytes);
// The layer's launches, in order, for a call that dec_layer_check_call has passed.
int dec_layer_run(const VllmDeformDecLayerDesc *d, const uint16_t *tgt, const uint16_t *query_pos, const float *reference_points,
                  const uint8_t *self_attn_mask, const uint16_t *memory_text, const uint8_t *text_key_padding_mask, const uint16_t *memory,
                  const uint8_t *memory_padding_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int Lq, int Lt,
                  int S, uint16_t *out, void *workspace, hipStream_t st);

}  // namespace vllm
