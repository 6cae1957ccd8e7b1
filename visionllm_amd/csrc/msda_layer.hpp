// What the deformable-attention layer's inference entry (msda_layer.hip) and its training entries (msda_layer_train.cpp, kernels in
// msda_layer_bwd.hip) share.  Host code only.
#pragma once
#include "kernels.hpp"

namespace vllm {

// Where one forward pass keeps its internal tensors: carved from the workspace by vllm_msda_layer_forward, from the caller's `saved`
// memory (value, loc, attw, opout_bf16) and the workspace (opout) by vllm_msda_layer_forward_train.
struct MsdaLayerBufs {
    float *value;           // [B, S, C] fp32, or bf16 in the same memory where the forward stores the value so (decoder route)
    float *loc;             // [B*Lq, M*L*P*2] offsets -> sampling locations
    float *attw;            // [B*Lq, M*L*P]   logits -> softmax weights
    float *opout;           // [B*Lq, C] fp32 operator output (scratch: unused where the operator writes bf16 itself)
    uint16_t *opout_bf16;   // [B*Lq, C] the operand of output_proj
};

int msda_layer_check_desc(const VllmMsdaLayerDesc *d);
// vllm_msda_layer_forward's workspace for a checked descriptor: its size, and its pieces in `workspace` (16-byte aligned)
long msda_layer_ws_bytes(const VllmMsdaLayerDesc *d, int B, int Lq, int S);
MsdaLayerBufs msda_layer_bufs(const VllmMsdaLayerDesc *d, void *workspace, int B, int Lq, int S);
// The forward pass behind both entries: every launch, in order.  *value_is_bf16 (host memory, may be null) tells how the value was stored.
// `residual` [B*Lq, C] bf16 (16-byte aligned, dense rows; null = none): out = residual + output_proj(...), added in output_proj's epilogue
// (deform_encoder_layer.hip); without it the launches and the bits are what they were.
int msda_layer_run(const VllmMsdaLayerDesc *d, const uint16_t *query, const float *ref, const uint16_t *input_flatten,
                   const uint8_t *padding_mask, const int64_t *shapes, const int64_t *lsi, int B, int Lq, int S, uint16_t *out,
                   const MsdaLayerBufs &b, int *value_is_bf16, hipStream_t st, const uint16_t *residual = nullptr);
// true where msda_layer_run MAY store the value as bf16 for these sizes (the sizes' part of its decision)
bool msda_layer_value_may_be_bf16(const VllmMsdaLayerDesc *d, int Lq, int S);

// msda_layer_bwd.hip
// dq [R, npad] bf16 = {grad_loc * (sx, sy) | w * (grad_w - sum_{L*P} grad_w w) | 0}: the backward of msda_prep_kernel
int msda_prep_bwd_launch(const float *grad_loc, const float *grad_w, const float *w, const float *ref, const int64_t *shapes, long R, int M,
                         int L, int P, int ref_dim, int four_d, uint16_t *dq, int npad, hipStream_t st);
// dst [rows, cols] bf16 = src fp32, round to nearest even; rows with a non-zero mask byte (mask may be null) are written as zeros
int f32_to_bf16_masked_launch(const float *src, uint16_t *dst, long rows, int cols, const uint8_t *mask, hipStream_t st);
int bf16_to_f32_launch(const uint16_t *src, float *dst, long n, hipStream_t st);

}  // namespace vllm
