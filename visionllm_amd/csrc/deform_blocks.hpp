// The blocks that the deformable encoder layer (deform_encoder_layer.hip, which owns the kernels and these definitions), the decoder
// layer (deform_decoder_layer.hip) and the decoder (deform_decoder.hip) are strung together from.  Host code only.
#pragma once
#include <array>
#include "kernels.hpp"

namespace vllm {

// y = LayerNorm(x + res) * w + b, y_pos = bf16(bf16(y) + pos) where given.  No checks: C a multiple of 64 in 64 .. 512, row operands
// as row_operand_ok (orchestrate.hpp) asks, w and b 16-byte aligned.
int add_layernorm_launch(const uint16_t *x, int ldx, const uint16_t *res, int ldr, const uint16_t *w, const uint16_t *b, uint16_t *y, int ldy,
                         const uint16_t *pos, int ldp, uint16_t *y_pos, int ldq, long rows, int C, float eps, hipStream_t st);
// out = bf16(a + b) over n elements.  No checks.
int add_launch(const uint16_t *a, const uint16_t *b, uint16_t *out, long n, hipStream_t st);

// The FFN behind a layer's attention: out = LayerNorm(x + fc2(act(fc1(x)))); act 0 = ReLU, VLLM_EPI_GELU = erf GELU.
struct FfnBlock {
    const uint16_t *fc1_w, *fc1_b, *fc2_w, *fc2_b, *norm_w, *norm_b;
    int act, d_ffn;
    float eps;
};
int ffn_check(const char *who, const FfnBlock &k);   // the descriptor's refusals: d_ffn, act, eps, a missing pointer
// fc1 + act and fc2 + residual, `slab_rows` rows at a time (h: one slab of the intermediate; t [R, C]: x + fc2(...)), then the
// LayerNorm t -> out, with out + pos -> y_pos where given.  Dense rows of C.
int ffn_block_run(hipStream_t st, const FfnBlock &k, const uint16_t *x, long R, int C, uint16_t *h, long slab_rows, uint16_t *t, uint16_t *out,
                  const uint16_t *pos, uint16_t *y_pos);

// an attention block's weights and biases, for the callers' alignment loops
inline std::array<const uint16_t *, 8> msda_weights(const VllmMsdaLayerDesc &at)
{
    return {at.value_proj_w, at.value_proj_b, at.sampling_offsets_w, at.sampling_offsets_b, at.attention_weights_w, at.attention_weights_b,
            at.output_proj_w, at.output_proj_b};
}

}  // namespace vllm
