// The Grounding-DINO ENCODER for bf16 modules at inference: the text enhancer as one call, and the loop of GroundingDinoEncoder.forward
// around the three blocks of GroundingDinoEncoderLayer as one call.
// Reference: grounding_dino/modeling_ov_grounding_dino_mask_dn.py -- GroundingDinoTextEnhancerLayer :787-857, get_sine_pos_embed :1185-1214,
//            GroundingDinoEncoderLayer :1217-1290, GroundingDinoEncoder :1560-1722.
//
// One call, one stream, a caller workspace (include/vllm_hip.h, section f2g).
// The enhancer is the decoder layer's block 1 (deform_decoder_layer.hip) with a mask per (image, head) and the FFN block of
// deform_blocks.hpp behind it:
//   add_bf16               q = text + pos                          (only with a position embedding)
//   GEMM N = 2C on q       in_proj_w[0:2C] -> [q | k];   GEMM N = C on text, in_proj_w[2C:3C] -> v
//   mha (mha.hip)          on the column slices, mask slab (b H + h) % n_masks
//   GEMM out_proj          with `text` added in its epilogue (EPI_RESIDUAL);   add_layernorm in place (layer_norm_before)
//   fc1 + ReLU / GELU, fc2 + residual, add_layernorm -> out (layer_norm_after)
// The encoder, once per call: encoder_refpoints_kernel and (unless the caller has it) text_pos_embed_kernel; then per layer fusion_run
// (fusion_layer.cpp), the enhancer's launches on the fused text, enc_layer_run (deform_encoder_layer.hip) on the fused vision features.
// One piece of the workspace serves the three blocks of every layer, one behind the other; vision and text ping-pong in two buffers
// each and the last layer writes the caller's outputs.  No atomics anywhere: the same bits on every run.
#include <math.h>
#include "common.hpp"
#include "orchestrate.hpp"
#include "deform_blocks.hpp"
#include "mha_core.hpp"
#include "gdino_encoder.hpp"

namespace vllm {
namespace {

// out[row, i] = sin (i even) / cos (i odd) of (p * 2 pi) / dim_t[i], p = positions[row] or the row's token index.  One thread per 8 consecutive
// columns of a row (one 16-byte store), no loop; fp32 as the module's statements, a true division, the accurate sinf / cosf, one rounding.
__global__ __launch_bounds__(256) void text_pos_embed_kernel(const float *__restrict__ positions, const float *__restrict__ dim_t, long rows, int Lt,
                                                             int C, uint16_t *__restrict__ out, int ld)
{
    const int cpr = C >> 3;   // 16-byte chunks per row
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < rows * cpr) {
        const long row = t / cpr;
        const int j = (int)(t - row * cpr);
        const float p = positions ? positions[row] : (float)(row % Lt);
        const float pos = p * 6.283185307179586f;
        const float4_t d0 = *reinterpret_cast<const float4_t *>(dim_t + j * 8), d1 = *reinterpret_cast<const float4_t *>(dim_t + j * 8 + 4);
        float o[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a0 = __fdiv_rn(pos, d0[e]), a1 = __fdiv_rn(pos, d1[e]);
            o[e] = (e & 1) ? cosf(a0) : sinf(a0);
            o[4 + e] = (e & 1) ? cosf(a1) : sinf(a1);
        }
        *reinterpret_cast<uint4_t *>(out + row * ld + j * 8) = pack8(o);
    }
}

// One thread per (image, token): the token's level l (the last whose start is not behind it), its column and row there, then
// ((c + 0.5) / (valid_ratio[b, l] * extent)) * valid_ratio[b, l'] for every level l' -- each product and the division one fp32 operation
// in the module's order (c + 0.5 is exact: the module's linspace has step 1).  2 L floats per thread, written as float2.
constexpr int REFPOINT_MAX_LEVELS = 16;
__global__ __launch_bounds__(256) void encoder_refpoints_kernel(const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
                                                                const float *__restrict__ vr, long rows, int S, int L, float *__restrict__ out)
{
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const long b = r / S;
    const long s = r - b * S;
    int l = 0;
    for (int i = 1; i < L; ++i)
        if (lsi[i] <= s) l = i;
    const long H = shapes[2 * l], W = shapes[2 * l + 1] > 0 ? shapes[2 * l + 1] : 1;
    const long idx = s - lsi[l];
    const long row = idx / W, col = idx - row * W;
    const float2_t *vrb = reinterpret_cast<const float2_t *>(vr) + b * L;
    const float2_t own = vrb[l];
    const float x = __fdiv_rn((float)col + 0.5f, own[0] * (float)W), y = __fdiv_rn((float)row + 0.5f, own[1] * (float)H);
    float2_t *o = reinterpret_cast<float2_t *>(out) + r * L;
    for (int i = 0; i < L; ++i) {
        const float2_t v = vrb[i];
        o[i] = (float2_t){x * v[0], y * v[1]};
    }
}

int text_pos_embed_launch(const float *positions, const float *dim_t, long rows, int Lt, int C, uint16_t *out, int ld, hipStream_t st)
{
    VLLM_LAUNCH(text_pos_embed_kernel, dim3((unsigned)((rows * (C / 8) + 255) / 256)), dim3(256), 0, st, positions, dim_t, rows, Lt, C, out, ld);
    VLLM_CHECK_LAUNCH("text_pos_embed_kernel");
    return VLLM_OK;
}

int encoder_refpoints_launch(const int64_t *shapes, const int64_t *lsi, const float *vr, long rows, int S, int L, float *out, hipStream_t st)
{
    VLLM_LAUNCH(encoder_refpoints_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, shapes, lsi, vr, rows, S, L, out);
    VLLM_CHECK_LAUNCH("encoder_refpoints_kernel");
    return VLLM_OK;
}

// ---- the text enhancer -------------------------------------------------------------------------------------------------------------------
const char *const ENH = "text_enhancer";

struct EnhWs {
    long xp, qk, v, ctx, y, h, t, total;   // xp: text + pos; qk [R, 2C]; v, ctx [R, C]; y: text + attention, normalised in place; h [R, d_ffn]; t: y + fc2(...)
};
EnhWs enh_ws(const VllmTextEnhancerDesc *d, long B, long Lt)
{
    const long R = B * Lt, C = d->d_model, F = d->d_ffn;
    EnhWs w;
    Carver cv;
    w.xp = cv.take(R * C * 2);
    w.qk = cv.take(R * 2 * C * 2);
    w.v = cv.take(R * C * 2);
    w.ctx = cv.take(R * C * 2);
    w.y = cv.take(R * C * 2);
    w.h = cv.take(R * F * 2);
    w.t = cv.take(R * C * 2);
    w.total = cv.off;
    return w;
}

FfnBlock enh_ffn(const VllmTextEnhancerDesc *d)
{
    return {d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, d->norm_after_w, d->norm_after_b, d->act, d->d_ffn, d->norm_after_eps};
}

int enh_check_desc(const VllmTextEnhancerDesc *d)
{
    VLLM_REQUIRE(d, "%s: null descriptor", ENH);
    const int C = d->d_model;
    VLLM_REQUIRE(C >= 64 && C <= 512 && C % 64 == 0, "%s: d_model=%d (a multiple of 64 in 64 .. 512)", ENH, C);
    VLLM_REQUIRE(d->n_heads >= 1 && C % d->n_heads == 0 && (C / d->n_heads == 32 || C / d->n_heads == 64),
                 "%s: n_heads=%d with d_model=%d (head dim 32 or 64)", ENH, d->n_heads, C);
    TRY(ffn_check(ENH, enh_ffn(d)));
    VLLM_REQUIRE(d->norm_before_eps >= 0.f, "%s: negative eps", ENH);
    VLLM_REQUIRE(d->in_proj_w && d->in_proj_b && d->out_proj_w && d->out_proj_b && d->norm_before_w && d->norm_before_b, "%s: missing weights", ENH);
    return VLLM_OK;
}

int enh_check_sizes(const VllmTextEnhancerDesc *d, int B, int Lt)
{
    const long widest = d->d_ffn > 2 * d->d_model ? d->d_ffn : 2 * d->d_model;
    // (the GEMMs address an operand with 32-bit byte offsets)
    VLLM_REQUIRE(B >= 0 && Lt >= 0 && (long)B * Lt * widest * 2 < (1L << 31),
                 "%s: B=%d Lt=%d (B, Lt >= 0; B Lt rows of the widest intermediate below 2^31 bytes)", ENH, B, Lt);
    return VLLM_OK;
}

// the pieces of the workspace and the attention's operands, as the checks and the launches both see them
struct EnhCall {
    uint16_t *xp, *qk, *v, *ctx, *y, *h, *t;
    int H, D;
    AttnOperand q, k, vv, o;
};
EnhCall enh_call(const VllmTextEnhancerDesc *d, const EnhWs &w, void *workspace, long Lt)
{
    char *ws = (char *)workspace;
    const int C = d->d_model;
    EnhCall c;
    c.xp = (uint16_t *)(ws + w.xp); c.qk = (uint16_t *)(ws + w.qk); c.v = (uint16_t *)(ws + w.v); c.ctx = (uint16_t *)(ws + w.ctx);
    c.y = (uint16_t *)(ws + w.y); c.h = (uint16_t *)(ws + w.h); c.t = (uint16_t *)(ws + w.t);
    c.H = d->n_heads; c.D = C / c.H;
    c.q = {c.qk, Lt * 2 * C, 2 * C}; c.k = {c.qk + C, Lt * 2 * C, 2 * C}; c.vv = {c.v, Lt * C, C}; c.o = {c.ctx, Lt * C, C};
    return c;
}

// every refusal of vllm_text_enhancer_forward behind the descriptor's and the sizes', on the operands the launches will get (B Lt > 0)
int enh_check_call(const VllmTextEnhancerDesc *d, const uint16_t *text, const uint16_t *pos, int n_masks, int B, int Lt, const uint16_t *out,
                   const void *workspace, long workspace_bytes)
{
    VLLM_REQUIRE(text && out, "%s: null pointer (text / out)", ENH);
    VLLM_REQUIRE(n_masks >= 1, "%s: n_masks=%d (at least 1)", ENH, n_masks);
    VLLM_REQUIRE(aligned16(text) && aligned16(pos) && aligned16(out), "%s: misaligned text / pos / out (16 bytes)", ENH);
    for (const uint16_t *p : {d->in_proj_w, d->in_proj_b, d->out_proj_w, d->out_proj_b, d->norm_before_w, d->norm_before_b, d->fc1_w, d->fc1_b,
                              d->fc2_w, d->fc2_b, d->norm_after_w, d->norm_after_b})
        VLLM_REQUIRE(aligned16(p), "%s: misaligned weight or bias (16 bytes)", ENH);
    const long bytes = (long)B * Lt * d->d_model * 2;
    VLLM_REQUIRE(!ranges_overlap(out, bytes, text, bytes) && !ranges_overlap(out, bytes, pos, bytes), "%s: out overlaps an input (text / pos)", ENH);
    const EnhWs w = enh_ws(d, B, Lt);
    VLLM_REQUIRE(workspace, "%s: null workspace (%ld bytes)", ENH, w.total);
    VLLM_REQUIRE(aligned16(workspace), "%s: misaligned workspace (16 bytes)", ENH);
    VLLM_REQUIRE(workspace_bytes >= w.total, "%s: workspace too small (%ld < %ld bytes)", ENH, workspace_bytes, w.total);
    VLLM_REQUIRE(!ranges_overlap(workspace, w.total, text, bytes) && !ranges_overlap(workspace, w.total, pos, bytes) &&
                     !ranges_overlap(workspace, w.total, out, bytes),
                 "%s: workspace overlaps an operand", ENH);
    const EnhCall c = enh_call(d, w, const_cast<void *>(workspace), Lt);
    // the attention kernel's own gate, asked before anything is enqueued (dense slices of the buffers above: it cannot refuse them)
    return mha_fwd_check(c.q, c.k, c.vv, c.o, B, Lt, Lt, c.H, c.D);
}

int enh_run(const VllmTextEnhancerDesc *d, const uint16_t *text, const uint16_t *pos, const uint8_t *attn_mask, int n_masks, int B, int Lt,
            uint16_t *out, void *workspace, hipStream_t st)
{
    const int C = d->d_model;
    const long R = (long)B * Lt;
    const EnhCall c = enh_call(d, enh_ws(d, B, Lt), workspace, Lt);
    // queries = keys = text + pos (:841)
    const uint16_t *qin = text;
    if (pos) { TRY(add_launch(text, pos, c.xp, R * C, st)); qin = c.xp; }
    // nn.MultiheadAttention (:842-844): the packed in_proj, sliced by pointer offset
    TRY(gemm(st, EPI_BIAS, qin, C, d->in_proj_w, C, d->in_proj_b, c.qk, 2 * C, (int)R, 2 * C, C));
    TRY(gemm(st, EPI_BIAS, text, C, d->in_proj_w + 2L * C * C, C, d->in_proj_b + 2 * C, c.v, C, (int)R, C, C));
    TRY(mha_fwd_launch(c.q, c.k, c.vv, c.o, attn_mask, nullptr, B, Lt, Lt, c.H, c.D, 1.0f / sqrtf((float)c.D), st, n_masks));
    // text + attention (:846) in out_proj's epilogue, layer_norm_before (:847) in place
    TRY(gemm(st, EPI_RESIDUAL, c.ctx, C, d->out_proj_w, C, d->out_proj_b, c.y, C, (int)R, C, C, nullptr, text, C));
    TRY(add_layernorm_launch(c.y, C, nullptr, 0, d->norm_before_w, d->norm_before_b, c.y, C, nullptr, 0, nullptr, 0, R, C, d->norm_before_eps, st));
    // the FFN and layer_norm_after (:849-855), the whole intermediate at once
    return ffn_block_run(st, enh_ffn(d), c.y, R, C, c.h, R, c.t, out, nullptr, nullptr);
}

// ---- the encoder ---------------------------------------------------------------------------------------------------------------------------
const char *const ENC = "gdino_encoder";

struct EncoderWs {
    long layer, layer_bytes;   // one block's workspace, the largest of every layer's three, reused by each
    long vis[2], txt[2];       // vision [B S, C] and text [B Lt, C], ping-pong: [0] the fusion layer's outputs, [1] the layer's
    long ref, tpos;            // reference points [B, S, L, 2] fp32; the text position embedding [B Lt, C]
    long total;
};
EncoderWs encoder_ws(const VllmGdinoEncoderDesc *d, long B, long S, long Lt)
{
    const long C = d->fusion[0].d_model, L = d->deformable[0].attn.n_levels;
    EncoderWs w;
    w.layer_bytes = 0;
    for (int l = 0; l < d->n_layers; ++l)
        for (const long b : {fusion_ws_bytes(&d->fusion[l], (int)B, (int)S, (int)Lt), enh_ws(&d->enhancer[l], B, Lt).total,
                             enc_layer_ws_bytes(&d->deformable[l], (int)B, (int)S)})
            if (b > w.layer_bytes) w.layer_bytes = b;
    Carver cv;
    w.layer = cv.take(w.layer_bytes);
    for (int i = 0; i < 2; ++i) w.vis[i] = cv.take(B * S * C * 2);
    for (int i = 0; i < 2; ++i) w.txt[i] = cv.take(B * Lt * C * 2);
    w.ref = cv.take(B * S * L * 2 * 4);
    w.tpos = cv.take(B * Lt * C * 2);
    w.total = cv.off;
    return w;
}

int encoder_check_desc(const VllmGdinoEncoderDesc *d)
{
    VLLM_REQUIRE(d, "%s: null descriptor", ENC);
    VLLM_REQUIRE(d->n_layers >= 1 && d->n_layers <= 64 && d->fusion && d->enhancer && d->deformable,
                 "%s: n_layers=%d (1 .. 64, with the three arrays of descriptors)", ENC, d->n_layers);
    for (int l = 0; l < d->n_layers; ++l) {
        TRY(fusion_check_desc(&d->fusion[l]));
        TRY(enh_check_desc(&d->enhancer[l]));
        TRY(enc_layer_check_desc(&d->deformable[l]));
        const VllmMsdaLayerDesc &at = d->deformable[l].attn, &a0 = d->deformable[0].attn;
        VLLM_REQUIRE(d->fusion[l].d_model == a0.d_model && d->enhancer[l].d_model == a0.d_model && at.d_model == a0.d_model &&
                         at.n_levels == a0.n_levels,
                     "%s: layer %d has d_model=%d / %d / %d (fusion / enhancer / deformable) and n_levels=%d, layer 0 %d and %d", ENC, l,
                     d->fusion[l].d_model, d->enhancer[l].d_model, at.d_model, at.n_levels, a0.d_model, a0.n_levels);
    }
    VLLM_REQUIRE(d->deformable[0].attn.n_levels <= REFPOINT_MAX_LEVELS, "%s: n_levels=%d above %d", ENC, d->deformable[0].attn.n_levels,
                 REFPOINT_MAX_LEVELS);
    VLLM_REQUIRE(d->dim_t, "%s: missing dim_t", ENC);
    return VLLM_OK;
}

int encoder_check_sizes(const VllmGdinoEncoderDesc *d, int B, int S, int Lt)
{
    VLLM_REQUIRE(B >= 0 && S >= 0 && Lt >= 0 && (long)B * S < (1L << 31), "%s: B=%d S=%d Lt=%d (non-negative, B S below 2^31)", ENC, B, S, Lt);
    if ((long)B * S == 0 || (long)B * Lt == 0) return VLLM_OK;   // nothing to do: the blocks' own size rules are not asked
    for (int l = 0; l < d->n_layers; ++l) {
        TRY(fusion_check_sizes(&d->fusion[l], B, S, Lt));
        TRY(enh_check_sizes(&d->enhancer[l], B, Lt));
    }
    return VLLM_OK;
}

long g_enh_calls = 0, g_enc_calls = 0;

}  // namespace
}  // namespace vllm

using namespace vllm;

static_assert(sizeof(VllmTextEnhancerDesc) == 4 * sizeof(int32_t) + 2 * sizeof(float) + 12 * sizeof(void *), "VllmTextEnhancerDesc: 12 pointers behind six scalars");
static_assert(sizeof(VllmGdinoEncoderDesc) == 2 * sizeof(int32_t) + 4 * sizeof(void *), "VllmGdinoEncoderDesc: 4 pointers behind two scalars");

extern "C" unsigned long vllm_text_enhancer_desc_sizeof(void) { return sizeof(VllmTextEnhancerDesc); }
extern "C" unsigned long vllm_gdino_encoder_desc_sizeof(void) { return sizeof(VllmGdinoEncoderDesc); }
extern "C" long vllm_text_enhancer_calls(void) { return g_enh_calls; }
extern "C" long vllm_gdino_encoder_calls(void) { return g_enc_calls; }

extern "C" int vllm_text_pos_embed_bf16(const float *positions, const float *dim_t, int B, int Lt, int C, uint16_t *out, int ld_out,
                                        vllm_stream_t stream)
{
    VLLM_REQUIRE(C >= 64 && C <= 512 && C % 64 == 0, "text_pos_embed: C=%d (a multiple of 64 in 64 .. 512)", C);
    VLLM_REQUIRE(B >= 0 && Lt >= 0 && (long)B * Lt < (1L << 31), "text_pos_embed: B=%d Lt=%d", B, Lt);
    if ((long)B * Lt == 0) return VLLM_OK;
    VLLM_REQUIRE(dim_t && out, "text_pos_embed: null pointer (dim_t / out)");
    VLLM_REQUIRE(aligned16(dim_t) && aligned16(out) && (reinterpret_cast<uintptr_t>(positions) & 3u) == 0 && ld_out >= C && ld_out % 8 == 0,
                 "text_pos_embed: misaligned operand (dim_t, out 16 bytes; positions 4) or ld_out=%d (a multiple of 8, at least C)", ld_out);
    return text_pos_embed_launch(positions, dim_t, (long)B * Lt, Lt, C, out, ld_out, (hipStream_t)stream);
}

extern "C" int vllm_encoder_refpoints_f32(const int64_t *spatial_shapes, const int64_t *level_start_index, const float *valid_ratios, int B, int S,
                                          int L, float *out, vllm_stream_t stream)
{
    VLLM_REQUIRE(L >= 1 && L <= REFPOINT_MAX_LEVELS, "encoder_refpoints: L=%d (1 .. %d)", L, REFPOINT_MAX_LEVELS);
    VLLM_REQUIRE(B >= 0 && S >= 0 && (long)B * S < (1L << 31), "encoder_refpoints: B=%d S=%d (0 <= B S < 2^31)", B, S);
    if ((long)B * S == 0) return VLLM_OK;
    VLLM_REQUIRE(spatial_shapes && level_start_index && valid_ratios && out, "encoder_refpoints: null pointer");
    VLLM_REQUIRE(aligned8(spatial_shapes) && aligned8(level_start_index) && aligned8(valid_ratios) && aligned16(out),
                 "encoder_refpoints: misaligned operand (out 16 bytes; spatial_shapes, level_start_index, valid_ratios 8)");
    return encoder_refpoints_launch(spatial_shapes, level_start_index, valid_ratios, (long)B * S, S, L, out, (hipStream_t)stream);
}

extern "C" long vllm_text_enhancer_workspace_bytes(const VllmTextEnhancerDesc *d, int B, int Lt)
{
    if (enh_check_desc(d) != VLLM_OK || enh_check_sizes(d, B, Lt) != VLLM_OK) return -1;
    if ((long)B * Lt == 0) return 0;
    return enh_ws(d, B, Lt).total;
}

extern "C" int vllm_text_enhancer_forward(const VllmTextEnhancerDesc *d, const uint16_t *text, const uint16_t *pos, const uint8_t *attn_mask,
                                          int n_masks, int B, int Lt, uint16_t *out, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    TRY(enh_check_desc(d));
    TRY(enh_check_sizes(d, B, Lt));
    if ((long)B * Lt == 0) return VLLM_OK;
    TRY(enh_check_call(d, text, pos, n_masks, B, Lt, out, workspace, workspace_bytes));
    ++g_enh_calls;
    return enh_run(d, text, pos, attn_mask, n_masks, B, Lt, out, workspace, (hipStream_t)stream);
}

extern "C" long vllm_gdino_encoder_workspace_bytes(const VllmGdinoEncoderDesc *d, int B, int S, int Lt)
{
    if (encoder_check_desc(d) != VLLM_OK || encoder_check_sizes(d, B, S, Lt) != VLLM_OK) return -1;
    if ((long)B * S == 0 || (long)B * Lt == 0) return 0;
    return encoder_ws(d, B, S, Lt).total;
}

extern "C" int vllm_gdino_encoder_forward(const VllmGdinoEncoderDesc *d, const uint16_t *vision, const uint16_t *vision_pos,
                                          const uint8_t *vision_padding_mask, const float *valid_ratios, const int64_t *spatial_shapes,
                                          const int64_t *level_start_index, const uint16_t *text, const uint8_t *text_padding_mask,
                                          const uint8_t *text_self_attn_mask, int n_masks, const float *text_positions,
                                          const uint16_t *text_pos_embed, int B, int S, int Lt, uint16_t *out_vision, uint16_t *out_text,
                                          void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    TRY(encoder_check_desc(d));
    TRY(encoder_check_sizes(d, B, S, Lt));
    if ((long)B * S == 0 || (long)B * Lt == 0) return VLLM_OK;
    const int NL = d->n_layers, C = d->fusion[0].d_model, L = d->deformable[0].attn.n_levels;
    const long Rv = (long)B * S, Rt = (long)B * Lt, vbytes = Rv * C * 2, tbytes = Rt * C * 2;
    VLLM_REQUIRE(vision && vision_pos && valid_ratios && spatial_shapes && level_start_index && text && out_vision && out_text,
                 "%s: null pointer (vision / vision_pos / valid_ratios / spatial_shapes / level_start_index / text / out_vision / out_text)", ENC);
    VLLM_REQUIRE(n_masks >= 1, "%s: n_masks=%d (at least 1)", ENC, n_masks);
    VLLM_REQUIRE(aligned16(vision) && aligned16(vision_pos) && aligned16(text) && aligned16(text_pos_embed) && aligned16(out_vision) &&
                     aligned16(out_text) && aligned16(d->dim_t) && aligned8(valid_ratios) && aligned8(spatial_shapes) && aligned8(level_start_index) &&
                     (reinterpret_cast<uintptr_t>(text_positions) & 3u) == 0,
                 "%s: misaligned vision / vision_pos / text / text_pos_embed / out_vision / out_text / dim_t (16 bytes), valid_ratios / "
                 "spatial_shapes / level_start_index (8) or text_positions (4)", ENC);
    const struct { const void *p; long bytes; } inputs[] = {{vision, vbytes}, {vision_pos, vbytes}, {text, tbytes}, {text_pos_embed, tbytes},
                                                            {valid_ratios, (long)B * L * 8}, {text_positions, Rt * 4}};
    for (const auto &in : inputs)
        VLLM_REQUIRE(!ranges_overlap(out_vision, vbytes, in.p, in.bytes) && !ranges_overlap(out_text, tbytes, in.p, in.bytes),
                     "%s: an output overlaps an input (vision / vision_pos / text / text_pos_embed / valid_ratios / text_positions)", ENC);
    VLLM_REQUIRE(!ranges_overlap(out_vision, vbytes, out_text, tbytes), "%s: the two outputs overlap", ENC);
    const EncoderWs w = encoder_ws(d, B, S, Lt);
    VLLM_REQUIRE(workspace, "%s: null workspace (%ld bytes)", ENC, w.total);
    VLLM_REQUIRE(aligned16(workspace), "%s: misaligned workspace (16 bytes)", ENC);
    VLLM_REQUIRE(workspace_bytes >= w.total, "%s: workspace too small (%ld < %ld bytes)", ENC, workspace_bytes, w.total);
    for (const auto &in : inputs)
        VLLM_REQUIRE(!ranges_overlap(workspace, w.total, in.p, in.bytes), "%s: workspace overlaps an operand", ENC);
    VLLM_REQUIRE(!ranges_overlap(workspace, w.total, out_vision, vbytes) && !ranges_overlap(workspace, w.total, out_text, tbytes),
                 "%s: workspace overlaps an operand", ENC);
    char *ws = (char *)workspace;
    uint16_t *vis[2] = {(uint16_t *)(ws + w.vis[0]), (uint16_t *)(ws + w.vis[1])}, *txt[2] = {(uint16_t *)(ws + w.txt[0]), (uint16_t *)(ws + w.txt[1])};
    float *ref = (float *)(ws + w.ref);
    const uint16_t *tpos = text_pos_embed ? text_pos_embed : (uint16_t *)(ws + w.tpos);
    // every block's own refusals, on the operands it will get, before anything is enqueued
    for (int l = 0; l < NL; ++l) {
        const bool last = l + 1 == NL;
        TRY(fusion_check_call(&d->fusion[l], l == 0 ? vision : vis[1], l == 0 ? text : txt[1], B, S, Lt, vis[0], txt[0], ws + w.layer, w.layer_bytes));
        TRY(enh_check_call(&d->enhancer[l], txt[0], tpos, n_masks, B, Lt, last ? out_text : txt[1], ws + w.layer, w.layer_bytes));
        TRY(enc_layer_check_call(&d->deformable[l], vis[0], vision_pos, nullptr, ref, spatial_shapes, level_start_index, B, S,
                                 last ? out_vision : vis[1], nullptr, ws + w.layer, w.layer_bytes));
    }
    ++g_enc_calls;
    hipStream_t st = (hipStream_t)stream;

    // once per call: get_reference_points (:1672) and the text position embedding, the same tensor in every layer (:1260-1262)
    TRY(encoder_refpoints_launch(spatial_shapes, level_start_index, valid_ratios, Rv, S, L, ref, st));
    if (!text_pos_embed) TRY(text_pos_embed_launch(text_positions, d->dim_t, Rt, Lt, C, (uint16_t *)(ws + w.tpos), C, st));
    const uint16_t *xv = vision, *xt = text;
    for (int l = 0; l < NL; ++l) {
        const bool last = l + 1 == NL;
        uint16_t *yv = last ? out_vision : vis[1], *yt = last ? out_text : txt[1];
        // :1264-1269
        TRY(fusion_run(&d->fusion[l], xv, xt, vision_padding_mask, text_padding_mask, B, S, Lt, vis[0], txt[0], ws + w.layer, st));
        // :1271-1275
        TRY(enh_run(&d->enhancer[l], txt[0], tpos, text_self_attn_mask, n_masks, B, Lt, yt, ws + w.layer, st));
        // :1277-1284
        TRY(enc_layer_run(&d->deformable[l], vis[0], vision_pos, nullptr, ref, vision_padding_mask, spatial_shapes, level_start_index, B, S, yv,
                          nullptr, ws + w.layer, st));
        xv = yv; xt = yt;
    }
    return VLLM_OK;
}
