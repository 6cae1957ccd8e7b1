// The deformable DECODER LAYER of the detection and pose heads for bf16 modules at inference, as one call:
//   1. q = tgt + pos;  x = LN_sa(tgt + out_proj(MHA(q Wq, q Wk, tgt Wv, self_attn_mask)))
//   2. x = LN_text(x + out_proj_t(MHA((x + pos) Wq, text Wk, text Wv, text_key_padding_mask)))
//   3. x = LN_ca(x + cross_attn(x + pos, reference_points, memory, ...))
//   4. out = LN_ffn(x + fc2(act(fc1(x))))
// Reference: DeformableTransformerDecoderLayer.forward  unipose/modeling_unipose.py:3250-3323;
//            GroundingDinoDecoderLayer.forward          grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1332-1407.
//
// One call, one stream, a caller workspace.  The launches, in order (blocks 1 and 2 only where the descriptor has them):
//   add_bf16                 xp = tgt + pos, once: every later `x + pos` is the y_pos output of the LayerNorm in front of its reader
//   1. GEMM N = 2C on q with in_proj_w[0:2C] -> [q | k];  GEMM N = C on tgt with in_proj_w[2C:3C] -> v;  mha (mha.hip) on the slices;
//      out_proj with `tgt` added in its epilogue (EPI_RESIDUAL);  add_layernorm in place, y_pos -> xp
//   2. GEMM N = C on xp with in_proj_w[0:C] -> q;  GEMM N = 2C on memory_text with in_proj_w[C:3C] -> [k | v];  mha;  out_proj + residual;
//      add_layernorm in place, y_pos -> xp
//   3. the attention layer (msda_layer_run), whose output_proj adds x in its epilogue;  add_layernorm in place
//   4. fc1 + ReLU / GELU (EPI_RELU / EPI_GELU);  fc2 + residual;  add_layernorm -> out
// Weight slices are pointer offsets into the module's own in_proj parameter: nothing is copied or repacked per call.
#include "common.hpp"
#include "orchestrate.hpp"
#include "msda_layer.hpp"
#include "deform_blocks.hpp"
#include "deform_decoder_layer.hpp"
#include "mha_core.hpp"

namespace vllm {
namespace {

struct DecWs {
    long xp, a, b, qk, v, ctx, tkv, h, attn, total;   // xp: x + pos; a, b: the running x, ping-pong; qk [R, 2C]; v [R, C] (block 2: its q);
};                                                    // ctx [R, C]; tkv [B Lt, 2C]; h [R, d_ffn]; attn: the attention layer's own
DecWs dec_ws(const VllmDeformDecLayerDesc *d, long B, long Lq, long Lt, long S)
{
    const long R = B * Lq, C = d->cross_attn.d_model, F = d->d_ffn;
    const bool mha = d->has_self_attn || d->has_text_attn;
    DecWs w;
    Carver cv;
    w.xp = cv.take(R * C * 2);
    w.a = cv.take(R * C * 2);
    w.b = cv.take(R * C * 2);
    w.qk = cv.take(d->has_self_attn ? R * 2 * C * 2 : 0);
    w.v = cv.take(mha ? R * C * 2 : 0);
    w.ctx = cv.take(mha ? R * C * 2 : 0);
    w.tkv = cv.take(d->has_text_attn ? B * Lt * 2 * C * 2 : 0);
    w.h = cv.take(R * F * 2);
    w.attn = cv.take(msda_layer_ws_bytes(&d->cross_attn, (int)B, (int)Lq, (int)S));
    w.total = cv.off;
    return w;
}

FfnBlock dec_ffn(const VllmDeformDecLayerDesc *d)
{
    return {d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, d->ffn_norm_w, d->ffn_norm_b, d->act, d->d_ffn, d->ffn_norm_eps};
}

long g_calls = 0;

}  // namespace

int dec_layer_check_desc(const VllmDeformDecLayerDesc *d)
{
    VLLM_REQUIRE(d, "deform_dec_layer: null descriptor");
    TRY(msda_layer_check_desc(&d->cross_attn));
    const VllmMsdaLayerDesc &at = d->cross_attn;
    const int C = at.d_model;
    VLLM_REQUIRE(C >= 64 && C <= 512 && C % 64 == 0, "deform_dec_layer: d_model=%d must be a multiple of 64 in 64 .. 512 (the LayerNorm kernel's rows)", C);
    TRY(ffn_check("deform_dec_layer", dec_ffn(d)));
    if (d->has_self_attn || d->has_text_attn)
        VLLM_REQUIRE(d->n_heads_sa >= 1 && C % d->n_heads_sa == 0 && (C / d->n_heads_sa == 32 || C / d->n_heads_sa == 64),
                     "deform_dec_layer: n_heads_sa=%d with d_model=%d (head dim 32 or 64)", d->n_heads_sa, C);
    VLLM_REQUIRE(d->sa_norm_eps >= 0.f && d->text_norm_eps >= 0.f && d->ca_norm_eps >= 0.f, "deform_dec_layer: negative eps");
    VLLM_REQUIRE(!d->has_self_attn || (d->sa_in_proj_w && d->sa_in_proj_b && d->sa_out_proj_w && d->sa_out_proj_b && d->sa_norm_w && d->sa_norm_b),
                 "deform_dec_layer: missing weights (self-attention)");
    VLLM_REQUIRE(!d->has_text_attn || (d->text_in_proj_w && d->text_in_proj_b && d->text_out_proj_w && d->text_out_proj_b && d->text_norm_w && d->text_norm_b),
                 "deform_dec_layer: missing weights (text attention)");
    VLLM_REQUIRE(d->ca_norm_w && d->ca_norm_b && at.value_proj_b && at.sampling_offsets_b && at.attention_weights_b && at.output_proj_b,
                 "deform_dec_layer: missing weights");
    return VLLM_OK;
}

int dec_layer_check_sizes(const VllmDeformDecLayerDesc *d, int B, int Lq, int Lt, int S)
{
    VLLM_REQUIRE(B >= 0 && Lq >= 0 && Lt >= 0 && S >= 0 && (long)B * Lq < (1L << 31) && (long)B * S < (1L << 31) && (long)B * Lt < (1L << 31),
                 "deform_dec_layer: B=%d Lq=%d Lt=%d S=%d (non-negative, B Lq, B Lt and B S below 2^31)", B, Lq, Lt, S);
    // (the GEMMs address an operand with 32-bit byte offsets)
    VLLM_REQUIRE((long)B * Lq * (d->d_ffn > 2 * d->cross_attn.d_model ? d->d_ffn : 2 * d->cross_attn.d_model) * 2 < (1L << 31),
                 "deform_dec_layer: B Lq=%ld rows of the widest intermediate reach 2^31 bytes", (long)B * Lq);
    VLLM_REQUIRE(!d->has_text_attn || (long)B * Lt * 2 * d->cross_attn.d_model * 2 < (1L << 31),
                 "deform_dec_layer: B Lt=%ld rows of the text's [k | v] reach 2^31 bytes", (long)B * Lt);
    return VLLM_OK;
}

long dec_layer_ws_bytes(const VllmDeformDecLayerDesc *d, int B, int Lq, int Lt, int S) { return dec_ws(d, B, Lq, Lt, S).total; }

// the pieces of the workspace and the attention blocks' shape, as the checks and the launches both see them
struct DecCall {
    uint16_t *xp, *bufa, *bufb, *qk, *vb, *ctx, *tkv, *h;
    char *attn;
    int H, D;
    AttnOperand sa_q, sa_k, sa_v;   // self-attention: q | k interleaved in qk [R, 2C], v in vb
    AttnOperand ta_q, ta_k, ta_v;   // text attention: q in vb, k | v interleaved in tkv [B Lt, 2C]
    AttnOperand ctx_o;              // both write ctx [R, C]
};
static DecCall dec_call(const VllmDeformDecLayerDesc *d, const DecWs &w, void *workspace, long Lq, long Lt)
{
    char *ws = (char *)workspace;
    const int C = d->cross_attn.d_model;
    DecCall c;
    c.xp = (uint16_t *)(ws + w.xp); c.bufa = (uint16_t *)(ws + w.a); c.bufb = (uint16_t *)(ws + w.b); c.qk = (uint16_t *)(ws + w.qk);
    c.vb = (uint16_t *)(ws + w.v); c.ctx = (uint16_t *)(ws + w.ctx); c.tkv = (uint16_t *)(ws + w.tkv); c.h = (uint16_t *)(ws + w.h);
    c.attn = ws + w.attn;
    c.H = d->n_heads_sa;
    c.D = d->has_self_attn || d->has_text_attn ? C / c.H : 32;
    c.sa_q = {c.qk, Lq * 2 * C, 2 * C}; c.sa_k = {c.qk + C, Lq * 2 * C, 2 * C}; c.sa_v = {c.vb, Lq * C, C};
    c.ta_q = {c.vb, Lq * C, C}; c.ta_k = {c.tkv, Lt * 2 * C, 2 * C}; c.ta_v = {c.tkv + C, Lt * 2 * C, 2 * C};
    c.ctx_o = {c.ctx, Lq * C, C};
    return c;
}

int dec_layer_check_call(const VllmDeformDecLayerDesc *d, const uint16_t *tgt, const uint16_t *query_pos, const float *reference_points,
                         const uint16_t *memory_text, const uint16_t *memory, const int64_t *spatial_shapes, const int64_t *level_start_index,
                         int B, int Lq, int Lt, int S, const uint16_t *out, const void *workspace, long workspace_bytes)
{
    const VllmMsdaLayerDesc &at = d->cross_attn;
    const bool sa = d->has_self_attn != 0, ta = d->has_text_attn != 0;
    VLLM_REQUIRE(S > 0 && (!ta || Lt > 0), "deform_dec_layer: S=%d Lt=%d (an empty memory or text)", S, Lt);
    VLLM_REQUIRE(tgt && reference_points && memory && spatial_shapes && level_start_index && out && (!ta || memory_text),
                 "deform_dec_layer: null pointer (tgt / reference_points / memory_text / memory / spatial_shapes / level_start_index / out)");
    VLLM_REQUIRE(aligned16(tgt) && aligned16(query_pos) && aligned16(memory_text) && aligned16(memory) && aligned16(out) &&
                     (reinterpret_cast<uintptr_t>(reference_points) & (at.ref_dim == 4 ? 15u : 7u)) == 0,
                 "deform_dec_layer: misaligned tgt / query_pos / memory_text / memory / out (16 bytes) or reference_points (8 bytes, 16 with ref_dim 4)");
    for (const uint16_t *p : {d->sa_in_proj_w, d->sa_in_proj_b, d->sa_out_proj_w, d->sa_out_proj_b, d->sa_norm_w, d->sa_norm_b, d->text_in_proj_w,
                              d->text_in_proj_b, d->text_out_proj_w, d->text_out_proj_b, d->text_norm_w, d->text_norm_b, d->ca_norm_w, d->ca_norm_b,
                              d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, d->ffn_norm_w, d->ffn_norm_b})
        VLLM_REQUIRE(aligned16(p), "deform_dec_layer: misaligned weight or bias (16 bytes)");
    for (const uint16_t *p : msda_weights(at)) VLLM_REQUIRE(aligned16(p), "deform_dec_layer: misaligned weight or bias (16 bytes)");
    const long R = (long)B * Lq;
    const int C = at.d_model;
    const long obytes = R * C * 2;
    VLLM_REQUIRE(!ranges_overlap(out, obytes, tgt, obytes) && !ranges_overlap(out, obytes, query_pos, obytes) &&
                     !ranges_overlap(out, obytes, memory, (long)B * S * C * 2) && !(ta && ranges_overlap(out, obytes, memory_text, (long)B * Lt * C * 2)),
                 "deform_dec_layer: out overlaps an input (tgt / query_pos / memory_text / memory)");
    const DecWs w = dec_ws(d, B, Lq, Lt, S);
    VLLM_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.total,
                 "deform_dec_layer: workspace too small (%ld < %ld bytes) or misaligned", workspace_bytes, w.total);
    const DecCall c = dec_call(d, w, const_cast<void *>(workspace), Lq, Lt);
    // the attention kernel's own gate, asked before anything is enqueued (dense slices of the buffers above: it cannot refuse them)
    if (sa) TRY(mha_fwd_check(c.sa_q, c.sa_k, c.sa_v, c.ctx_o, B, Lq, Lq, c.H, c.D));
    if (ta) TRY(mha_fwd_check(c.ta_q, c.ta_k, c.ta_v, c.ctx_o, B, Lq, Lt, c.H, c.D));
    return VLLM_OK;
}

int dec_layer_run(const VllmDeformDecLayerDesc *d, const uint16_t *tgt, const uint16_t *query_pos, const float *reference_points,
                  const uint8_t *self_attn_mask, const uint16_t *memory_text, const uint8_t *text_key_padding_mask, const uint16_t *memory,
                  const uint8_t *memory_padding_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int Lq, int Lt,
                  int S, uint16_t *out, void *workspace, hipStream_t st)
{
    const VllmMsdaLayerDesc &at = d->cross_attn;
    const bool sa = d->has_self_attn != 0, ta = d->has_text_attn != 0;
    const long R = (long)B * Lq;
    const int C = at.d_model;
    const DecCall c = dec_call(d, dec_ws(d, B, Lq, Lt, S), workspace, Lq, Lt);
    uint16_t *xp = c.xp, *bufa = c.bufa, *bufb = c.bufb, *qk = c.qk, *vb = c.vb, *ctx = c.ctx, *tkv = c.tkv;
    const float scale = 1.0f / sqrtf((float)c.D);

    // (the launchers without the public entries' checks: dec_layer_check_desc has C a multiple of 64 in 64 .. 512 and the norms' pointers,
    // dec_layer_check_call tgt / query_pos / out and every weight 16-byte aligned; x, y and xp are 256-byte aligned workspace, dense rows; R > 0)
    const uint16_t *cur = tgt;          // the running x
    const uint16_t *curp = tgt;         // x + pos
    if (query_pos) { TRY(add_launch(tgt, query_pos, xp, R * C, st)); curp = xp; }
    auto other = [&]() { return cur == bufa ? bufb : bufa; };
    // the tail of an attention block whose residual sum is in y: the LayerNorm in place, with x + pos for the block behind it
    auto finish_block = [&](uint16_t *y, const uint16_t *nw, const uint16_t *nb, float eps, bool want_pos) {
        const bool yp = want_pos && query_pos;
        TRY(add_layernorm_launch(y, C, nullptr, 0, nw, nb, y, C, yp ? query_pos : nullptr, C, yp ? xp : nullptr, C, R, C, eps, st));
        cur = y;
        if (want_pos) curp = query_pos ? xp : y;
        return VLLM_OK;
    };

    // 1. self-attention of the queries (modeling_unipose.py:3280-3284; ...mask_dn.py:1349-1356)
    if (sa) {
        TRY(gemm(st, EPI_BIAS, curp, C, d->sa_in_proj_w, C, d->sa_in_proj_b, qk, 2 * C, (int)R, 2 * C, C));
        TRY(gemm(st, EPI_BIAS, tgt, C, d->sa_in_proj_w + 2L * C * C, C, d->sa_in_proj_b + 2 * C, vb, C, (int)R, C, C));
        TRY(mha_fwd_launch(c.sa_q, c.sa_k, c.sa_v, c.ctx_o, self_attn_mask, nullptr, B, Lq, Lq, c.H, c.D, scale, st));
        uint16_t *y = other();
        TRY(gemm(st, EPI_RESIDUAL, ctx, C, d->sa_out_proj_w, C, d->sa_out_proj_b, y, C, (int)R, C, C, nullptr, cur, C));
        TRY(finish_block(y, d->sa_norm_w, d->sa_norm_b, d->sa_norm_eps, true));
    }
    // 2. text cross-attention (:3290-3294; :1361-1371)
    if (ta) {
        TRY(gemm(st, EPI_BIAS, curp, C, d->text_in_proj_w, C, d->text_in_proj_b, vb, C, (int)R, C, C));
        TRY(gemm(st, EPI_BIAS, memory_text, C, d->text_in_proj_w + (long)C * C, C, d->text_in_proj_b + C, tkv, 2 * C, B * Lt, 2 * C, C));
        TRY(mha_fwd_launch(c.ta_q, c.ta_k, c.ta_v, c.ctx_o, nullptr, text_key_padding_mask, B, Lq, Lt, c.H, c.D, scale, st));
        uint16_t *y = other();
        TRY(gemm(st, EPI_RESIDUAL, ctx, C, d->text_out_proj_w, C, d->text_out_proj_b, y, C, (int)R, C, C, nullptr, cur, C));
        TRY(finish_block(y, d->text_norm_w, d->text_norm_b, d->text_norm_eps, true));
    }
    // 3. deformable cross-attention over the memory (:3303-3309; :1377-1391): the residual goes into output_proj's epilogue
    {
        uint16_t *y = other();
        TRY(msda_layer_run(&at, curp, reference_points, memory, memory_padding_mask, spatial_shapes, level_start_index, B, Lq, S, y,
                           msda_layer_bufs(&at, c.attn, B, Lq, S), nullptr, st, cur));
        TRY(finish_block(y, d->ca_norm_w, d->ca_norm_b, d->ca_norm_eps, false));
    }
    // 4. FFN (:3241-3248; :1394-1400), the whole intermediate at once
    return ffn_block_run(st, dec_ffn(d), cur, R, C, c.h, R, other(), out, nullptr, nullptr);
}

}  // namespace vllm

using namespace vllm;

extern "C" unsigned long vllm_deform_dec_layer_desc_sizeof(void) { return sizeof(VllmDeformDecLayerDesc); }
extern "C" long vllm_deform_dec_layer_calls(void) { return g_calls; }

extern "C" long vllm_deform_dec_layer_workspace_bytes(const VllmDeformDecLayerDesc *d, int B, int Lq, int Lt, int S)
{
    if (dec_layer_check_desc(d) != VLLM_OK || dec_layer_check_sizes(d, B, Lq, Lt, S) != VLLM_OK) return -1;
    if ((long)B * Lq == 0) return 0;
    return dec_layer_ws_bytes(d, B, Lq, Lt, S);
}

extern "C" int vllm_deform_dec_layer_forward(const VllmDeformDecLayerDesc *d, const uint16_t *tgt, const uint16_t *query_pos,
                                             const float *reference_points, const uint8_t *self_attn_mask, const uint16_t *memory_text,
                                             const uint8_t *text_key_padding_mask, const uint16_t *memory, const uint8_t *memory_padding_mask,
                                             const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int Lq, int Lt, int S,
                                             uint16_t *out, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    TRY(dec_layer_check_desc(d));
    TRY(dec_layer_check_sizes(d, B, Lq, Lt, S));
    if ((long)B * Lq == 0) return VLLM_OK;
    TRY(dec_layer_check_call(d, tgt, query_pos, reference_points, memory_text, memory, spatial_shapes, level_start_index, B, Lq, Lt, S, out,
                             workspace, workspace_bytes));
    ++g_calls;
    return dec_layer_run(d, tgt, query_pos, reference_points, self_attn_mask, memory_text, text_key_padding_mask, memory, memory_padding_mask,
                         spatial_shapes, level_start_index, B, Lq, Lt, S, out, workspace, (hipStream_t)stream);
}
