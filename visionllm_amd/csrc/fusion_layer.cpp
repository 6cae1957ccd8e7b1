// The FUSION LAYER of Grounding-DINO for bf16 modules at inference: pre-LayerNorm, bi-directional image <-> text attention, layer scale.
// Reference: GroundingDinoBiMultiHeadAttention / GroundingDinoFusionLayer  grounding_dino/modeling_ov_grounding_dino_mask_dn.py:860-1101.
//
// One call, one stream, a caller workspace.  The launches, in order (header section f2f):
//   two LayerNorms; four projection GEMMs (bias); the text -> image attention (keys split, xattn.hip); the image -> text attention
//   (one split), whose output takes the memory of values_vision_proj's, which the attention in front has read; the two output
//   projections with the residual and the layer scale in their epilogue.
// Host code only.
#include <math.h>
#include "common.hpp"
#include "orchestrate.hpp"
#include "mha_core.hpp"

namespace vllm {
namespace {

const char *const WHO = "fusion_layer";

struct FusWs {
    long vn, tn, qv, vv, kt, vt, at, xa, total;   // normalised inputs; the four projections (vv later: the image side's attention output); text side's attention output; partials
    long xa_bytes;
};
FusWs fus_ws(const VllmFusionLayerDesc *d, long B, long S, long Lt)
{
    const long C = d->d_model, E = d->embed_dim;
    FusWs w;
    Carver cv;
    w.vn = cv.take(B * S * C * 2);
    w.tn = cv.take(B * Lt * C * 2);
    w.qv = cv.take(B * S * E * 2);
    w.vv = cv.take(B * S * E * 2);
    w.kt = cv.take(B * Lt * E * 2);
    w.vt = cv.take(B * Lt * E * 2);
    w.at = cv.take(B * Lt * E * 2);
    // the partials of whichever direction the plan splits (text -> image at the workload's shape); the two run one behind the other
    const long x1 = xattn_ws_bytes((int)B, (int)Lt, (int)S, d->n_heads, d->embed_dim / d->n_heads);
    const long x2 = xattn_ws_bytes((int)B, (int)S, (int)Lt, d->n_heads, d->embed_dim / d->n_heads);
    w.xa_bytes = x1 > x2 ? x1 : x2;
    w.xa = cv.take(w.xa_bytes);
    w.total = cv.off;
    return w;
}

int fus_check_desc(const VllmFusionLayerDesc *d)
{
    VLLM_REQUIRE(d, "%s: null descriptor", WHO);
    VLLM_REQUIRE(d->d_model >= 64 && d->d_model <= 512 && d->d_model % 64 == 0, "%s: d_model=%d (a multiple of 64 in 64 .. 512)", WHO, d->d_model);
    VLLM_REQUIRE(d->n_heads >= 1 && d->n_heads <= 64 && d->embed_dim > 0 && d->embed_dim % d->n_heads == 0 &&
                     (d->embed_dim / d->n_heads == 128 || d->embed_dim / d->n_heads == 256),
                 "%s: embed_dim=%d n_heads=%d (head dim 128 or 256)", WHO, d->embed_dim, d->n_heads);
    VLLM_REQUIRE(d->vision_norm_eps >= 0.f && d->text_norm_eps >= 0.f, "%s: negative eps", WHO);
    const uint16_t *const *p = &d->vision_norm_w;
    for (int i = 0; i < 18; ++i) VLLM_REQUIRE(p[i], "%s: missing weights", WHO);
    return VLLM_OK;
}

int fus_check_sizes(const VllmFusionLayerDesc *d, int B, int S, int Lt)
{
    VLLM_REQUIRE(B >= 0 && S >= 0 && Lt >= 0 && (long)B * S * d->embed_dim * 2 < (1L << 31) && (long)B * Lt * d->embed_dim * 2 < (1L << 31),
                 "%s: B=%d S=%d Lt=%d (B, S, Lt >= 0; B S embed_dim 2 and B Lt embed_dim 2 below 2^31)", WHO, B, S, Lt);
    VLLM_REQUIRE((long)B * S == 0 || Lt >= 1, "%s: Lt=%d (at least one text token)", WHO, Lt);
    return VLLM_OK;
}

long g_calls = 0;

}  // namespace
}  // namespace vllm

using namespace vllm;

static_assert(sizeof(VllmFusionLayerDesc) == 3 * sizeof(int32_t) + 2 * sizeof(float) + 4 + 18 * sizeof(void *), "VllmFusionLayerDesc: 18 pointers behind five scalars");

extern "C" unsigned long vllm_fusion_layer_desc_sizeof(void) { return sizeof(VllmFusionLayerDesc); }
extern "C" long vllm_fusion_layer_calls(void) { return g_calls; }

extern "C" long vllm_fusion_layer_workspace_bytes(const VllmFusionLayerDesc *d, int B, int S, int Lt)
{
    if (fus_check_desc(d) != VLLM_OK || fus_check_sizes(d, B, S, Lt) != VLLM_OK) return -1;
    if ((long)B * S == 0) return 0;
    return fus_ws(d, B, S, Lt).total;
}

extern "C" int vllm_fusion_layer_forward(const VllmFusionLayerDesc *d, const uint16_t *vision, const uint16_t *text,
                                         const uint8_t *vision_padding_mask, const uint8_t *text_padding_mask, int B, int S, int Lt,
                                         uint16_t *out_vision, uint16_t *out_text, void *workspace, long workspace_bytes,
                                         vllm_stream_t stream)
{
    TRY(fus_check_desc(d));
    TRY(fus_check_sizes(d, B, S, Lt));
    if ((long)B * S == 0) return VLLM_OK;
    VLLM_REQUIRE(vision && text && out_vision && out_text, "%s: null pointer (vision / text / out_vision / out_text)", WHO);
    VLLM_REQUIRE(aligned16(vision) && aligned16(text) && aligned16(out_vision) && aligned16(out_text),
                 "%s: misaligned vision / text / out_vision / out_text (16 bytes)", WHO);
    const uint16_t *const *wp = &d->vision_norm_w;
    for (int i = 0; i < 18; ++i) VLLM_REQUIRE(aligned16(wp[i]), "%s: misaligned weight, bias or parameter (16 bytes)", WHO);
    const int C = d->d_model, E = d->embed_dim, H = d->n_heads, D = E / H;
    const long Rv = (long)B * S, Rt = (long)B * Lt, vbytes = Rv * C * 2, tbytes = Rt * C * 2;
    VLLM_REQUIRE(!ranges_overlap(out_vision, vbytes, vision, vbytes) && !ranges_overlap(out_vision, vbytes, text, tbytes) &&
                     !ranges_overlap(out_text, tbytes, vision, vbytes) && !ranges_overlap(out_text, tbytes, text, tbytes) &&
                     !ranges_overlap(out_vision, vbytes, out_text, tbytes),
                 "%s: out_vision / out_text overlap an input or each other", WHO);
    const FusWs w = fus_ws(d, B, S, Lt);
    VLLM_REQUIRE(workspace, "%s: null workspace (%ld bytes)", WHO, w.total);
    VLLM_REQUIRE(aligned16(workspace), "%s: misaligned workspace (16 bytes)", WHO);
    VLLM_REQUIRE(workspace_bytes >= w.total, "%s: workspace too small (%ld < %ld bytes)", WHO, workspace_bytes, w.total);
    VLLM_REQUIRE(!ranges_overlap(workspace, w.total, vision, vbytes) && !ranges_overlap(workspace, w.total, text, tbytes) &&
                     !ranges_overlap(workspace, w.total, out_vision, vbytes) && !ranges_overlap(workspace, w.total, out_text, tbytes),
                 "%s: workspace overlaps an operand", WHO);
    char *ws = (char *)workspace;
    uint16_t *vn = (uint16_t *)(ws + w.vn), *tn = (uint16_t *)(ws + w.tn), *qv = (uint16_t *)(ws + w.qv), *vv = (uint16_t *)(ws + w.vv);
    uint16_t *kt = (uint16_t *)(ws + w.kt), *vt = (uint16_t *)(ws + w.vt), *at = (uint16_t *)(ws + w.at), *av = vv;
    const long sE = (long)S * E, tE = (long)Lt * E;
    const AttnOperand Qv = {qv, sE, E}, Vv = {vv, sE, E}, Av = {av, sE, E}, Kt = {kt, tE, E}, Vt = {vt, tE, E}, At = {at, tE, E};
    // the attention launches' own gates, before anything is enqueued
    TRY(xattn_fwd_check(Kt, Qv, Vv, At, B, Lt, S, H, D, ws + w.xa, w.xa_bytes));
    TRY(xattn_fwd_check(Qv, Kt, Vt, Av, B, S, Lt, H, D, ws + w.xa, w.xa_bytes));
    ++g_calls;
    hipStream_t st = (hipStream_t)stream;
    const float scale = 1.0f / sqrtf((float)D);
    // 1. pre layer norm (:1090-1091)
    TRY(norm_bf16_launch(false, vision, C, d->vision_norm_w, d->vision_norm_b, vn, C, Rv, C, d->vision_norm_eps, st));
    TRY(norm_bf16_launch(false, text, C, d->text_norm_w, d->text_norm_b, tn, C, Rt, C, d->text_norm_eps, st));
    // 2. the four projections (:927-937)
    TRY(gemm(st, EPI_BIAS, vn, C, d->vision_proj_w, C, d->vision_proj_b, qv, E, (int)Rv, E, C));
    TRY(gemm(st, EPI_BIAS, vn, C, d->values_vision_proj_w, C, d->values_vision_proj_b, vv, E, (int)Rv, E, C));
    TRY(gemm(st, EPI_BIAS, tn, C, d->text_proj_w, C, d->text_proj_b, kt, E, (int)Rt, E, C));
    TRY(gemm(st, EPI_BIAS, tn, C, d->values_text_proj_w, C, d->values_text_proj_b, vt, E, (int)Rt, E, C));
    // 3. text -> image (:958-971, :983): the keys are the image tokens, split by the plan
    TRY(xattn_fwd_launch(Kt, Qv, Vv, At, vision_padding_mask, B, Lt, S, H, D, scale, ws + w.xa, w.xa_bytes, st));
    // 4. image -> text (:973-977, :982), into the memory of values_vision_proj's output
    TRY(xattn_fwd_launch(Qv, Kt, Vt, Av, text_padding_mask, B, S, Lt, H, D, scale, ws + w.xa, w.xa_bytes, st));
    // 5. output projections, layer scale, residual on the NORMALISED inputs (:1003-1004, :1098-1099)
    TRY(gemm(st, EPI_RESIDUAL, av, E, d->out_vision_proj_w, E, d->out_vision_proj_b, out_vision, C, (int)Rv, C, E, d->vision_param, vn, C));
    return gemm(st, EPI_RESIDUAL, at, E, d->out_text_proj_w, E, d->out_text_proj_b, out_text, C, (int)Rt, C, E, d->text_param, tn, C);
}
