// The FUSION LAYER of Grounding-DINO for bf16 modules at inference: pre-LayerNorm, bi-directional image <-> text attention, layer scale.
// Reference: GroundingDinoBiMultiHeadAttention / GroundingDinoFusionLayer  grounding_dino/modeling_ov_grounding_dino_mask_dn.py:860-1101.
//
// One call, one stream, a caller workspace.  The launches, in order (header section f2f):
//   two LayerNorms; four projection GEMMs (bias); the text -> image attention (keys split, xattn.hip); the image -> text attention
//   (one split), whose output takes the memory of values_vision_proj's, which the attention in front has read; the two output
//   projections with the residual and the layer scale in their epilogue.
// The refusals, the workspace size and the launches are functions of their own (gdino_encoder.hpp): the public entry and the encoder's
// one call (gdino_encoder.hip) run the same statements.  Host code only.
#include <math.h>
#include "common.hpp"
#include "orchestrate.hpp"
#include "mha_core.hpp"
#include "gdino_encoder.hpp"

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

}  // namespace

int fusion_check_desc(const VllmFusionLayerDesc *d)
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

int fusion_check_sizes(const VllmFusionLayerDesc *d, int B, int S, int Lt)
{
    VLLM_REQUIRE(B >= 0 && S >= 0 && Lt >= 0 && (long)B * S * d->embed_dim * 2 < (1L << 31) && (long)B * Lt * d->embed_dim * 2 < (1L << 31),
                 "%s: B=%d S=%d Lt=%d (B, S, Lt >= 0; B S embed_dim 2 and B Lt embed_dim 2 below 2^31)", WHO, B, S, Lt);
    VLLM_REQUIRE((long)B * S == 0 || Lt >= 1, "%s: Lt=%d (at least one text token)", WHO, Lt);
    return VLLM_OK;
}

long fusion_ws_bytes(const VllmFusionLayerDesc *d, int B, int S, int Lt) { return fus_ws(d, B, S, Lt).total; }

namespace {

// the pieces of the workspace and the attention launches' operands, as the checks and the launches both see them
struct FusCall {
    uint16_t *vn, *tn, *qv, *vv, *kt, *vt, *at, *av;
    char *xa;
    long xa_bytes;
    AttnOperand Qv, Vv, Av, Kt, Vt, At;
};
FusCall fus_call(const VllmFusionLayerDesc *d, const FusWs &w, void *workspace, long S, long Lt)
{
    char *ws = (char *)workspace;
    const int E = d->embed_dim;
    FusCall c;
    c.vn = (uint16_t *)(ws + w.vn); c.tn = (uint16_t *)(ws + w.tn); c.qv = (uint16_t *)(ws + w.qv); c.vv = (uint16_t *)(ws + w.vv);
    c.kt = (uint16_t *)(ws + w.kt); c.vt = (uint16_t *)(ws + w.vt); c.at = (uint16_t *)(ws + w.at); c.av = c.vv;
    c.xa = ws + w.xa; c.xa_bytes = w.xa_bytes;
    const long sE = S * E, tE = Lt * E;
    c.Qv = {c.qv, sE, E}; c.Vv = {c.vv, sE, E}; c.Av = {c.av, sE, E}; c.Kt = {c.kt, tE, E}; c.Vt = {c.vt, tE, E}; c.At = {c.at, tE, E};
    return c;
}

long g_calls = 0;

}  // namespace

int fusion_check_call(const VllmFusionLayerDesc *d, const uint16_t *vision, const uint16_t *text, int B, int S, int Lt, const uint16_t *out_vision,
                      const uint16_t *out_text, const void *workspace, long workspace_bytes)
{
    VLLM_REQUIRE(vision && text && out_vision && out_text, "%s: null pointer (vision / text / out_vision / out_text)", WHO);
    VLLM_REQUIRE(aligned16(vision) && aligned16(text) && aligned16(out_vision) && aligned16(out_text),
                 "%s: misaligned vision / text / out_vision / out_text (16 bytes)", WHO);
    const uint16_t *const *wp = &d->vision_norm_w;
    for (int i = 0; i < 18; ++i) VLLM_REQUIRE(aligned16(wp[i]), "%s: misaligned weight, bias or parameter (16 bytes)", WHO);
    const int C = d->d_model, H = d->n_heads, D = d->embed_dim / H;
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
    const FusCall c = fus_call(d, w, const_cast<void *>(workspace), S, Lt);
    // the attention launches' own gates, before anything is enqueued
    TRY(xattn_fwd_check(c.Kt, c.Qv, c.Vv, c.At, B, Lt, S, H, D, c.xa, c.xa_bytes));
    TRY(xattn_fwd_check(c.Qv, c.Kt, c.Vt, c.Av, B, S, Lt, H, D, c.xa, c.xa_bytes));
    return VLLM_OK;
}

int fusion_run(const VllmFusionLayerDesc *d, const uint16_t *vision, const uint16_t *text, const uint8_t *vision_padding_mask,
               const uint8_t *text_padding_mask, int B, int S, int Lt, uint16_t *out_vision, uint16_t *out_text, void *workspace, hipStream_t st)
{
    const int C = d->d_model, E = d->embed_dim, H = d->n_heads, D = E / H;
    const long Rv = (long)B * S, Rt = (long)B * Lt;
    const FusCall c = fus_call(d, fus_ws(d, B, S, Lt), workspace, S, Lt);
    const float scale = 1.0f / sqrtf((float)D);
    // 1. pre layer norm (:1090-1091)
    TRY(norm_bf16_launch(false, vision, C, d->vision_norm_w, d->vision_norm_b, c.vn, C, Rv, C, d->vision_norm_eps, st));
    TRY(norm_bf16_launch(false, text, C, d->text_norm_w, d->text_norm_b, c.tn, C, Rt, C, d->text_norm_eps, st));
    // 2. the four projections (:927-937)
    TRY(gemm(st, EPI_BIAS, c.vn, C, d->vision_proj_w, C, d->vision_proj_b, c.qv, E, (int)Rv, E, C));
    TRY(gemm(st, EPI_BIAS, c.vn, C, d->values_vision_proj_w, C, d->values_vision_proj_b, c.vv, E, (int)Rv, E, C));
    TRY(gemm(st, EPI_BIAS, c.tn, C, d->text_proj_w, C, d->text_proj_b, c.kt, E, (int)Rt, E, C));
    TRY(gemm(st, EPI_BIAS, c.tn, C, d->values_text_proj_w, C, d->values_text_proj_b, c.vt, E, (int)Rt, E, C));
    // 3. text -> image (:958-971, :983): the keys are the image tokens, split by the plan
    TRY(xattn_fwd_launch(c.Kt, c.Qv, c.Vv, c.At, vision_padding_mask, B, Lt, S, H, D, scale, c.xa, c.xa_bytes, st));
    // 4. image -> text (:973-977, :982), into the memory of values_vision_proj's output
    TRY(xattn_fwd_launch(c.Qv, c.Kt, c.Vt, c.Av, text_padding_mask, B, S, Lt, H, D, scale, c.xa, c.xa_bytes, st));
    // 5. output projections, layer scale, residual on the NORMALISED inputs (:1003-1004, :1098-1099)
    TRY(gemm(st, EPI_RESIDUAL, c.av, E, d->out_vision_proj_w, E, d->out_vision_proj_b, out_vision, C, (int)Rv, C, E, d->vision_param, c.vn, C));
    return gemm(st, EPI_RESIDUAL, c.at, E, d->out_text_proj_w, E, d->out_text_proj_b, out_text, C, (int)Rt, C, E, d->text_param, c.tn, C);
}

}  // namespace vllm

using namespace vllm;

static_assert(sizeof(VllmFusionLayerDesc) == 3 * sizeof(int32_t) + 2 * sizeof(float) + 4 + 18 * sizeof(void *), "VllmFusionLayerDesc: 18 pointers behind five scalars");

extern "C" unsigned long vllm_fusion_layer_desc_sizeof(void) { return sizeof(VllmFusionLayerDesc); }
extern "C" long vllm_fusion_layer_calls(void) { return g_calls; }

extern "C" long vllm_fusion_layer_workspace_bytes(const VllmFusionLayerDesc *d, int B, int S, int Lt)
{
    if (fusion_check_desc(d) != VLLM_OK || fusion_check_sizes(d, B, S, Lt) != VLLM_OK) return -1;
    if ((long)B * S == 0) return 0;
    return fusion_ws_bytes(d, B, S, Lt);
}

extern "C" int vllm_fusion_layer_forward(const VllmFusionLayerDesc *d, const uint16_t *vision, const uint16_t *text,
                                         const uint8_t *vision_padding_mask, const uint8_t *text_padding_mask, int B, int S, int Lt,
                                         uint16_t *out_vision, uint16_t *out_text, void *workspace, long workspace_bytes,
                                         vllm_stream_t stream)
{
    TRY(fusion_check_desc(d));
    TRY(fusion_check_sizes(d, B, S, Lt));
    if ((long)B * S == 0) return VLLM_OK;
    TRY(fusion_check_call(d, vision, text, B, S, Lt, out_vision, out_text, workspace, workspace_bytes));
    ++g_calls;
    return fusion_run(d, vision, text, vision_padding_mask, text_padding_mask, B, S, Lt, out_vision, out_text, workspace, (hipStream_t)stream);
}
