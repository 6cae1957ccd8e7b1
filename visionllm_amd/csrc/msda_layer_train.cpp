// Training the deformable-attention layer behind the C ABI (MSDeformAttn.forward unipose/ops/modules/ms_deform_attn.py:83-145 and its
// mmcv / Grounding-DINO twins; the forward pass is msda_layer.hip's, statement for statement).
//   forward_train: msda_layer_run with the tensors the backward needs in the caller's `saved` memory instead of scratch --
//       saved: [value fp32 | bf16][loc fp32][attw fp32][opout bf16], every piece rounded up to 256 bytes;  workspace: [opout fp32]
//   backward, from grad_out g [R, C] (R = B Lq rows):
//       dW_o = g^T opout, db_o = colsum g;  gop = g W_o (fp32)                                  gemm_wgrad; bf16 GEMM on W_o^T, EPI_F32
//       grad_value, grad_loc, grad_attw = operator'(value, loc, attw; gop)                      vllm_msda_backward_f32 (a bf16-saved value widened first)
//       dq [R, Npad] bf16 = [grad_loc (sx, sy) | softmax'(attw; grad_attw) | 0]                 msda_prep_bwd_kernel
//       grad_query = dq W_cat;  dW_cat = dq^T query, db_cat = colsum dq                         W_cat [Npad, C] = [W_offsets; W_logits; 0] in the workspace
//       gv [B S, C] bf16 = grad_value, rows of padded keys zero                                 f32_to_bf16_masked_kernel
//       dW_v = gv^T input_flatten, db_v = colsum gv;  grad_input_flatten = gv W_v
//   Npad = 3 M L P rounded up to 64: the two query linears share one input-gradient and one weight-gradient GEMM, and M L P = 96 (the
//   3-level pixel decoder) meets gemm_wgrad's multiple-of-64 rule.  A NULL gradient pointer skips that product and everything only it needed.
// No allocation, no synchronisation, one stream; the workspace is the caller's.
#include <algorithm>
#include "orchestrate.hpp"
#include "msda_layer.hpp"

using namespace vllm;

namespace {
struct Dims { int C, M, L, P, D, MLP, Npad; long R, VS; };   // R query rows, VS value rows

int check_layer(const VllmMsdaLayerDesc *d, int B, int Lq, int S, Dims *o, const char *who)
{
    TRY(msda_layer_check_desc(d));
    VLLM_REQUIRE(B >= 0 && Lq >= 0 && S >= 0, "%s: negative size", who);
    VLLM_REQUIRE((long)B * S < (1L << 31) && (long)B * Lq < (1L << 31), "%s: too many rows for one launch", who);
    const long mlp = (long)d->n_heads * d->n_levels * d->n_points;
    VLLM_REQUIRE(mlp < (1L << 24), "%s: heads * levels * points = %ld", who, mlp);
    o->C = d->d_model; o->M = d->n_heads; o->L = d->n_levels; o->P = d->n_points; o->D = o->C / o->M; o->MLP = (int)mlp;
    o->Npad = (int)((3 * mlp + 63) / 64 * 64);
    o->R = (long)B * Lq; o->VS = (long)B * S;
    return VLLM_OK;
}

struct Saved { long value, loc, attw, opb, total; };
Saved saved_layout(const Dims &q)
{
    Saved s;
    Carver cv;
    s.value = cv.take(q.VS * q.C * 4);   // sized for fp32; a bf16 value uses the first half
    s.loc = cv.take(q.R * q.MLP * 2 * 4);
    s.attw = cv.take(q.R * q.MLP * 4);
    s.opb = cv.take(q.R * q.C * 2);
    s.total = cv.off;
    return s;
}

// forward: [opout]; backward: [wt][gop][vwide][gv][gl][gw][dq][wcat][dwcat][dbcat][gv16][wg]
struct Ws { long wt, gop, vwide, gv, gl, gw, dq, wcat, dwcat, dbcat, gv16, wg, wg_bytes, total; };
Ws ws_layout(const VllmMsdaLayerDesc *d, const Dims &q, int Lq, int S)
{
    const long C = q.C, N = q.Npad;
    Ws w;
    Carver cv;
    w.wt = cv.take(std::max(C, N) * C * 2);                                   // W^T of the input-gradient GEMM at hand
    w.gop = cv.take(q.R * C * 4);                                            // the operator's grad_output
    w.vwide = cv.take(msda_layer_value_may_be_bf16(d, Lq, S) ? q.VS * C * 4 : 0);   // a bf16-saved value, widened
    w.gv = cv.take(q.VS * C * 4);
    w.gl = cv.take(q.R * q.MLP * 2 * 4);
    w.gw = cv.take(q.R * q.MLP * 4);
    w.dq = cv.take(q.R * N * 2);
    w.wcat = cv.take(N * C * 2);
    w.dwcat = cv.take(N * C * 2);
    w.dbcat = cv.take(N * 2);
    w.gv16 = cv.take(q.VS * C * 2);
    const long wg = std::max({gemm_wgrad_workspace_bytes((int)q.R, (int)C, (int)C), gemm_wgrad_workspace_bytes((int)q.R, (int)N, (int)C),
                              gemm_wgrad_workspace_bytes((int)q.VS, (int)C, (int)C)});
    w.wg_bytes = std::max(0L, wg);
    w.wg = cv.take(w.wg_bytes);
    w.total = cv.off;
    return w;
}

bool aligned_to(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int check_operands(const VllmMsdaLayerDesc *d, const uint16_t *query, const float *ref, const uint16_t *x, const int64_t *shapes,
                   const int64_t *lsi, const void *saved, long saved_bytes, long need, const char *who)
{
    VLLM_REQUIRE(query && ref && x && shapes && lsi, "%s: null pointer", who);
    VLLM_REQUIRE(aligned16(query) && aligned16(x) && aligned_to(ref, d->ref_dim == 4 ? 16 : 8),
                 "%s: query and input_flatten must be 16-byte aligned, reference_points %d-byte", who, d->ref_dim == 4 ? 16 : 8);
    const void *ps[] = {d->value_proj_w, d->value_proj_b, d->sampling_offsets_w, d->sampling_offsets_b, d->attention_weights_w,
                        d->attention_weights_b, d->output_proj_w, d->output_proj_b};
    for (const void *p : ps) VLLM_REQUIRE(p && aligned16(p), "%s: weights and biases must be 16-byte aligned device pointers", who);
    VLLM_REQUIRE(saved && aligned16(saved) && saved_bytes >= need, "%s: saved memory too small (%ld < %ld bytes) or misaligned", who, saved_bytes, need);
    return VLLM_OK;
}

int copy_d2d(void *dst, const void *src, long bytes, hipStream_t st, const char *who)
{
    VLLM_REQUIRE(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, st) == hipSuccess, "%s: device copy failed", who);
    return VLLM_OK;
}
int zero_bytes(void *p, long bytes, hipStream_t st, const char *who)
{
    if (bytes > 0) VLLM_REQUIRE(hipMemsetAsync(p, 0, (size_t)bytes, st) == hipSuccess, "%s: memset failed", who);
    return VLLM_OK;
}
}  // namespace

extern "C" int vllm_msda_layer_grads_sizeof(void) { return (int)sizeof(VllmMsdaLayerGrads); }

extern "C" long vllm_msda_layer_saved_bytes(const VllmMsdaLayerDesc *d, int B, int Lq, int S)
{
    Dims q;
    if (check_layer(d, B, Lq, S, &q, "msda_layer_saved_bytes") != VLLM_OK) return -1;
    return saved_layout(q).total;
}

extern "C" long vllm_msda_layer_forward_train_workspace_bytes(const VllmMsdaLayerDesc *d, int B, int Lq, int S)
{
    Dims q;
    if (check_layer(d, B, Lq, S, &q, "msda_layer_forward_train_workspace_bytes") != VLLM_OK) return -1;
    return align256(q.R * q.C * 4);
}

extern "C" long vllm_msda_layer_backward_workspace_bytes(const VllmMsdaLayerDesc *d, int B, int Lq, int S)
{
    Dims q;
    if (check_layer(d, B, Lq, S, &q, "msda_layer_backward_workspace_bytes") != VLLM_OK) return -1;
    return ws_layout(d, q, Lq, S).total;
}

extern "C" int vllm_msda_layer_forward_train(const VllmMsdaLayerDesc *d, const uint16_t *query, const float *ref,
                                             const uint16_t *input_flatten, const uint8_t *padding_mask, const int64_t *shapes,
                                             const int64_t *lsi, int B, int Lq, int S, uint16_t *out, void *saved, long saved_bytes,
                                             int *value_is_bf16, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    const char *who = "msda_layer_forward_train";
    Dims q;
    TRY(check_layer(d, B, Lq, S, &q, who));
    if (q.R == 0) {
        if (value_is_bf16) *value_is_bf16 = 0;
        return VLLM_OK;
    }
    VLLM_REQUIRE(S > 0, "%s: empty value", who);
    const Saved s = saved_layout(q);
    TRY(check_operands(d, query, ref, input_flatten, shapes, lsi, saved, saved_bytes, s.total, who));
    VLLM_REQUIRE(out && aligned16(out), "%s: out must be a 16-byte aligned device pointer", who);
    const long need = align256(q.R * q.C * 4);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= need, "%s: workspace too small (%ld < %ld bytes) or misaligned", who, ws_bytes, need);
    char *sv = (char *)saved;
    const MsdaLayerBufs b = {(float *)(sv + s.value), (float *)(sv + s.loc), (float *)(sv + s.attw), (float *)workspace, (uint16_t *)(sv + s.opb)};
    return msda_layer_run(d, query, ref, input_flatten, padding_mask, shapes, lsi, B, Lq, S, out, b, value_is_bf16, (hipStream_t)stream);
}

extern "C" int vllm_msda_layer_backward(const VllmMsdaLayerDesc *d, const uint16_t *query, const float *ref, const uint16_t *input_flatten,
                                        const uint8_t *padding_mask, const int64_t *shapes, const int64_t *lsi, int B, int Lq, int S,
                                        const void *saved, long saved_bytes, int value_is_bf16, const uint16_t *grad_out,
                                        uint16_t *grad_query, uint16_t *grad_input_flatten, const VllmMsdaLayerGrads *grads,
                                        void *workspace, long ws_bytes, vllm_stream_t stream)
{
    const char *who = "msda_layer_backward";
    Dims q;
    TRY(check_layer(d, B, Lq, S, &q, who));
    VLLM_REQUIRE(grads, "%s: null gradient table", who);
    const VllmMsdaLayerGrads &g = *grads;
    VLLM_REQUIRE((!g.value_proj_b || g.value_proj_w) && (!g.sampling_offsets_b || g.sampling_offsets_w) &&
                 (!g.attention_weights_b || g.attention_weights_w) && (!g.output_proj_b || g.output_proj_w),
                 "%s: a bias gradient comes out of its weight gradient's launch (pass both)", who);
    const void *gp[] = {grad_query, grad_input_flatten, g.value_proj_w, g.value_proj_b, g.sampling_offsets_w, g.sampling_offsets_b,
                        g.attention_weights_w, g.attention_weights_b, g.output_proj_w, g.output_proj_b};
    for (const void *p : gp) VLLM_REQUIRE(aligned16(p), "%s: gradients must be 16-byte aligned", who);
    VLLM_REQUIRE(value_is_bf16 == 0 || (value_is_bf16 == 1 && msda_layer_value_may_be_bf16(d, Lq, S)),
                 "%s: value_is_bf16 = %d is not what forward_train reports for these sizes", who, value_is_bf16);
    hipStream_t st = (hipStream_t)stream;
    const int C = q.C, M = q.M, L = q.L, P = q.P, MLP = q.MLP, N = q.Npad;
    const long R = q.R, VS = q.VS;
    if (R == 0) {   // no queries: every parameter gradient is an empty sum, and so is grad_input_flatten
        return zero_bf16(st, who, {{grad_input_flatten, VS * C}, {g.value_proj_w, (long)C * C}, {g.value_proj_b, C},
                                   {g.sampling_offsets_w, 2L * MLP * C}, {g.sampling_offsets_b, 2L * MLP}, {g.attention_weights_w, (long)MLP * C},
                                   {g.attention_weights_b, MLP}, {g.output_proj_w, (long)C * C}, {g.output_proj_b, C}});
    }
    VLLM_REQUIRE(S > 0, "%s: empty value", who);
    const Saved s = saved_layout(q);
    TRY(check_operands(d, query, ref, input_flatten, shapes, lsi, saved, saved_bytes, s.total, who));
    VLLM_REQUIRE(grad_out && aligned16(grad_out), "%s: grad_out must be a 16-byte aligned device pointer", who);
    const Ws w = ws_layout(d, q, Lq, S);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "%s: workspace too small (%ld < %ld bytes) or misaligned", who, ws_bytes,
                 w.total);
    char *ws = (char *)workspace;
    const char *sv = (const char *)saved;
    const float *loc = (const float *)(sv + s.loc), *attw = (const float *)(sv + s.attw);
    const uint16_t *opb = (const uint16_t *)(sv + s.opb);
    uint16_t *wt = (uint16_t *)(ws + w.wt), *dq = (uint16_t *)(ws + w.dq), *wcat = (uint16_t *)(ws + w.wcat);
    uint16_t *dwcat = (uint16_t *)(ws + w.dwcat), *dbcat = (uint16_t *)(ws + w.dbcat), *gv16 = (uint16_t *)(ws + w.gv16);
    float *gop = (float *)(ws + w.gop), *gv = (float *)(ws + w.gv), *gl = (float *)(ws + w.gl), *gw = (float *)(ws + w.gw);
    void *wg = ws + w.wg;

    // what has to be computed: a product is needed by its own gradient or by anything further up the chain
    const bool need_q = grad_query || g.sampling_offsets_w || g.attention_weights_w;   // dq (prep backward)
    const bool need_v = grad_input_flatten || g.value_proj_w;                          // grad_value
    const bool need_op = need_q || need_v;                                             // the operator's backward

    // ---- output_proj ----
    if (g.output_proj_w) TRY(gemm_wgrad_launch(grad_out, C, opb, C, (int)R, C, C, g.output_proj_w, C, g.output_proj_b, wg, w.wg_bytes, st));
    if (!need_op) return VLLM_OK;
    TRY(linear_dgrad(st, EPI_F32, grad_out, d->output_proj_w, C, C, R, wt, gop, nullptr, nullptr, 0));
    // ---- operator ----
    const float *value = (const float *)(sv + s.value);
    if (value_is_bf16) {
        TRY(bf16_to_f32_launch((const uint16_t *)(sv + s.value), (float *)(ws + w.vwide), VS * C, st));
        value = (const float *)(ws + w.vwide);
    }
    // grad_value is accumulated with atomics: zero-filled in every case; the two per-point gradients unless the kernel writes every element itself
    TRY(zero_bytes(gv, VS * C * 4, st, who));
    if (!vllm_msda_backward_f32_writes_point_grads(value, loc, gop, gv, gl, B, S, M, q.D, L, Lq, P)) {
        TRY(zero_bytes(gl, R * MLP * 2 * 4, st, who));
        TRY(zero_bytes(gw, R * MLP * 4, st, who));
    }
    TRY(vllm_msda_backward_f32(value, shapes, lsi, loc, attw, gop, B, S, M, q.D, L, Lq, P, gv, gl, gw, stream));
    // ---- sampling_offsets / attention_weights: one input-gradient and one weight-gradient GEMM over the concatenation ----
    if (need_q) {
        TRY(msda_prep_bwd_launch(gl, gw, attw, ref, shapes, R, M, L, P, d->ref_dim, d->use_4d_normalizer, dq, N, st));
        if (grad_query) {
            TRY(copy_d2d(wcat, d->sampling_offsets_w, 2L * MLP * C * 2, st, who));
            TRY(copy_d2d(wcat + 2L * MLP * C, d->attention_weights_w, (long)MLP * C * 2, st, who));
            TRY(zero_bytes(wcat + 3L * MLP * C, (N - 3L * MLP) * C * 2, st, who));
            TRY(linear_dgrad(st, EPI_BIAS, dq, wcat, N, C, R, wt, grad_query, nullptr, nullptr, 0));
        }
        if (g.sampling_offsets_w || g.attention_weights_w) {
            TRY(gemm_wgrad_launch(dq, N, query, C, (int)R, N, C, dwcat, C, dbcat, wg, w.wg_bytes, st));
            if (g.sampling_offsets_w) TRY(copy_d2d(g.sampling_offsets_w, dwcat, 2L * MLP * C * 2, st, who));
            if (g.sampling_offsets_b) TRY(copy_d2d(g.sampling_offsets_b, dbcat, 2L * MLP * 2, st, who));
            if (g.attention_weights_w) TRY(copy_d2d(g.attention_weights_w, dwcat + 2L * MLP * C, (long)MLP * C * 2, st, who));
            if (g.attention_weights_b) TRY(copy_d2d(g.attention_weights_b, dbcat + 2L * MLP, (long)MLP * 2, st, who));
        }
    }
    // ---- value_proj: the key-padding zero fill's backward is the narrowing pass's row mask ----
    if (need_v) {
        TRY(f32_to_bf16_masked_launch(gv, gv16, VS, C, padding_mask, st));
        if (g.value_proj_w) TRY(gemm_wgrad_launch(gv16, C, input_flatten, C, (int)VS, C, C, g.value_proj_w, C, g.value_proj_b, wg, w.wg_bytes, st));
        if (grad_input_flatten) TRY(linear_dgrad(st, EPI_BIAS, gv16, d->value_proj_w, C, C, VS, wt, grad_input_flatten, nullptr, nullptr, 0));
    }
    return VLLM_OK;
}
