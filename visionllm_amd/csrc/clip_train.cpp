// Training one CLIP encoder layer behind the C ABI (transformers 4.34 CLIPEncoderLayer.forward: layer_norm1 -> CLIPAttention -> residual ->
// layer_norm2 -> CLIPMLP -> residual; the reference builds CLIPVisionModel in the vis_encoder slot, visionllmv2/train/train.py:382-384, and
// trains it with freeze_vis_encoder=False, :163, 534).  vit_train.cpp without QK-norm and LayerScale, with LayerNorm and either activation.
//   forward_train: the statement order of vit.cpp WITHOUT folded norms --
//       xn1 = LN1(x) -> qkv = xn1 Wqkv^T + b -> ctx, lse = attention(q, k, v)   (softmax scale inside the kernel, as in the inference path)
//       -> x1 = x + ctx Wo^T + b   (EPI_RESIDUAL, no scale)
//       -> xn2 = LN2(x1) -> a1 = act(h1), h1 = xn2 W1^T + b   (EPI_QUICK_GELU_SAVE / EPI_GELU_SAVE) -> out = x1 + a1 W2^T + b
//   saved (caller buffers): qkv, ctx, lse, x1, h1, a1: (5 C + 2 I) M bf16 elements + lse.  No LayerScale, so no pre-LayerScale output is kept.
//   recomputed in the backward, one norm launch each: xn1 = LN1(x), xn2 = LN2(x1).
//   backward, from grad_out g:
//       dW2 = g^T a1, db2 = colsum g;  dh1 = (g W2) act'(h1)                 (gemm_wgrad; bf16 GEMM on W2^T, EPI_QUICK_GELU_BWD / EPI_GELU_BWD)
//       dW1 = dh1^T xn2, db1;  dxn2 = dh1 W1
//       g1 = LN2'(x1; dxn2) + g, grad_norm2 w / b                             (ln_res_bwd_kernel, grad_res = g: x1's two uses in one rounding)
//       dWo = g1^T ctx, dbo;  dctx = g1 Wo;  dqkv = attention'(qkv, ctx, lse; dctx)
//       dWqkv = dqkv^T xn1, dbqkv (its k block exactly zero: softmax is invariant to the k bias);  dxn1 = dqkv Wqkv
//       grad_x = LN1'(x; dxn1) + g1, grad_norm1 w / b
//   A NULL gradient pointer skips that product, and everything only it needed.
// No allocation, no synchronisation, one stream; the workspace is the caller's.
#include <algorithm>
#include <math.h>
#include "orchestrate.hpp"

using namespace vllm;

namespace {
struct Dims { int C, H, D, I, B, S; long M; bool quick; };

int check_layer(const VllmClipLayerTrain *d, int B, int S, Dims *o, const char *who)
{
    VLLM_REQUIRE(d, "%s: null descriptor", who);
    VLLM_REQUIRE(d->hidden > 0 && d->heads > 0 && d->hidden % d->heads == 0, "%s: hidden %d / heads %d", who, d->hidden, d->heads);
    const int hd = d->hidden / d->heads;
    VLLM_REQUIRE(hd == 64 || hd == 128, "%s: head_dim %d not supported by the attention kernels (64 or 128)", who, hd);
    VLLM_REQUIRE(d->inter > 0 && d->hidden % 64 == 0 && d->inter % 64 == 0 && d->hidden <= 8192,
                 "%s: hidden / intermediate must be multiples of 64, hidden <= 8192 (the row-wise backward kernels)", who);
    VLLM_REQUIRE(d->act == VLLM_EPI_GELU || d->act == VLLM_EPI_QUICK_GELU, "%s: act %d (VLLM_EPI_GELU or VLLM_EPI_QUICK_GELU)", who, d->act);
    VLLM_REQUIRE(B >= 0 && S > 0 && (long)B * S < (1L << 31) / 4, "%s: B=%d S=%d", who, B, S);
    const void *ps[] = {d->norm1_w, d->norm1_b, d->qkv_w, d->qkv_b, d->proj_w, d->proj_b, d->norm2_w, d->norm2_b, d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b};
    for (const void *p : ps) VLLM_REQUIRE(p, "%s: layer parameters missing", who);
    for (const void *p : ps) VLLM_REQUIRE(aligned16(p), "%s: parameters must be 16-byte aligned", who);
    o->C = d->hidden; o->H = d->heads; o->D = hd; o->I = d->inter; o->B = B; o->S = S; o->M = (long)B * S; o->quick = d->act == VLLM_EPI_QUICK_GELU;
    return VLLM_OK;
}

int check_saved(const VllmClipLayerSaved *s, const char *who)
{
    VLLM_REQUIRE(s && s->qkv && s->ctx && s->lse && s->x1 && s->h1 && s->a1, "%s: saved buffers missing", who);
    const void *ps[] = {s->qkv, s->ctx, s->lse, s->x1, s->h1, s->a1};
    for (const void *p : ps) VLLM_REQUIRE(aligned16(p), "%s: saved buffers must be 16-byte aligned", who);
    return VLLM_OK;
}

// forward: [sk][xn]; backward: [sk][xn][ga][gb][gi][gq][wt][wg][np][ad]
struct Ws { long sk, sk_bytes, xn, ga, gb, gi, gq, wt, wg, wg_bytes, np, np_bytes, ad, ad_bytes, fwd_total, total; };
Ws ws_layout(const Dims &q)
{
    const long M = q.M, C = q.C, I = q.I;
    Ws w;
    Carver cv;
    w.sk_bytes = M >= 1024 ? SK_SCRATCH_BYTES : 0;   // stream-K tail of the 8-phase GEMM, as the other orchestrators size it
    w.sk = cv.take(w.sk_bytes);
    w.xn = cv.take(M * C * 2);                            // LN1(x) / LN2(x1); dctx between them in the backward
    w.fwd_total = cv.off;
    w.ga = cv.take(M * C * 2);                            // dxn1
    w.gb = cv.take(M * C * 2);                            // dxn2 -> g1 (in place), kept until LN1's backward
    w.gi = cv.take(M * I * 2);                            // dh1
    w.gq = cv.take(M * 3 * C * 2);                        // dqkv
    w.wt = cv.take(std::max(3 * C * C, C * I) * 2);       // W^T of the input-gradient GEMM at hand
    const long wg = std::max({gemm_wgrad_workspace_bytes((int)M, (int)C, (int)I), gemm_wgrad_workspace_bytes((int)M, (int)I, (int)C),
                   gemm_wgrad_workspace_bytes((int)M, (int)C, (int)C), gemm_wgrad_workspace_bytes((int)M, (int)(3 * C), (int)C)});
    w.wg_bytes = std::max(0L, wg);
    w.wg = cv.take(w.wg_bytes);
    w.np_bytes = std::max(0L, ln_res_bwd_workspace_bytes(M, (int)C));   // column-sum partials of the LayerNorm backward
    w.np = cv.take(w.np_bytes);
    w.ad_bytes = std::max(0L, vllm_attn_bwd_workspace_bytes(q.B, q.S, q.H, q.D));
    w.ad = cv.take(w.ad_bytes);
    w.total = cv.off;
    return w;
}
}  // namespace

extern "C" int vllm_clip_layer_train_sizeof(void) { return (int)sizeof(VllmClipLayerTrain); }
extern "C" int vllm_clip_layer_saved_sizeof(void) { return (int)sizeof(VllmClipLayerSaved); }
extern "C" int vllm_clip_layer_grads_sizeof(void) { return (int)sizeof(VllmClipLayerGrads); }

extern "C" long vllm_clip_layer_backward_workspace_bytes(const VllmClipLayerTrain *d, int B, int S)
{
    Dims q;
    if (check_layer(d, B, S, &q, "clip_layer_backward_workspace_bytes") != VLLM_OK) return -1;
    return ws_layout(q).total;
}

extern "C" int vllm_clip_layer_forward_train(const VllmClipLayerTrain *d, const uint16_t *x, int B, int S, uint16_t *out,
                                             const VllmClipLayerSaved *saved, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    Dims q;
    TRY(check_layer(d, B, S, &q, "clip_layer_forward_train"));
    if (q.M == 0) return VLLM_OK;
    TRY(check_saved(saved, "clip_layer_forward_train"));
    VLLM_REQUIRE(x && out && aligned16(x) && aligned16(out), "clip_layer_forward_train: x and out must be 16-byte aligned device pointers");
    const Ws w = ws_layout(q);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.fwd_total, "clip_layer_forward_train: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.fwd_total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int C = q.C, I = q.I;
    const long M = q.M;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, "clip_layer_forward_train"));
    uint16_t *xn = (uint16_t *)(ws + w.xn);
    const VllmClipLayerSaved &s = *saved;

    TRY(norm_bf16_launch(false, x, C, d->norm1_w, d->norm1_b, xn, C, M, C, d->eps, st));
    TRY(gemm(st, EPI_BIAS, xn, C, d->qkv_w, C, d->qkv_b, s.qkv, 3 * C, (int)M, 3 * C, C, nullptr, nullptr, 0, 0, 0, sk, w.sk_bytes));
    {
        AttnArgs a;
        a.q = s.qkv; a.k = s.qkv + C; a.v = s.qkv + 2 * C; a.out = s.ctx;
        a.q_bs = a.k_bs = a.v_bs = (long)q.S * 3 * C;
        a.q_ts = a.k_ts = a.v_ts = 3 * C;
        a.q_hs = a.k_hs = a.v_hs = q.D;
        a.B = q.B; a.S = q.S; a.H = q.H; a.nqt = 0;
        a.scale_log2e = (1.0f / sqrtf((float)q.D)) * 1.4426950408889634f;
        a.lse = s.lse;
        TRY(attn_fwd_launch(a, q.D, st));
    }
    TRY(gemm(st, EPI_RESIDUAL, s.ctx, C, d->proj_w, C, d->proj_b, s.x1, C, (int)M, C, C, nullptr, x, C, 0, 0, sk, w.sk_bytes));
    TRY(norm_bf16_launch(false, s.x1, C, d->norm2_w, d->norm2_b, xn, C, M, C, d->eps, st));
    GemmArgs fc1 = gemm_args(xn, C, d->fc1_w, C, d->fc1_b, s.a1, I, M, I, C);   // the epilogue also leaves its pre-activation for the backward
    fc1.pre = s.h1;
    gemm_set_scratch(fc1, sk, w.sk_bytes);
    TRY(gemm_bf16_launch(q.quick ? EPI_QUICK_GELU_SAVE : EPI_GELU_SAVE, fc1, st));
    TRY(gemm(st, EPI_RESIDUAL, s.a1, I, d->fc2_w, I, d->fc2_b, out, C, (int)M, C, I, nullptr, s.x1, C, 0, 0, sk, w.sk_bytes));
    return VLLM_OK;
}

extern "C" int vllm_clip_layer_backward(const VllmClipLayerTrain *d, const uint16_t *x, int B, int S, const uint16_t *grad_out,
                                        const VllmClipLayerSaved *saved, uint16_t *grad_x, const VllmClipLayerGrads *grads, void *workspace,
                                        long ws_bytes, vllm_stream_t stream)
{
    Dims q;
    TRY(check_layer(d, B, S, &q, "clip_layer_backward"));
    VLLM_REQUIRE(grads, "clip_layer_backward: null gradient table");
    const VllmClipLayerGrads &g = *grads;
    VLLM_REQUIRE((!g.qkv_b || g.qkv_w) && (!g.proj_b || g.proj_w) && (!g.fc1_b || g.fc1_w) && (!g.fc2_b || g.fc2_w),
                 "clip_layer_backward: a bias gradient comes out of its weight gradient's launch (pass both)");
    const void *gp[] = {grad_x, g.norm1_w, g.norm1_b, g.qkv_w, g.qkv_b, g.proj_w, g.proj_b, g.norm2_w, g.norm2_b, g.fc1_w, g.fc1_b, g.fc2_w, g.fc2_b};
    for (const void *p : gp) VLLM_REQUIRE(aligned16(p), "clip_layer_backward: gradients must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int C = q.C, I = q.I;
    const long M = q.M;
    if (M == 0) {   // no rows: every parameter gradient is an empty sum
        return zero_bf16(st, "clip_layer_backward", {{g.norm1_w, C}, {g.norm1_b, C}, {g.qkv_w, 3L * C * C}, {g.qkv_b, 3L * C}, {g.proj_w, (long)C * C},
                                                     {g.proj_b, C}, {g.norm2_w, C}, {g.norm2_b, C}, {g.fc1_w, (long)I * C}, {g.fc1_b, I},
                                                     {g.fc2_w, (long)C * I}, {g.fc2_b, C}});
    }
    TRY(check_saved(saved, "clip_layer_backward"));
    VLLM_REQUIRE(x && grad_out && aligned16(x) && aligned16(grad_out), "clip_layer_backward: x and grad_out must be 16-byte aligned device pointers");
    const Ws w = ws_layout(q);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "clip_layer_backward: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.total);
    char *ws = (char *)workspace;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, "clip_layer_backward"));
    uint16_t *xn = (uint16_t *)(ws + w.xn), *ga = (uint16_t *)(ws + w.ga), *gb = (uint16_t *)(ws + w.gb);
    uint16_t *gi = (uint16_t *)(ws + w.gi), *gq = (uint16_t *)(ws + w.gq), *wt = (uint16_t *)(ws + w.wt);
    void *wg = ws + w.wg, *np = ws + w.np;
    const VllmClipLayerSaved &s = *saved;

    // what has to be computed: a product is needed by its own gradient or by anything further up the chain
    const bool n1 = grad_x || g.norm1_w || g.norm1_b;                      // LN1's backward (dxn1)
    const bool dq = n1 || g.qkv_w;                                         // dqkv (attention backward)
    const bool x1 = dq || g.proj_w;                                        // g1, the gradient at the mid hidden state
    const bool n2 = x1 || g.norm2_w || g.norm2_b;                          // dxn2
    const bool h1 = n2 || g.fc1_w;                                         // dh1

    // ---- MLP block ----
    if (g.fc2_w) TRY(gemm_wgrad_launch(grad_out, C, s.a1, I, (int)M, C, I, g.fc2_w, I, g.fc2_b, wg, w.wg_bytes, st));
    if (h1) TRY(linear_dgrad(st, q.quick ? EPI_QUICK_GELU_BWD : EPI_GELU_BWD, grad_out, d->fc2_w, C, I, M, wt, gi, s.h1, sk, w.sk_bytes));
    if (g.fc1_w) {
        TRY(norm_bf16_launch(false, s.x1, C, d->norm2_w, d->norm2_b, xn, C, M, C, d->eps, st));
        TRY(gemm_wgrad_launch(gi, I, xn, C, (int)M, I, C, g.fc1_w, C, g.fc1_b, wg, w.wg_bytes, st));
    }
    if (!n2) return VLLM_OK;
    TRY(linear_dgrad(st, EPI_BIAS, gi, d->fc1_w, I, C, M, wt, gb, nullptr, sk, w.sk_bytes));
    TRY(ln_res_bwd_launch(s.x1, C, gb, C, d->norm2_w, d->eps, M, C, x1 ? gb : nullptr, C, x1 ? grad_out : nullptr, C, g.norm2_w, g.norm2_b, np,
                          w.np_bytes, st));
    if (!x1) return VLLM_OK;
    const uint16_t *g1 = gb;
    // ---- attention block ----
    if (g.proj_w) TRY(gemm_wgrad_launch(g1, C, s.ctx, C, (int)M, C, C, g.proj_w, C, g.proj_b, wg, w.wg_bytes, st));
    if (!dq) return VLLM_OK;
    uint16_t *dctx = xn;   // (LN2(x1) has been consumed)
    TRY(linear_dgrad(st, EPI_BIAS, g1, d->proj_w, C, C, M, wt, dctx, nullptr, sk, w.sk_bytes));
    TRY(attn_bwd_launch(s.qkv, s.ctx, s.lse, dctx, q.B, q.S, q.H, q.D, 1.0f / sqrtf((float)q.D), gq, ws + w.ad, w.ad_bytes, false, st));
    if (g.qkv_w) {
        TRY(norm_bf16_launch(false, x, C, d->norm1_w, d->norm1_b, xn, C, M, C, d->eps, st));
        TRY(gemm_wgrad_launch(gq, 3 * C, xn, C, (int)M, 3 * C, C, g.qkv_w, C, g.qkv_b, wg, w.wg_bytes, st));
        // The k projection's bias has no gradient: it adds q_i . b_k to every score of query row i, and softmax does not see a shift of a
        // row.  What the column sum of the computed dK holds is rounding noise only (measured: 1e-3 of the other bias gradients' size, as
        // in torch's bf16 autograd), so the k block of grad_qkv_b is written as the exact value.
        if (g.qkv_b) VLLM_REQUIRE(hipMemsetAsync(g.qkv_b + C, 0, (size_t)C * 2, st) == hipSuccess, "clip_layer_backward: memset failed");
    }
    if (!n1) return VLLM_OK;
    TRY(linear_dgrad(st, EPI_BIAS, gq, d->qkv_w, 3 * C, C, M, wt, ga, nullptr, sk, w.sk_bytes));
    TRY(ln_res_bwd_launch(x, C, ga, C, d->norm1_w, d->eps, M, C, grad_x, C, grad_x ? g1 : nullptr, C, g.norm1_w, g.norm1_b, np, w.np_bytes, st));
    return VLLM_OK;
}
