// Training one pre-norm encoder layer behind the C ABI, for both vision towers the reference may train (freeze_vis_encoder=False,
// visionllmv2/train/train.py:163, 534):
//   InternViT (InternVisionEncoderLayer.forward, modeling_intern_vit.py:182-210, run under torch.utils.checkpoint, :259-262): RMSNorm,
//       an optional qkv bias, an optional QK-norm, LayerScale behind proj and fc2, erf GELU;
//   CLIP (transformers 4.34 CLIPEncoderLayer.forward, built in the vis_encoder slot, train.py:382-384): LayerNorm with bias, no QK-norm,
//       no LayerScale, quick-GELU or erf GELU.
// One chain serves both; [..] marks what only one family has.
//   forward_train: the statement order of vit.cpp WITHOUT folded norms --
//       xn1 = norm1(x) -> qkv = xn1 Wqkv^T + b -> [q, k = q_norm(q), k_norm(k)] -> ctx, lse = attention(q, k, v)
//       -> x1 = x + (ctx Wproj^T + b) [ls1]   ([EPI_RESIDUAL_SAVE: y1 = ctx Wproj^T + b leaves too]; EPI_RESIDUAL without LayerScale)
//       -> xn2 = norm2(x1) -> a1 = act(h1), h1 = xn2 Wfc1^T + b   (EPI_GELU_SAVE / EPI_QUICK_GELU_SAVE) -> out = x1 + (a1 Wfc2^T + b) [ls2]   [y2]
//   saved (caller buffers): qkv BEFORE the QK-norm, ctx, lse, x1, h1, a1, [y1, y2]: (5 C + 2 I) M bf16 elements + lse [+ 2 C M].
//   recomputed in the backward, one norm launch each: xn1 = norm1(x), xn2 = norm2(x1), [the post-norm q / k (with v copied beside them:
//       the attention backward reads one packed [M, 3C] tensor)].  Saving them instead would add 2 (qk-norm: 5) x M x C x 2 bytes to
//       what a layer keeps; a norm launch reads and writes 2 x M x C x 2 bytes once.
//   backward, from grad_out g:
//       [gy2 = g ls2, grad_ls2 = sum g y2  (ls_bwd_kernel)]; gy2 = g without LayerScale
//       dWfc2 = gy2^T a1, db = colsum gy2;  dh1 = (gy2 Wfc2) act'(h1)          (gemm_wgrad; bf16 GEMM on Wfc2^T, EPI_GELU_BWD / EPI_QUICK_GELU_BWD)
//       dWfc1 = dh1^T xn2, db;  dxn2 = dh1 Wfc1
//       g1 = norm2'(x1; dxn2) + g, grad_norm2                                  (rms_bwd_kernel / ln_res_bwd_kernel, grad_res = g: x1's two uses in one rounding)
//       [gy1 = g1 ls1, grad_ls1 = sum g1 y1]; gy1 = g1 without;  dWproj = gy1^T ctx, db;  dctx = gy1 Wproj
//       dqkv = attention'(q, k, v, ctx, lse; dctx);  [QK-norm backward in place on its q / k blocks (G = 2), grad_q_norm / grad_k_norm]
//       dWqkv = dqkv^T xn1, db (CLIP: its k block exactly zero, see there);  dxn1 = dqkv Wqkv;  grad_x = norm1'(x; dxn1) + g1, grad_norm1
//   A NULL gradient pointer skips that product, and everything only it needed.
// No allocation, no synchronisation, one stream; the workspace is the caller's.
#include <algorithm>
#include <math.h>
#include "orchestrate.hpp"

using namespace vllm;

namespace {
// A layer of either family; a pointer is null where the family (or this layer) has no such parameter / saved tensor / gradient, and
// `given` is false for a caller's null struct (the checks name it).
struct Layer {
    bool given;
    int C, H, I, B, S;
    bool rms;    // InternViT: RMSNorm without bias, LayerScale; otherwise CLIP: LayerNorm with bias, qkv bias required
    int act;     // VLLM_EPI_GELU or VLLM_EPI_QUICK_GELU
    float eps;
    const uint16_t *norm1_w, *norm1_b, *qkv_w, *qkv_b, *q_norm_w, *k_norm_w, *proj_w, *proj_b, *ls1, *norm2_w, *norm2_b, *fc1_w, *fc1_b,
        *fc2_w, *fc2_b, *ls2;
    int D() const { return C / H; }
    long M() const { return (long)B * S; }
};
struct Saved { uint16_t *qkv, *ctx; float *lse; uint16_t *y1, *x1, *h1, *a1, *y2; };   // (a null struct: nothing given)
struct Grads {
    bool given;
    uint16_t *norm1_w, *norm1_b, *qkv_w, *qkv_b, *q_norm_w, *k_norm_w, *proj_w, *proj_b, *ls1, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w,
        *fc2_b, *ls2;
};

// The public structs -> the description above
Layer layer(const VllmVitLayerTrain *d, int B, int S)
{
    if (!d) return {};
    return {true, d->hidden, d->heads, d->inter, B, S, true, VLLM_EPI_GELU, d->eps, d->norm1_w, nullptr, d->qkv_w, d->qkv_b, d->q_norm_w,
            d->k_norm_w, d->proj_w, d->proj_b, d->ls1, d->norm2_w, nullptr, d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, d->ls2};
}
Layer layer(const VllmClipLayerTrain *d, int B, int S)
{
    if (!d) return {};
    return {true, d->hidden, d->heads, d->inter, B, S, false, d->act, d->eps, d->norm1_w, d->norm1_b, d->qkv_w, d->qkv_b, nullptr,
            nullptr, d->proj_w, d->proj_b, nullptr, d->norm2_w, d->norm2_b, d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, nullptr};
}
Saved table(const VllmVitLayerSaved *s) { return s ? Saved{s->qkv, s->ctx, s->lse, s->y1, s->x1, s->h1, s->a1, s->y2} : Saved{}; }
Saved table(const VllmClipLayerSaved *s) { return s ? Saved{s->qkv, s->ctx, s->lse, nullptr, s->x1, s->h1, s->a1, nullptr} : Saved{}; }
Grads table(const VllmVitLayerGrads *g)
{
    if (!g) return {};
    return {true, g->norm1_w, nullptr, g->qkv_w, g->qkv_b, g->q_norm_w, g->k_norm_w, g->proj_w, g->proj_b, g->ls1, g->norm2_w, nullptr,
            g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, g->ls2};
}
Grads table(const VllmClipLayerGrads *g)
{
    if (!g) return {};
    return {true, g->norm1_w, g->norm1_b, g->qkv_w, g->qkv_b, nullptr, nullptr, g->proj_w, g->proj_b, nullptr, g->norm2_w, g->norm2_b,
            g->fc1_w, g->fc1_b, g->fc2_w, g->fc2_b, nullptr};
}

int check(const Layer &l, const char *who)
{
    VLLM_REQUIRE(l.given, "%s: null descriptor", who);
    VLLM_REQUIRE(l.C > 0 && l.H > 0 && l.C % l.H == 0, "%s: hidden %d / heads %d", who, l.C, l.H);
    VLLM_REQUIRE(l.D() == 64 || l.D() == 128, "%s: head_dim %d not supported by the attention kernels (64 or 128)", who, l.D());
    VLLM_REQUIRE(l.I > 0 && l.C % 64 == 0 && l.I % 64 == 0 && l.C <= 8192,
                 "%s: hidden / intermediate must be multiples of 64, hidden <= 8192 (the row-wise backward kernels)", who);
    VLLM_REQUIRE(l.act == VLLM_EPI_GELU || l.act == VLLM_EPI_QUICK_GELU, "%s: act %d (VLLM_EPI_GELU or VLLM_EPI_QUICK_GELU)", who, l.act);
    VLLM_REQUIRE(l.B >= 0 && l.S > 0 && l.M() < (1L << 31) / 4, "%s: B=%d S=%d", who, l.B, l.S);
    VLLM_REQUIRE(l.norm1_w && l.qkv_w && l.proj_w && l.proj_b && l.norm2_w && l.fc1_w && l.fc1_b && l.fc2_w && l.fc2_b &&
                     (l.rms ? l.ls1 && l.ls2 : l.norm1_b && l.qkv_b && l.norm2_b), "%s: layer parameters missing", who);
    VLLM_REQUIRE((l.q_norm_w != nullptr) == (l.k_norm_w != nullptr), "%s: q_norm and k_norm come together", who);
    const void *ps[] = {l.norm1_w, l.norm1_b, l.qkv_w, l.qkv_b, l.q_norm_w, l.k_norm_w, l.proj_w, l.proj_b, l.ls1, l.norm2_w, l.norm2_b,
                        l.fc1_w, l.fc1_b, l.fc2_w, l.fc2_b, l.ls2};
    for (const void *p : ps) VLLM_REQUIRE(aligned16(p), "%s: parameters must be 16-byte aligned", who);
    return VLLM_OK;
}

int check_saved(const Layer &l, const Saved &s, const char *who)
{
    VLLM_REQUIRE(s.qkv && s.ctx && s.lse && s.x1 && s.h1 && s.a1 && (!l.ls1 || (s.y1 && s.y2)), "%s: saved buffers missing", who);
    const void *ps[] = {s.qkv, s.ctx, s.lse, s.y1, s.x1, s.h1, s.a1, s.y2};
    for (const void *p : ps) VLLM_REQUIRE(aligned16(p), "%s: saved buffers must be 16-byte aligned", who);
    return VLLM_OK;
}

// forward: [sk][xn][qkn]; backward: [sk][xn][qkn][ga][gb][gi][gq][wt][wg][np][ad]   (qkn: no bytes without a QK-norm)
struct Ws { long sk, sk_bytes, xn, qkn, ga, gb, gi, gq, wt, wg, wg_bytes, np, np_bytes, ad, ad_bytes, fwd_total, total; };
Ws ws_layout(const Layer &l)
{
    const long M = l.M(), C = l.C, I = l.I;
    Ws w;
    Carver cv;
    w.sk_bytes = M >= 1024 ? SK_SCRATCH_BYTES : 0;   // stream-K tail of the 8-phase GEMM, as the other orchestrators size it
    w.sk = cv.take(w.sk_bytes);
    w.xn = cv.take(M * C * 2);                            // norm1(x) / norm2(x1); dctx between them in the backward
    w.qkn = cv.take(l.q_norm_w ? M * 3 * C * 2 : 0);      // post-norm q, k (forward) + v copied beside them (backward)
    w.fwd_total = cv.off;
    w.ga = cv.take(M * C * 2);                            // gy2, then gy1 (LayerScale); dxn1
    w.gb = cv.take(M * C * 2);                            // dxn2 -> g1 (in place), kept until norm1's backward
    w.gi = cv.take(M * I * 2);                            // dh1
    w.gq = cv.take(M * 3 * C * 2);                        // dqkv
    w.wt = cv.take(std::max(3 * C * C, C * I) * 2);       // W^T of the input-gradient GEMM at hand
    const long wg = std::max({gemm_wgrad_workspace_bytes((int)M, (int)C, (int)I), gemm_wgrad_workspace_bytes((int)M, (int)I, (int)C),
                   gemm_wgrad_workspace_bytes((int)M, (int)C, (int)C), gemm_wgrad_workspace_bytes((int)M, (int)(3 * C), (int)C)});
    w.wg_bytes = std::max(0L, wg);
    w.wg = cv.take(w.wg_bytes);
    // column-sum partials of the row-wise backwards: two fp32 rows per block, for the QK-norm's q and k (G = 2, the largest RMSNorm user) as
    // for a LayerNorm's weight and bias (ln_res_bwd_workspace_bytes answers the same number)
    w.np_bytes = std::max(0L, rms_bwd_workspace_bytes(M, (int)C, 2));
    w.np = cv.take(w.np_bytes);
    w.ad_bytes = std::max(0L, vllm_attn_bwd_workspace_bytes(l.B, l.S, l.H, l.D()));
    w.ad = cv.take(w.ad_bytes);
    w.total = cv.off;
    return w;
}

long workspace_bytes(const Layer &l, const char *who) { return check(l, who) == VLLM_OK ? ws_layout(l).total : -1; }

int forward_train(const Layer &l, const uint16_t *x, uint16_t *out, const Saved &s, void *workspace, long ws_bytes, vllm_stream_t stream,
                  const char *who)
{
    TRY(check(l, who));
    if (l.M() == 0) return VLLM_OK;
    TRY(check_saved(l, s, who));
    VLLM_REQUIRE(x && out && aligned16(x) && aligned16(out), "%s: x and out must be 16-byte aligned device pointers", who);
    const Ws w = ws_layout(l);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.fwd_total, "%s: workspace too small (%ld < %ld bytes) or misaligned", who,
                 ws_bytes, w.fwd_total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int C = l.C, I = l.I;
    const long M = l.M();
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, who));
    uint16_t *xn = (uint16_t *)(ws + w.xn), *qkn = (uint16_t *)(ws + w.qkn);
    const bool quick = l.act == VLLM_EPI_QUICK_GELU;

    TRY(norm_bf16_launch(l.rms, x, C, l.norm1_w, l.norm1_b, xn, C, M, C, l.eps, st));
    TRY(gemm(st, EPI_BIAS, xn, C, l.qkv_w, C, l.qkv_b, s.qkv, 3 * C, (int)M, 3 * C, C, nullptr, nullptr, 0, 0, 0, sk, w.sk_bytes));
    const uint16_t *qk = s.qkv;
    if (l.q_norm_w) {   // out of place: the backward normalises the pre-norm q / k again
        TRY(norm_bf16_launch(true, s.qkv, 3 * C, l.q_norm_w, nullptr, qkn, 3 * C, M, C, l.eps, st, l.k_norm_w, 2));
        qk = qkn;
    }
    TRY(attn_fwd_launch(packed_qkv_attn(qk, s.qkv, s.ctx, l.B, l.S, l.H, l.D(), 1.0f / sqrtf((float)l.D()), s.lse), l.D(), st));
    // the GEMMs whose epilogue also leaves its pre-activation / pre-LayerScale output (`pre`) for the backward; a residual GEMM without
    // LayerScale has nothing to leave and is the inference encoder's
    auto gemm_pre = [&](int epi, GemmArgs a, const uint16_t *ls, const uint16_t *res, uint16_t *pre) {
        a.scale = ls; a.res = res; a.ldr = res ? C : 0; a.pre = pre;
        gemm_set_scratch(a, sk, w.sk_bytes);
        return gemm_bf16_launch(epi, a, st);
    };
    TRY(gemm_pre(l.ls1 ? EPI_RESIDUAL_SAVE : EPI_RESIDUAL, gemm_args(s.ctx, C, l.proj_w, C, l.proj_b, s.x1, C, M, C, C), l.ls1, x, s.y1));
    TRY(norm_bf16_launch(l.rms, s.x1, C, l.norm2_w, l.norm2_b, xn, C, M, C, l.eps, st));
    TRY(gemm_pre(quick ? EPI_QUICK_GELU_SAVE : EPI_GELU_SAVE, gemm_args(xn, C, l.fc1_w, C, l.fc1_b, s.a1, I, M, I, C), nullptr, nullptr, s.h1));
    TRY(gemm_pre(l.ls2 ? EPI_RESIDUAL_SAVE : EPI_RESIDUAL, gemm_args(s.a1, I, l.fc2_w, I, l.fc2_b, out, C, M, C, I), l.ls2, s.x1, s.y2));
    return VLLM_OK;
}

int backward(const Layer &l, const uint16_t *x, const uint16_t *grad_out, const Saved &s, uint16_t *grad_x, const Grads &g, void *workspace,
             long ws_bytes, vllm_stream_t stream, const char *who)
{
    TRY(check(l, who));
    VLLM_REQUIRE(g.given, "%s: null gradient table", who);
    VLLM_REQUIRE((!g.qkv_b || (l.qkv_b && g.qkv_w)) && (!g.proj_b || g.proj_w) && (!g.fc1_b || g.fc1_w) && (!g.fc2_b || g.fc2_w),
                 "%s: a bias gradient comes out of its weight gradient's launch (pass both), and only for a bias the layer has", who);
    VLLM_REQUIRE(l.q_norm_w || (!g.q_norm_w && !g.k_norm_w), "%s: the layer has no QK-norm", who);
    const void *gp[] = {grad_x, g.norm1_w, g.norm1_b, g.qkv_w, g.qkv_b, g.q_norm_w, g.k_norm_w, g.proj_w, g.proj_b, g.ls1, g.norm2_w, g.norm2_b,
                        g.fc1_w, g.fc1_b, g.fc2_w, g.fc2_b, g.ls2};
    for (const void *p : gp) VLLM_REQUIRE(aligned16(p), "%s: gradients must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const int C = l.C, I = l.I, D = l.D();
    const long M = l.M();
    if (M == 0) {   // no rows: every parameter gradient is an empty sum
        return zero_bf16(st, who, {{g.norm1_w, C}, {g.norm1_b, C}, {g.qkv_w, 3L * C * C}, {g.qkv_b, 3L * C}, {g.q_norm_w, C}, {g.k_norm_w, C},
                                   {g.proj_w, (long)C * C}, {g.proj_b, C}, {g.ls1, C}, {g.norm2_w, C}, {g.norm2_b, C}, {g.fc1_w, (long)I * C},
                                   {g.fc1_b, I}, {g.fc2_w, (long)C * I}, {g.fc2_b, C}, {g.ls2, C}});
    }
    TRY(check_saved(l, s, who));
    VLLM_REQUIRE(x && grad_out && aligned16(x) && aligned16(grad_out), "%s: x and grad_out must be 16-byte aligned device pointers", who);
    const Ws w = ws_layout(l);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "%s: workspace too small (%ld < %ld bytes) or misaligned", who,
                 ws_bytes, w.total);
    char *ws = (char *)workspace;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, who));
    uint16_t *xn = (uint16_t *)(ws + w.xn), *qkn = (uint16_t *)(ws + w.qkn), *ga = (uint16_t *)(ws + w.ga), *gb = (uint16_t *)(ws + w.gb);
    uint16_t *gi = (uint16_t *)(ws + w.gi), *gq = (uint16_t *)(ws + w.gq), *wt = (uint16_t *)(ws + w.wt);
    void *wg = ws + w.wg, *np = ws + w.np;

    // what has to be computed: a product is needed by its own gradient or by anything further up the chain
    const bool n1 = grad_x || g.norm1_w || g.norm1_b;                      // norm1's backward (dxn1)
    const bool dq = n1 || g.qkv_w || g.q_norm_w || g.k_norm_w;             // dqkv (attention backward)
    const bool y1 = dq || g.proj_w;                                        // gy1
    const bool x1 = y1 || g.ls1;                                           // g1, the gradient at the mid hidden state
    const bool n2 = x1 || g.norm2_w || g.norm2_b;                          // dxn2
    const bool h1 = n2 || g.fc1_w;                                         // dh1
    const bool y2 = h1 || g.fc2_w;                                         // gy2

    // a norm of the layer; its backward with the residual path's gradient added: gx = norm'(xin; gy) + gres
    auto norm = [&](const uint16_t *xin, const uint16_t *nw, const uint16_t *nb) { return norm_bf16_launch(l.rms, xin, C, nw, nb, xn, C, M, C, l.eps, st); };
    auto norm_bwd = [&](const uint16_t *xin, const uint16_t *gy, const uint16_t *nw, uint16_t *gx, const uint16_t *gres, uint16_t *gw, uint16_t *gbias) {
        return l.rms ? rms_bwd_launch(xin, C, gy, C, nw, nullptr, 1, l.eps, M, C, gx, C, gres, C, gw, nullptr, np, w.np_bytes, st)
                     : ln_res_bwd_launch(xin, C, gy, C, nw, l.eps, M, C, gx, C, gres, C, gw, gbias, np, w.np_bytes, st);
    };
    // The recomputed norm output is read by the weight-gradient GEMM behind it and by nothing else (the norm's backward takes the norm's
    // input; dctx overwrites the slot), so a frozen Linear weight costs no norm launch.

    // ---- MLP block ----
    const uint16_t *gy2 = grad_out;   // the gradient at fc2's output: behind LayerScale where there is one
    if (l.ls2) {
        if (y2 || g.ls2) TRY(ls_bwd_launch(grad_out, C, s.y2, C, l.ls2, M, C, y2 ? ga : nullptr, C, g.ls2, np, w.np_bytes, st));
        gy2 = ga;
    }
    if (g.fc2_w) TRY(gemm_wgrad_launch(gy2, C, s.a1, I, (int)M, C, I, g.fc2_w, I, g.fc2_b, wg, w.wg_bytes, st));
    if (h1) TRY(linear_dgrad(st, l.act == VLLM_EPI_QUICK_GELU ? EPI_QUICK_GELU_BWD : EPI_GELU_BWD, gy2, l.fc2_w, C, I, M, wt, gi, s.h1, sk, w.sk_bytes));
    if (g.fc1_w) {
        TRY(norm(s.x1, l.norm2_w, l.norm2_b));
        TRY(gemm_wgrad_launch(gi, I, xn, C, (int)M, I, C, g.fc1_w, C, g.fc1_b, wg, w.wg_bytes, st));
    }
    if (!n2) return VLLM_OK;
    TRY(linear_dgrad(st, EPI_BIAS, gi, l.fc1_w, I, C, M, wt, gb, nullptr, sk, w.sk_bytes));
    TRY(norm_bwd(s.x1, gb, l.norm2_w, x1 ? gb : nullptr, x1 ? grad_out : nullptr, g.norm2_w, g.norm2_b));
    if (!x1) return VLLM_OK;
    const uint16_t *g1 = gb;
    // ---- attention block ----
    const uint16_t *gy1 = g1;
    if (l.ls1) {
        TRY(ls_bwd_launch(g1, C, s.y1, C, l.ls1, M, C, y1 ? ga : nullptr, C, g.ls1, np, w.np_bytes, st));
        gy1 = ga;
    }
    if (g.proj_w) TRY(gemm_wgrad_launch(gy1, C, s.ctx, C, (int)M, C, C, g.proj_w, C, g.proj_b, wg, w.wg_bytes, st));
    if (!dq) return VLLM_OK;
    uint16_t *dctx = xn;   // (norm2(x1) has been consumed)
    TRY(linear_dgrad(st, EPI_BIAS, gy1, l.proj_w, C, C, M, wt, dctx, nullptr, sk, w.sk_bytes));
    const uint16_t *qkv_n = s.qkv;
    if (l.q_norm_w) {
        TRY(norm_bf16_launch(true, s.qkv, 3 * C, l.q_norm_w, nullptr, qkn, 3 * C, M, C, l.eps, st, l.k_norm_w, 2));
        VLLM_REQUIRE(hipMemcpy2DAsync(qkn + 2 * C, (size_t)3 * C * 2, s.qkv + 2 * C, (size_t)3 * C * 2, (size_t)C * 2, (size_t)M, hipMemcpyDeviceToDevice, st) ==
                         hipSuccess, "%s: copy of the v block failed", who);
        qkv_n = qkn;
    }
    TRY(attn_bwd_launch(qkv_n, s.ctx, s.lse, dctx, l.B, l.S, l.H, D, 1.0f / sqrtf((float)D), gq, ws + w.ad, w.ad_bytes, false, st));
    if (l.q_norm_w)   // in place on the q and k blocks of dqkv; the v block stays
        TRY(rms_bwd_launch(s.qkv, 3 * C, gq, 3 * C, l.q_norm_w, l.k_norm_w, 2, l.eps, M, C, gq, 3 * C, nullptr, 0, g.q_norm_w, g.k_norm_w, np,
                           w.np_bytes, st));
    if (g.qkv_w) {
        TRY(norm(x, l.norm1_w, l.norm1_b));
        TRY(gemm_wgrad_launch(gq, 3 * C, xn, C, (int)M, 3 * C, C, g.qkv_w, C, g.qkv_b, wg, w.wg_bytes, st));
        // CLIP: the k projection's bias has no gradient: it adds q_i . b_k to every score of query row i, and softmax does not see a shift
        // of a row.  What the column sum of the computed dK holds is rounding noise only (measured: 1e-3 of the other bias gradients' size,
        // as in torch's bf16 autograd), so the k block of grad_qkv_b is written as the exact value.  (InternViT keeps the column sum: behind
        // a QK-norm the k bias does reach the scores.)
        if (!l.rms && g.qkv_b) VLLM_REQUIRE(hipMemsetAsync(g.qkv_b + C, 0, (size_t)C * 2, st) == hipSuccess, "%s: memset failed", who);
    }
    if (!n1) return VLLM_OK;
    TRY(linear_dgrad(st, EPI_BIAS, gq, l.qkv_w, 3 * C, C, M, wt, ga, nullptr, sk, w.sk_bytes));
    return norm_bwd(x, ga, l.norm1_w, grad_x, grad_x ? g1 : nullptr, g.norm1_w, g.norm1_b);
}
}  // namespace

// ---- the two families' entry points: each fills the description from its own structs and passes its own name on ----
extern "C" int vllm_vit_layer_train_sizeof(void) { return (int)sizeof(VllmVitLayerTrain); }
extern "C" int vllm_vit_layer_saved_sizeof(void) { return (int)sizeof(VllmVitLayerSaved); }
extern "C" int vllm_vit_layer_grads_sizeof(void) { return (int)sizeof(VllmVitLayerGrads); }
extern "C" int vllm_clip_layer_train_sizeof(void) { return (int)sizeof(VllmClipLayerTrain); }
extern "C" int vllm_clip_layer_saved_sizeof(void) { return (int)sizeof(VllmClipLayerSaved); }
extern "C" int vllm_clip_layer_grads_sizeof(void) { return (int)sizeof(VllmClipLayerGrads); }

extern "C" long vllm_vit_layer_backward_workspace_bytes(const VllmVitLayerTrain *d, int B, int S)
{
    return workspace_bytes(layer(d, B, S), "vit_layer_backward_workspace_bytes");
}
extern "C" long vllm_clip_layer_backward_workspace_bytes(const VllmClipLayerTrain *d, int B, int S)
{
    return workspace_bytes(layer(d, B, S), "clip_layer_backward_workspace_bytes");
}

extern "C" int vllm_vit_layer_forward_train(const VllmVitLayerTrain *d, const uint16_t *x, int B, int S, uint16_t *out,
                                            const VllmVitLayerSaved *saved, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    return forward_train(layer(d, B, S), x, out, table(saved), workspace, ws_bytes, stream, "vit_layer_forward_train");
}
extern "C" int vllm_clip_layer_forward_train(const VllmClipLayerTrain *d, const uint16_t *x, int B, int S, uint16_t *out,
                                             const VllmClipLayerSaved *saved, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    return forward_train(layer(d, B, S), x, out, table(saved), workspace, ws_bytes, stream, "clip_layer_forward_train");
}

extern "C" int vllm_vit_layer_backward(const VllmVitLayerTrain *d, const uint16_t *x, int B, int S, const uint16_t *grad_out,
                                       const VllmVitLayerSaved *saved, uint16_t *grad_x, const VllmVitLayerGrads *grads, void *workspace,
                                       long ws_bytes, vllm_stream_t stream)
{
    return backward(layer(d, B, S), x, grad_out, table(saved), grad_x, table(grads), workspace, ws_bytes, stream, "vit_layer_backward");
}
extern "C" int vllm_clip_layer_backward(const VllmClipLayerTrain *d, const uint16_t *x, int B, int S, const uint16_t *grad_out,
                                        const VllmClipLayerSaved *saved, uint16_t *grad_x, const VllmClipLayerGrads *grads, void *workspace,
                                        long ws_bytes, vllm_stream_t stream)
{
    return backward(layer(d, B, S), x, grad_out, table(saved), grad_x, table(grads), workspace, ws_bytes, stream, "clip_layer_backward");
}
