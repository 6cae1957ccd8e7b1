// Training one InternViT encoder layer behind the C ABI (InternVisionEncoderLayer.forward, modeling_intern_vit.py:182-210, run under
// torch.utils.checkpoint by the encoder, :259-262; trained with freeze_vis_encoder=False, visionllmv2/train/train.py:163, 534).
//   forward_train: the statement order of vit.cpp WITHOUT folded norms --
//       xn1 = norm1(x) -> qkv = xn1 Wqkv^T (+ b) -> [q, k = q_norm(q), k_norm(k)] -> ctx, lse = attention(q, k, v)
//       -> x1 = x + (ctx Wproj^T + b) ls1   (EPI_RESIDUAL_SAVE: y1 = ctx Wproj^T + b leaves too)
//       -> xn2 = norm2(x1) -> a1 = gelu(h1), h1 = xn2 Wfc1^T + b   (EPI_GELU_SAVE) -> out = x1 + (a1 Wfc2^T + b) ls2   (y2 leaves too)
//   saved (caller buffers): qkv BEFORE the QK-norm, ctx, lse, y1, x1, h1, a1, y2.
//   recomputed in the backward, one norm launch each: xn1 = norm1(x), xn2 = norm2(x1), the post-norm q / k (with v copied beside them:
//       the attention backward reads one packed [M, 3C] tensor).  Saving them instead would add 2 (qk-norm: 5) x M x C x 2 bytes to the
//       (10 C + 4 I) x M bytes a layer keeps; a norm launch reads and writes 2 x M x C x 2 bytes once.
//   backward, from grad_out g:
//       gy2 = g ls2, grad_ls2 = sum g y2                                      (ls_bwd_kernel)
//       dWfc2 = gy2^T a1, db = colsum gy2;  dh1 = (gy2 Wfc2) gelu'(h1)         (gemm_wgrad; bf16 GEMM on Wfc2^T, EPI_GELU_BWD)
//       dWfc1 = dh1^T xn2;  dxn2 = dh1 Wfc1
//       g1 = norm2'(x1; dxn2) + g, grad_norm2                                  (rms_bwd_kernel, grad_res = g: x1's two uses in one rounding)
//       gy1 = g1 ls1, grad_ls1 = sum g1 y1;  dWproj = gy1^T ctx;  dctx = gy1 Wproj
//       dqkv = attention'(q, k, v, ctx, lse; dctx);  QK-norm backward in place on its q / k blocks (G = 2), grad_q_norm / grad_k_norm
//       dWqkv = dqkv^T xn1;  dxn1 = dqkv Wqkv;  grad_x = norm1'(x; dxn1) + g1, grad_norm1
//   A NULL gradient pointer skips that product, and everything only it needed.
// No allocation, no synchronisation, one stream; the workspace is the caller's.
#include <algorithm>
#include <math.h>
#include "orchestrate.hpp"

using namespace vllm;

namespace {
struct Dims { int C, H, D, I, B, S; long M; bool qkn; };

int check_layer(const VllmVitLayerTrain *d, int B, int S, Dims *o, const char *who)
{
    VLLM_REQUIRE(d, "%s: null descriptor", who);
    VLLM_REQUIRE(d->hidden > 0 && d->heads > 0 && d->hidden % d->heads == 0, "%s: hidden %d / heads %d", who, d->hidden, d->heads);
    const int hd = d->hidden / d->heads;
    VLLM_REQUIRE(hd == 64 || hd == 128, "%s: head_dim %d not supported by the attention kernels (64 or 128)", who, hd);
    VLLM_REQUIRE(d->inter > 0 && d->hidden % 64 == 0 && d->inter % 64 == 0 && d->hidden <= 8192,
                 "%s: hidden / intermediate must be multiples of 64, hidden <= 8192 (the row-wise backward kernels)", who);
    VLLM_REQUIRE(B >= 0 && S > 0 && (long)B * S < (1L << 31) / 4, "%s: B=%d S=%d", who, B, S);
    VLLM_REQUIRE(d->norm1_w && d->qkv_w && d->proj_w && d->proj_b && d->ls1 && d->norm2_w && d->fc1_w && d->fc1_b && d->fc2_w && d->fc2_b && d->ls2,
                 "%s: layer parameters missing", who);
    VLLM_REQUIRE((d->q_norm_w != nullptr) == (d->k_norm_w != nullptr), "%s: q_norm and k_norm come together", who);
    const void *ps[] = {d->norm1_w, d->qkv_w, d->qkv_b, d->q_norm_w, d->k_norm_w, d->proj_w, d->proj_b, d->ls1, d->norm2_w, d->fc1_w, d->fc1_b,
                        d->fc2_w, d->fc2_b, d->ls2};
    for (const void *p : ps) VLLM_REQUIRE(aligned16(p), "%s: parameters must be 16-byte aligned", who);
    o->C = d->hidden; o->H = d->heads; o->D = hd; o->I = d->inter; o->B = B; o->S = S; o->M = (long)B * S; o->qkn = d->q_norm_w != nullptr;
    return VLLM_OK;
}

int check_saved(const VllmVitLayerSaved *s, const char *who)
{
    VLLM_REQUIRE(s && s->qkv && s->ctx && s->lse && s->y1 && s->x1 && s->h1 && s->a1 && s->y2, "%s: saved buffers missing", who);
    const void *ps[] = {s->qkv, s->ctx, s->lse, s->y1, s->x1, s->h1, s->a1, s->y2};
    for (const void *p : ps) VLLM_REQUIRE(aligned16(p), "%s: saved buffers must be 16-byte aligned", who);
    return VLLM_OK;
}

// forward: [sk][xn][qkn]; backward: [sk][xn][qkn][ga][gb][gi][gq][wt][wg][np][ad]
struct Ws { long sk, sk_bytes, xn, qkn, ga, gb, gi, gq, wt, wg, wg_bytes, np, np_bytes, ad, ad_bytes, fwd_total, total; };
Ws ws_layout(const Dims &q)
{
    const long M = q.M, C = q.C, I = q.I;
    Ws w;
    Carver cv;
    w.sk_bytes = M >= 1024 ? SK_SCRATCH_BYTES : 0;   // stream-K tail of the 8-phase GEMM, as the other orchestrators size it
    w.sk = cv.take(w.sk_bytes);
    w.xn = cv.take(M * C * 2);                            // norm1(x) / norm2(x1)
    w.qkn = cv.take(q.qkn ? M * 3 * C * 2 : 0);           // post-norm q, k (forward) + v copied beside them (backward)
    w.fwd_total = cv.off;
    w.ga = cv.take(M * C * 2);                            // gy2, then gy1
    w.gb = cv.take(M * C * 2);                            // dxn2 -> g1 (in place), kept until norm1's backward
    w.gi = cv.take(M * I * 2);                            // dh1
    w.gq = cv.take(M * 3 * C * 2);                        // dqkv; its first M x C elements carry dctx / dxn1 around it
    w.wt = cv.take(std::max(3 * C * C, C * I) * 2);       // W^T of the input-gradient GEMM at hand
    const long wg = std::max({gemm_wgrad_workspace_bytes((int)M, (int)C, (int)I), gemm_wgrad_workspace_bytes((int)M, (int)I, (int)C),
                   gemm_wgrad_workspace_bytes((int)M, (int)C, (int)C), gemm_wgrad_workspace_bytes((int)M, (int)(3 * C), (int)C)});
    w.wg_bytes = std::max(0L, wg);
    w.wg = cv.take(w.wg_bytes);
    w.np_bytes = std::max(0L, rms_bwd_workspace_bytes(M, (int)C, 2));   // column-sum partials (G = 2 is the largest user)
    w.np = cv.take(w.np_bytes);
    w.ad_bytes = std::max(0L, vllm_attn_bwd_workspace_bytes(q.B, q.S, q.H, q.D));
    w.ad = cv.take(w.ad_bytes);
    w.total = cv.off;
    return w;
}
}  // namespace

extern "C" int vllm_vit_layer_train_sizeof(void) { return (int)sizeof(VllmVitLayerTrain); }
extern "C" int vllm_vit_layer_saved_sizeof(void) { return (int)sizeof(VllmVitLayerSaved); }
extern "C" int vllm_vit_layer_grads_sizeof(void) { return (int)sizeof(VllmVitLayerGrads); }

extern "C" long vllm_vit_layer_backward_workspace_bytes(const VllmVitLayerTrain *d, int B, int S)
{
    Dims q;
    if (check_layer(d, B, S, &q, "vit_layer_backward_workspace_bytes") != VLLM_OK) return -1;
    return ws_layout(q).total;
}

extern "C" int vllm_vit_layer_forward_train(const VllmVitLayerTrain *d, const uint16_t *x, int B, int S, uint16_t *out,
                                            const VllmVitLayerSaved *saved, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    Dims q;
    TRY(check_layer(d, B, S, &q, "vit_layer_forward_train"));
    if (q.M == 0) return VLLM_OK;
    TRY(check_saved(saved, "vit_layer_forward_train"));
    VLLM_REQUIRE(x && out && aligned16(x) && aligned16(out), "vit_layer_forward_train: x and out must be 16-byte aligned device pointers");
    const Ws w = ws_layout(q);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.fwd_total, "vit_layer_forward_train: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.fwd_total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int C = q.C, I = q.I;
    const long M = q.M;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, "vit_layer_forward_train"));
    uint16_t *xn = (uint16_t *)(ws + w.xn), *qkn = (uint16_t *)(ws + w.qkn);
    const VllmVitLayerSaved &s = *saved;

    TRY(norm_bf16_launch(true, x, C, d->norm1_w, nullptr, xn, C, M, C, d->eps, st));
    TRY(gemm(st, EPI_BIAS, xn, C, d->qkv_w, C, d->qkv_b, s.qkv, 3 * C, (int)M, 3 * C, C, nullptr, nullptr, 0, 0, 0, sk, w.sk_bytes));
    const uint16_t *qk = s.qkv;
    if (q.qkn) {   // out of place: the backward normalises the pre-norm q / k again
        TRY(norm_bf16_launch(true, s.qkv, 3 * C, d->q_norm_w, nullptr, qkn, 3 * C, M, C, d->eps, st, d->k_norm_w, 2));
        qk = qkn;
    }
    {
        AttnArgs a;
        a.q = qk; a.k = qk + C; a.v = s.qkv + 2 * C; a.out = s.ctx;
        a.q_bs = a.k_bs = a.v_bs = (long)q.S * 3 * C;
        a.q_ts = a.k_ts = a.v_ts = 3 * C;
        a.q_hs = a.k_hs = a.v_hs = q.D;
        a.B = q.B; a.S = q.S; a.H = q.H; a.nqt = 0;
        a.scale_log2e = (1.0f / sqrtf((float)q.D)) * 1.4426950408889634f;
        a.lse = s.lse;
        TRY(attn_fwd_launch(a, q.D, st));
    }
    // the three GEMMs whose epilogue also leaves its pre-activation / pre-LayerScale output for the backward
    auto gemm_save = [&](int epi, GemmArgs a, uint16_t *pre) {
        a.pre = pre;
        gemm_set_scratch(a, sk, w.sk_bytes);
        return gemm_bf16_launch(epi, a, st);
    };
    GemmArgs proj = gemm_args(s.ctx, C, d->proj_w, C, d->proj_b, s.x1, C, M, C, C);
    proj.scale = d->ls1; proj.res = x; proj.ldr = C;
    TRY(gemm_save(EPI_RESIDUAL_SAVE, proj, s.y1));
    TRY(norm_bf16_launch(true, s.x1, C, d->norm2_w, nullptr, xn, C, M, C, d->eps, st));
    TRY(gemm_save(EPI_GELU_SAVE, gemm_args(xn, C, d->fc1_w, C, d->fc1_b, s.a1, I, M, I, C), s.h1));
    GemmArgs fc2 = gemm_args(s.a1, I, d->fc2_w, I, d->fc2_b, out, C, M, C, I);
    fc2.scale = d->ls2; fc2.res = s.x1; fc2.ldr = C;
    TRY(gemm_save(EPI_RESIDUAL_SAVE, fc2, s.y2));
    return VLLM_OK;
}

extern "C" int vllm_vit_layer_backward(const VllmVitLayerTrain *d, const uint16_t *x, int B, int S, const uint16_t *grad_out,
                                       const VllmVitLayerSaved *saved, uint16_t *grad_x, const VllmVitLayerGrads *grads, void *workspace,
                                       long ws_bytes, vllm_stream_t stream)
{
    Dims q;
    TRY(check_layer(d, B, S, &q, "vit_layer_backward"));
    VLLM_REQUIRE(grads, "vit_layer_backward: null gradient table");
    const VllmVitLayerGrads &g = *grads;
    VLLM_REQUIRE((!g.qkv_b || (d->qkv_b && g.qkv_w)) && (!g.proj_b || g.proj_w) && (!g.fc1_b || g.fc1_w) && (!g.fc2_b || g.fc2_w),
                 "vit_layer_backward: a bias gradient comes out of its weight gradient's launch (pass both), and only for a bias the layer has");
    VLLM_REQUIRE(q.qkn || (!g.q_norm_w && !g.k_norm_w), "vit_layer_backward: the layer has no QK-norm");
    const void *gp[] = {grad_x, g.norm1_w, g.qkv_w, g.qkv_b, g.q_norm_w, g.k_norm_w, g.proj_w, g.proj_b, g.ls1, g.norm2_w, g.fc1_w, g.fc1_b,
                        g.fc2_w, g.fc2_b, g.ls2};
    for (const void *p : gp) VLLM_REQUIRE(aligned16(p), "vit_layer_backward: gradients must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int C = q.C, I = q.I;
    const long M = q.M;
    if (M == 0) {   // no rows: every parameter gradient is an empty sum
        return zero_bf16(st, "vit_layer_backward", {{g.norm1_w, C}, {g.qkv_w, 3L * C * C}, {g.qkv_b, 3L * C}, {g.q_norm_w, C}, {g.k_norm_w, C},
                                                    {g.proj_w, (long)C * C}, {g.proj_b, C}, {g.ls1, C}, {g.norm2_w, C}, {g.fc1_w, (long)I * C},
                                                    {g.fc1_b, I}, {g.fc2_w, (long)C * I}, {g.fc2_b, C}, {g.ls2, C}});
    }
    TRY(check_saved(saved, "vit_layer_backward"));
    VLLM_REQUIRE(x && grad_out && aligned16(x) && aligned16(grad_out), "vit_layer_backward: x and grad_out must be 16-byte aligned device pointers");
    const Ws w = ws_layout(q);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "vit_layer_backward: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.total);
    char *ws = (char *)workspace;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, "vit_layer_backward"));
    uint16_t *xn = (uint16_t *)(ws + w.xn), *qkn = (uint16_t *)(ws + w.qkn), *ga = (uint16_t *)(ws + w.ga), *gb = (uint16_t *)(ws + w.gb);
    uint16_t *gi = (uint16_t *)(ws + w.gi), *gq = (uint16_t *)(ws + w.gq), *wt = (uint16_t *)(ws + w.wt);
    void *wg = ws + w.wg, *np = ws + w.np;
    const VllmVitLayerSaved &s = *saved;

    // what has to be computed: a product is needed by its own gradient or by anything further up the chain
    const bool n1 = grad_x || g.norm1_w;                                   // norm1's backward (dxn1)
    const bool dq = n1 || g.qkv_w || g.q_norm_w || g.k_norm_w;             // dqkv (attention backward)
    const bool y1 = dq || g.proj_w;                                        // gy1
    const bool x1 = y1 || g.ls1;                                           // g1, the gradient at the mid hidden state
    const bool n2 = x1 || g.norm2_w;                                       // dxn2
    const bool h1 = n2 || g.fc1_w;                                         // dh1
    const bool y2 = h1 || g.fc2_w;                                         // gy2

    // ---- MLP block ----
    if (y2 || g.ls2) TRY(ls_bwd_launch(grad_out, C, s.y2, C, d->ls2, M, C, y2 ? ga : nullptr, C, g.ls2, np, w.np_bytes, st));
    if (g.fc2_w) TRY(gemm_wgrad_launch(ga, C, s.a1, I, (int)M, C, I, g.fc2_w, I, g.fc2_b, wg, w.wg_bytes, st));
    if (h1) TRY(linear_dgrad(st, EPI_GELU_BWD, ga, d->fc2_w, C, I, M, wt, gi, s.h1, sk, w.sk_bytes));
    if (g.fc1_w || n2) TRY(norm_bf16_launch(true, s.x1, C, d->norm2_w, nullptr, xn, C, M, C, d->eps, st));
    if (g.fc1_w) TRY(gemm_wgrad_launch(gi, I, xn, C, (int)M, I, C, g.fc1_w, C, g.fc1_b, wg, w.wg_bytes, st));
    const uint16_t *g1 = grad_out;
    if (n2) {
        TRY(linear_dgrad(st, EPI_BIAS, gi, d->fc1_w, I, C, M, wt, gb, nullptr, sk, w.sk_bytes));
        TRY(rms_bwd_launch(s.x1, C, gb, C, d->norm2_w, nullptr, 1, d->eps, M, C, x1 ? gb : nullptr, C, x1 ? grad_out : nullptr, C, g.norm2_w,
                           nullptr, np, w.np_bytes, st));
        g1 = gb;
    }
    if (!x1) return VLLM_OK;
    // ---- attention block ----
    TRY(ls_bwd_launch(g1, C, s.y1, C, d->ls1, M, C, y1 ? ga : nullptr, C, g.ls1, np, w.np_bytes, st));
    if (g.proj_w) TRY(gemm_wgrad_launch(ga, C, s.ctx, C, (int)M, C, C, g.proj_w, C, g.proj_b, wg, w.wg_bytes, st));
    if (!dq) return VLLM_OK;
    uint16_t *dctx = xn;   // (norm2(x1) has been consumed)
    TRY(linear_dgrad(st, EPI_BIAS, ga, d->proj_w, C, C, M, wt, dctx, nullptr, sk, w.sk_bytes));
    const uint16_t *qkv_n = s.qkv;
    if (q.qkn) {
        TRY(norm_bf16_launch(true, s.qkv, 3 * C, d->q_norm_w, nullptr, qkn, 3 * C, M, C, d->eps, st, d->k_norm_w, 2));
        VLLM_REQUIRE(hipMemcpy2DAsync(qkn + 2 * C, (size_t)3 * C * 2, s.qkv + 2 * C, (size_t)3 * C * 2, (size_t)C * 2, (size_t)M, hipMemcpyDeviceToDevice, st) ==
                         hipSuccess, "vit_layer_backward: copy of the v block failed");
        qkv_n = qkn;
    }
    TRY(attn_bwd_launch(qkv_n, s.ctx, s.lse, dctx, q.B, q.S, q.H, q.D, 1.0f / sqrtf((float)q.D), gq, ws + w.ad, w.ad_bytes, false, st));
    if (q.qkn)   // in place on the q and k blocks of dqkv; the v block stays
        TRY(rms_bwd_launch(s.qkv, 3 * C, gq, 3 * C, d->q_norm_w, d->k_norm_w, 2, d->eps, M, C, gq, 3 * C, nullptr, 0, g.q_norm_w, g.k_norm_w, np,
                           w.np_bytes, st));
    if (g.qkv_w || n1) TRY(norm_bf16_launch(true, x, C, d->norm1_w, nullptr, xn, C, M, C, d->eps, st));
    if (g.qkv_w) TRY(gemm_wgrad_launch(gq, 3 * C, xn, C, (int)M, 3 * C, C, g.qkv_w, C, g.qkv_b, wg, w.wg_bytes, st));
    if (!n1) return VLLM_OK;
    TRY(linear_dgrad(st, EPI_BIAS, gq, d->qkv_w, 3 * C, C, M, wt, ga, nullptr, sk, w.sk_bytes));
    TRY(rms_bwd_launch(x, C, ga, C, d->norm1_w, nullptr, 1, d->eps, M, C, grad_x, C, grad_x ? g1 : nullptr, C, g.norm1_w, nullptr, np, w.np_bytes, st));
    return VLLM_OK;
}
