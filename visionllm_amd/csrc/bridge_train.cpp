// Training the projector behind the C ABI (vl_bridge: modeling_visionllmv2.py:162-182, called with grad at :579; trained with
// freeze_vl_bridge=False, visionllmv2/train/train.py:162-170).  For Linear i: Y_i = A_{i-1} W_i^T + b_i, A_i = gelu(Y_i) between
// Linears; A_{-1} = x (or LayerNorm(x) for internvl_mlp).
//   forward_train: vllm_bridge_forward's GEMMs with the same schedules (out and every A_i bit-identical); the hidden Linears use
//     EPI_GELU_SAVE, which also stores H_i = Y_i (bf16) from the same fp32 accumulators.
//   backward, Linear by Linear from the last:  dW_i = dY_i^T A_{i-1}, db_i = colsum(dY_i)   (gemm_wgrad.hip)
//     dY_{i-1} = (dY_i W_i) * gelu'(H_{i-1})    (the bf16 GEMM with W_i^T as its weight and the EPI_GELU_BWD epilogue)
//     first Linear: dX = dY_0 W_0 (bf16), or for internvl_mlp dZ in fp32 (VLLM_EPI_F32) into the LayerNorm backward (bridge_bwd.hip).
// No allocation, no synchronisation, one stream; the workspace is the caller's.
#include <algorithm>
#include "orchestrate.hpp"

using namespace vllm;

namespace {
int check_train_desc(const VllmBridgeDesc *d, const char *who)
{
    VLLM_REQUIRE(d && d->depth >= 1 && d->depth <= 4, "%s: bad descriptor", who);
    VLLM_REQUIRE(d->pixel_shuffle == 0 && d->skip_cls == 0,
                 "%s: training takes the projector's input as forward(x) receives it (pixel_shuffle = skip_cls = 0); the fused select / "
                 "pixel-shuffle path is inference-only", who);
    VLLM_REQUIRE(d->kind == VLLM_BRIDGE_LINEAR ? d->depth == 1 : d->kind == VLLM_BRIDGE_INTERNVL_MLP ? d->depth == 2 : d->kind == VLLM_BRIDGE_MLP_GELU,
                 "%s: kind %d with depth %d", who, d->kind, d->depth);
    VLLM_REQUIRE(d->in_features > 0 && d->out_features > 0 && d->in_features % 64 == 0 && d->out_features % 64 == 0,
                 "%s: feature sizes must be multiples of 64", who);
    VLLM_REQUIRE(d->kind != VLLM_BRIDGE_INTERNVL_MLP || (d->ln_w && d->ln_b && aligned16(d->ln_w) && aligned16(d->ln_b) && d->in_features <= 16384),
                 "%s: internvl_mlp needs 16-byte aligned LayerNorm parameters (in_features <= 16384)", who);
    for (int i = 0; i < d->depth; ++i)
        VLLM_REQUIRE(d->w[i] && aligned16(d->w[i]) && (!d->b[i] || aligned16(d->b[i])), "%s: Linear %d: weight missing or parameters not 16-byte aligned", who, i);
    return VLLM_OK;
}

struct TrainWs { long wt, dy0, dy1, dz, wg, lnp, sk, sk_bytes, total; };
TrainWs train_ws_layout(const VllmBridgeDesc *d, long rows, bool need_gx)
{
    const long Cin = d->in_features, Cout = d->out_features;
    const bool ivl = d->kind == VLLM_BRIDGE_INTERNVL_MLP;
    TrainWs w;
    Carver cv;
    // (the sk slot first: the training forward uses only it, from the workspace's start)
    w.sk_bytes = rows >= 1024 ? SK_SCRATCH_BYTES : 0;   // stream-K tail of the 8-phase GEMM, as vllm_bridge_forward sizes it
    w.sk = cv.take(w.sk_bytes);
    w.wt = cv.take(Cout * std::max(d->depth > 1 ? Cout : 0L, (ivl || need_gx) ? Cin : 0L) * 2);   // W_i^T
    w.dy0 = cv.take(d->depth > 1 ? rows * Cout * 2 : 0);   // dY of the hidden Linears, ping-pong
    w.dy1 = cv.take(d->depth > 2 ? rows * Cout * 2 : 0);
    w.dz = cv.take(ivl ? rows * Cin * 4 : 0);              // LayerNorm output gradient, fp32
    long wg = 0;
    for (int i = 0; i < d->depth; ++i) wg = std::max(wg, gemm_wgrad_workspace_bytes((int)rows, (int)Cout, (int)(i == 0 ? Cin : Cout)));
    w.wg = cv.take(wg);
    w.lnp = cv.take(ivl ? ln_bwd_workspace_bytes(rows, (int)Cin) : 0);
    w.total = cv.off;
    return w;
}
}  // namespace

extern "C" long vllm_bridge_backward_workspace_bytes(const VllmBridgeDesc *d, long rows, int need_grad_x)
{
    if (check_train_desc(d, "bridge_backward_workspace_bytes") != VLLM_OK || rows < 0) return -1;
    return train_ws_layout(d, rows, need_grad_x != 0).total;
}

extern "C" int vllm_bridge_forward_train(const VllmBridgeDesc *d, const uint16_t *x, long rows, uint16_t *out, uint16_t *const *saved_pre,
                                         uint16_t *const *saved_act, uint16_t *saved_ln, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    TRY(check_train_desc(d, "bridge_forward_train"));
    VLLM_REQUIRE(rows >= 0 && rows < (1L << 31) / 4, "bridge_forward_train: rows=%ld", rows);
    if (rows == 0) return VLLM_OK;
    const int Cin = d->in_features, Cout = d->out_features;
    const bool ivl = d->kind == VLLM_BRIDGE_INTERNVL_MLP;
    VLLM_REQUIRE(x && out && aligned16(x) && aligned16(out), "bridge_forward_train: x and out must be 16-byte aligned device pointers");
    VLLM_REQUIRE(!ivl || (saved_ln && aligned16(saved_ln)), "bridge_forward_train: internvl_mlp needs saved_ln (16-byte aligned)");
    for (int i = 0; i + 1 < d->depth; ++i)
        VLLM_REQUIRE(saved_pre && saved_act && saved_pre[i] && saved_act[i] && aligned16(saved_pre[i]) && aligned16(saved_act[i]),
                     "bridge_forward_train: saved_pre[%d] / saved_act[%d] missing or not 16-byte aligned", i, i);
    const long sk_bytes = rows >= 1024 ? SK_SCRATCH_BYTES : 0;
    VLLM_REQUIRE(sk_bytes == 0 || (workspace && aligned16(workspace) && ws_bytes >= sk_bytes),
                 "bridge_forward_train: workspace too small (%ld < %ld bytes) or misaligned", ws_bytes, sk_bytes);
    hipStream_t st = (hipStream_t)stream;
    void *sk = sk_bytes ? workspace : nullptr;
    TRY(sk_scratch_reset(sk, st, "bridge_forward_train"));
    const uint16_t *in = x;
    if (ivl) {
        TRY(norm_bf16_launch(false, x, Cin, d->ln_w, d->ln_b, saved_ln, Cin, rows, Cin, d->ln_eps, st));
        in = saved_ln;
    }
    int K = Cin;
    for (int i = 0; i < d->depth; ++i) {
        const bool last = i == d->depth - 1;
        // the GEMM call of vllm_bridge_forward; a hidden Linear's epilogue also leaves its pre-activation for the backward
        GemmArgs a = gemm_args(in, K, d->w[i], K, d->b[i], last ? out : saved_act[i], Cout, rows, Cout, K);
        if (!last) a.pre = saved_pre[i];
        gemm_set_scratch(a, sk, sk_bytes);
        TRY(gemm_bf16_launch(last ? EPI_BIAS : EPI_GELU_SAVE, a, st));
        if (!last) in = saved_act[i];
        K = Cout;
    }
    return VLLM_OK;
}

extern "C" int vllm_bridge_backward(const VllmBridgeDesc *d, const uint16_t *x, long rows, const uint16_t *grad_out,
                                    const uint16_t *const *saved_pre, const uint16_t *const *saved_act, const uint16_t *saved_ln,
                                    uint16_t *grad_x, uint16_t *const *grad_w, uint16_t *const *grad_b, uint16_t *grad_ln_w,
                                    uint16_t *grad_ln_b, void *workspace, long ws_bytes, vllm_stream_t stream)
{
    TRY(check_train_desc(d, "bridge_backward"));
    VLLM_REQUIRE(rows >= 0 && rows < (1L << 31) / 4, "bridge_backward: rows=%ld", rows);
    const int Cin = d->in_features, Cout = d->out_features, D = d->depth;
    const bool ivl = d->kind == VLLM_BRIDGE_INTERNVL_MLP;
    VLLM_REQUIRE(grad_w, "bridge_backward: grad_w missing");
    for (int i = 0; i < D; ++i)
        VLLM_REQUIRE(grad_w[i] && aligned16(grad_w[i]) && (!grad_b || !grad_b[i] || aligned16(grad_b[i])),
                     "bridge_backward: grad_w[%d] missing, or a gradient not 16-byte aligned", i);
    VLLM_REQUIRE((!grad_ln_w || aligned16(grad_ln_w)) && (!grad_ln_b || aligned16(grad_ln_b)) && (!grad_x || aligned16(grad_x)),
                 "bridge_backward: gradients must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (rows == 0) {   // no rows: every parameter gradient is an empty sum
        for (int i = 0; i < D; ++i)
            TRY(zero_bf16(st, "bridge_backward", {{grad_w[i], (long)Cout * (i == 0 ? Cin : Cout)}, {grad_b ? grad_b[i] : nullptr, Cout}}));
        return zero_bf16(st, "bridge_backward", {{grad_ln_w, Cin}, {grad_ln_b, Cin}});
    }
    VLLM_REQUIRE(x && grad_out && aligned16(x) && aligned16(grad_out), "bridge_backward: x and grad_out must be 16-byte aligned device pointers");
    VLLM_REQUIRE(!ivl || (saved_ln && aligned16(saved_ln)), "bridge_backward: internvl_mlp needs saved_ln");
    for (int i = 0; i + 1 < D; ++i)
        VLLM_REQUIRE(saved_pre && saved_act && saved_pre[i] && saved_act[i] && aligned16(saved_pre[i]) && aligned16(saved_act[i]),
                     "bridge_backward: saved_pre[%d] / saved_act[%d] missing or not 16-byte aligned", i, i);
    const bool need_gx = grad_x != nullptr;
    const TrainWs w = train_ws_layout(d, rows, need_gx);
    // (a Linear bridge below the split and stream-K sizes with no grad_x needs none: NULL / 0 is accepted where the query answers 0)
    VLLM_REQUIRE(w.total == 0 || (workspace && aligned16(workspace) && ws_bytes >= w.total),
                 "bridge_backward: workspace too small (%ld < %ld bytes) or misaligned", ws_bytes, w.total);
    char *ws = (char *)workspace;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, "bridge_backward"));
    uint16_t *wt = (uint16_t *)(ws + w.wt);
    uint16_t *bufs[2] = {(uint16_t *)(ws + w.dy0), (uint16_t *)(ws + w.dy1)};
    const bool dx0 = need_gx || (ivl && (grad_ln_w || grad_ln_b));   // the first Linear's input gradient is needed
    const uint16_t *dy = grad_out;
    for (int i = D - 1; i >= 0; --i) {
        const int K = i == 0 ? Cin : Cout;
        const uint16_t *in = i > 0 ? saved_act[i - 1] : ivl ? saved_ln : x;
        TRY(gemm_wgrad_launch(dy, Cout, in, K, (int)rows, Cout, K, grad_w[i], K, grad_b ? grad_b[i] : nullptr, ws + w.wg,
                              w.total - w.wg, st));
        if (i > 0) {
            uint16_t *nxt = bufs[(D - 1 - i) & 1];
            TRY(linear_dgrad(st, EPI_GELU_BWD, dy, d->w[i], Cout, Cout, rows, wt, nxt, saved_pre[i - 1], sk, w.sk_bytes));
            dy = nxt;
        } else if (dx0) {
            if (ivl) {
                float *dz = (float *)(ws + w.dz);
                TRY(linear_dgrad(st, EPI_F32, dy, d->w[0], Cout, Cin, rows, wt, dz, nullptr, sk, w.sk_bytes));
                TRY(ln_bwd_launch(x, Cin, dz, Cin, d->ln_w, d->ln_eps, rows, Cin, grad_x, Cin, grad_ln_w, grad_ln_b, ws + w.lnp,
                                  w.total - w.lnp, st));
            } else {
                TRY(linear_dgrad(st, EPI_BIAS, dy, d->w[0], Cout, Cin, rows, wt, grad_x, nullptr, sk, w.sk_bytes));
            }
        }
    }
    return VLLM_OK;
}
