// The region encoder behind the C ABI, forward and backward (visionllmv2/model/region_encoder.py:68-147 with mask_pool_type =
// 'grid_sample'; trained by default, freeze_region_encoder=False).  Channels-last throughout; M1 = n (H / k)(W / k) rows after the first
// conv (k = patch / 2), M2 = M1 / 4 after the second, C1 = hidden / 4.
//   forward : im2col -> A1 [M1, Kpad];  y1 = A1 W1p^T + b1;  pre1, g1 = LayerNorm + GELU (y1);  y2 = g1 viewed [M2, 4 C1] times W2p^T + b2
//             (W2p: the 2 x 2 conv's weight permuted to (dy, dx, c), the order im2col leaves the four stage-1 pixels of a patch in);
//             pre2, g2 = LayerNorm + GELU (y2);  stem = g2 W3^T + b3;  pooling weights from the points;  pooled = the fused pooling of the
//             stem and the levels;  out = pooled Wu^T + bu.
//   backward: dWu, dbu = wgrad(grad_out, pooled);  dpooled = grad_out Wu;  dstem / grad_level_k = w_k (x) dpooled;  dW3, db3 = wgrad(dstem, g2);
//             dpre2 = (dstem W3) gelu'(pre2);  dy2, dln2 = LayerNorm backward(y2, dpre2);  dW2p, db2 = wgrad(dy2, g1 view) -> un-permuted;
//             dpre1 = (dy2 W2p) gelu'(pre1) on the [M2, 4 C1] view;  dy1, dln1 = LayerNorm backward(y1, dpre1);  dW1p, db1 = wgrad(dy1, A1)
//             -> unpadded.  No data gradient through the first conv.  The chain stops behind the deepest gradient that was asked for.
// No allocation, no synchronisation, one stream; the workspace is the caller's.
#include <algorithm>
#include "orchestrate.hpp"
#include "region_stem.hpp"

using namespace vllm;

namespace {

struct Dims { int hid, C1, E, O, k, K, kpad, n, H, W, h, w, HW, L, P; long M1, M2; };

int check_desc(const VllmRegionEncoder *d, Dims *q, const char *who)
{
    VLLM_REQUIRE(d, "%s: null descriptor", who);
    VLLM_REQUIRE(d->hidden > 0 && d->hidden % 4 == 0 && (d->hidden / 4) % 64 == 0 && d->hidden <= 2048 && ln_gelu_takes(d->hidden / 4) && ln_gelu_takes(d->hidden),
                 "%s: hidden %d: hidden / 4 and hidden must be multiples of 64 (hidden <= 2048)", who, d->hidden);
    VLLM_REQUIRE(d->embed > 0 && d->embed % 64 == 0 && d->out_dim > 0 && d->out_dim % 64 == 0, "%s: embed %d and out_dim %d must be multiples of 64", who,
                 d->embed, d->out_dim);
    VLLM_REQUIRE(d->patch > 0 && d->patch % 2 == 0 && d->patch <= 64, "%s: patch %d must be even (<= 64)", who, d->patch);
    VLLM_REQUIRE(d->H > 0 && d->W > 0 && d->H % d->patch == 0 && d->W % d->patch == 0, "%s: H %d and W %d must be multiples of patch %d", who, d->H, d->W,
                 d->patch);
    VLLM_REQUIRE(d->levels >= 1 && d->levels <= REGION_MAX_LEVELS, "%s: %d levels (1 .. 4)", who, d->levels);
    VLLM_REQUIRE(d->points >= 0 && d->n >= 0 && d->n <= 65535, "%s: n %d regions (<= 65535), %d points", who, d->n, d->points);
    VLLM_REQUIRE(d->pixel_is_f32 == 0 || d->pixel_is_f32 == 1, "%s: pixel_is_f32 %d", who, d->pixel_is_f32);
    q->hid = d->hidden; q->C1 = d->hidden / 4; q->E = d->embed; q->O = d->out_dim; q->k = d->patch / 2; q->K = 4 * q->k * q->k;
    q->kpad = (q->K + 63) / 64 * 64;
    q->n = d->n; q->H = d->H; q->W = d->W; q->h = d->H / d->patch; q->w = d->W / d->patch; q->HW = q->h * q->w; q->L = d->levels; q->P = d->points;
    VLLM_REQUIRE(region_pool_weights_fit(q->HW), "%s: a map of %d x %d positions (at most 4096 fit the pooling's LDS accumulators)", who, q->h, q->w);
    q->M2 = (long)q->n * q->HW; q->M1 = 4 * q->M2;
    VLLM_REQUIRE(q->M1 < (1L << 31) / 4, "%s: %ld stem rows (too many)", who, q->M1);
    return VLLM_OK;
}

// [sk: the GEMMs' stream-K scratch][w1p: W1 padded (forward) / dW1p (backward)][w2p: W2 permuted][dw2p][pw: the pooling weights, fp32]
// [wt: a transposed weight][dpool][dstem][d2: dpre2, dy2 in place][d1: dpre1, dy1 in place][wg: gemm_wgrad's split partials][lnp: the
// LayerNorm backward's partials]
struct Ws { long sk, sk_bytes, w1p, w2p, dw2p, pw, wt, dpool, dstem, d2, d1, wg, wg_bytes, lnp, lnp_bytes, total; };
Ws ws_layout(const Dims &q)
{
    Ws w;
    Carver cv;
    w.sk_bytes = q.M2 >= 1024 ? SK_SCRATCH_BYTES : 0;
    w.sk = cv.take(w.sk_bytes);
    w.w1p = cv.take((long)q.C1 * q.kpad * 2);
    w.w2p = cv.take((long)q.hid * 4 * q.C1 * 2);
    w.dw2p = cv.take((long)q.hid * 4 * q.C1 * 2);
    w.pw = cv.take((long)q.L * q.M2 * 4);
    w.wt = cv.take(std::max({(long)q.E * q.O, (long)q.hid * q.E, 4L * q.C1 * q.hid}) * 2);
    w.dpool = cv.take((long)q.n * q.E * 2);
    w.dstem = cv.take(q.M2 * q.E * 2);
    w.d2 = cv.take(q.M2 * q.hid * 2);
    w.d1 = cv.take(q.M1 * q.C1 * 2);
    w.wg_bytes = std::max({0L, gemm_wgrad_workspace_bytes(q.n, q.O, q.E), gemm_wgrad_workspace_bytes((int)q.M2, q.E, q.hid),
                           gemm_wgrad_workspace_bytes((int)q.M2, q.hid, 4 * q.C1), gemm_wgrad_workspace_bytes((int)q.M1, q.C1, q.kpad)});
    w.wg = cv.take(w.wg_bytes);
    w.lnp_bytes = std::max({0L, ln_res_bwd_workspace_bytes(q.M2, q.hid), ln_res_bwd_workspace_bytes(q.M1, q.C1)});
    w.lnp = cv.take(w.lnp_bytes);
    w.total = cv.off;
    return w;
}

int check_common(const VllmRegionEncoder *d, const Dims &q, const float *points, const uint8_t *valid, const VllmRegionEncoderSaved *s,
                 const void *workspace, long ws_bytes, const Ws &w, const char *who)
{
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "%s: workspace too small (%ld < %ld bytes), missing or misaligned", who, ws_bytes,
                 w.total);
    const uint16_t *const par[12] = {d->conv1_w, d->conv1_b, d->ln1_w, d->ln1_b, d->conv2_w, d->conv2_b, d->ln2_w, d->ln2_b, d->conv3_w, d->conv3_b,
                                     d->up_w, d->up_b};
    for (int i = 0; i < 12; ++i) VLLM_REQUIRE(par[i] && aligned16(par[i]), "%s: parameter %d missing or not 16-byte aligned", who, i);
    VLLM_REQUIRE(s && s->a1 && s->y1 && s->pre1 && s->g1 && s->y2 && s->pre2 && s->g2 && s->stem && s->pooled, "%s: a saved tensor is missing", who);
    VLLM_REQUIRE(aligned16(s->a1) && aligned16(s->y1) && aligned16(s->pre1) && aligned16(s->g1) && aligned16(s->y2) && aligned16(s->pre2) && aligned16(s->g2) &&
                     aligned16(s->stem) && aligned16(s->pooled), "%s: saved tensors must be 16-byte aligned", who);
    VLLM_REQUIRE(q.P == 0 || (points && valid && (reinterpret_cast<uintptr_t>(points) & 7u) == 0), "%s: points / valid missing, or points not 8-byte aligned", who);
    return VLLM_OK;
}

long g_calls = 0, g_wgrads = 0;

int wgrad(hipStream_t st, const uint16_t *dY, int ldy, const uint16_t *A, int lda, long M, int N, int K, uint16_t *dW, uint16_t *db, char *ws, const Ws &w)
{
    __atomic_fetch_add(&g_wgrads, 1, __ATOMIC_RELAXED);
    return gemm_wgrad_launch(dY, ldy, A, lda, (int)M, N, K, dW, K, db, ws + w.wg, w.wg_bytes, st);
}

}  // namespace

extern "C" int vllm_region_encoder_sizeof(void) { return (int)sizeof(VllmRegionEncoder); }
extern "C" int vllm_region_encoder_saved_sizeof(void) { return (int)sizeof(VllmRegionEncoderSaved); }
extern "C" int vllm_region_encoder_grads_sizeof(void) { return (int)sizeof(VllmRegionEncoderGrads); }
extern "C" long vllm_region_encoder_calls(void) { return __atomic_load_n(&g_calls, __ATOMIC_RELAXED); }
extern "C" long vllm_region_encoder_wgrad_launches(void) { return __atomic_load_n(&g_wgrads, __ATOMIC_RELAXED); }

extern "C" long vllm_region_encoder_workspace_bytes(const VllmRegionEncoder *d)
{
    Dims q;
    if (check_desc(d, &q, "region_encoder_workspace_bytes") != VLLM_OK) return -1;
    return ws_layout(q).total;
}

extern "C" int vllm_region_encoder_forward(const VllmRegionEncoder *d, const void *images, const void *masks, const float *points,
                                           const uint8_t *valid, uint16_t *out, const VllmRegionEncoderSaved *s, void *workspace, long ws_bytes,
                                           vllm_stream_t stream)
{
    const char *who = "region_encoder_forward";
    Dims q;
    TRY(check_desc(d, &q, who));
    if (q.n == 0) return VLLM_OK;
    const Ws w = ws_layout(q);
    TRY(check_common(d, q, points, valid, s, workspace, ws_bytes, w, who));
    VLLM_REQUIRE(images && masks && out && aligned16(out), "%s: null images / masks / out, or out not 16-byte aligned", who);
    VLLM_REQUIRE(((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(masks)) & (d->pixel_is_f32 ? 3u : 1u)) == 0,
                 "%s: images / masks not element aligned", who);
    RegionPoolArgs pa;
    char *ws = (char *)workspace;
    float *pw = (float *)(ws + w.pw);
    pa.maps = q.L + 1; pa.HW = q.HW; pa.C = q.E; pa.out = s->pooled;
    pa.x[0] = s->stem; pa.w[0] = pw; pa.row_stride[0] = q.E; pa.img_stride[0] = (long)q.HW * q.E;
    for (int l = 0; l < q.L; ++l) {
        VLLM_REQUIRE(d->level[l] && aligned16(d->level[l]) && d->level_row_stride[l] >= q.E && d->level_row_stride[l] % 8 == 0 && d->level_image_stride[l] % 8 == 0,
                     "%s: level %d missing, not 16-byte aligned, or with strides that are no multiples of 8 elements", who, l);
        pa.x[l + 1] = d->level[l]; pa.w[l + 1] = pw + (long)l * q.M2;
        pa.row_stride[l + 1] = d->level_row_stride[l]; pa.img_stride[l + 1] = d->level_image_stride[l];
    }
    hipStream_t st = (hipStream_t)stream;
    __atomic_fetch_add(&g_calls, 1, __ATOMIC_RELAXED);
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    uint16_t *w1p = (uint16_t *)(ws + w.w1p), *w2p = (uint16_t *)(ws + w.w2p);
    TRY(sk_scratch_reset(sk, st, who));
    TRY(pad_weight_launch(d->conv1_w, w1p, q.C1, q.K, q.kpad, st));
    TRY(region_wperm_launch(d->conv2_w, w2p, q.hid, 4 * q.C1, 0, st));
    TRY(region_im2col_launch(images, masks, d->pixel_is_f32, s->a1, q.n, q.H, q.W, q.k, q.kpad, st));
    GemmArgs a = gemm_args(s->a1, q.kpad, w1p, q.kpad, d->conv1_b, s->y1, q.C1, q.M1, q.C1, q.kpad);
    gemm_set_scratch(a, sk, w.sk_bytes);
    TRY(gemm_bf16_launch(EPI_BIAS, a, st));
    TRY(ln_gelu_launch(s->y1, q.C1, d->ln1_w, d->ln1_b, s->pre1, s->g1, q.M1, q.C1, d->eps, st));
    a = gemm_args(s->g1, 4 * q.C1, w2p, 4 * q.C1, d->conv2_b, s->y2, q.hid, q.M2, q.hid, 4 * q.C1);
    gemm_set_scratch(a, sk, w.sk_bytes);
    TRY(gemm_bf16_launch(EPI_BIAS, a, st));
    TRY(ln_gelu_launch(s->y2, q.hid, d->ln2_w, d->ln2_b, s->pre2, s->g2, q.M2, q.hid, d->eps, st));
    a = gemm_args(s->g2, q.hid, d->conv3_w, q.hid, d->conv3_b, s->stem, q.E, q.M2, q.E, q.hid);
    gemm_set_scratch(a, sk, w.sk_bytes);
    TRY(gemm_bf16_launch(EPI_BIAS, a, st));
    TRY(region_pool_weights_launch(points, valid, pw, q.n, q.L, q.h, q.w, q.P, st));
    TRY(region_pool_launch(pa, q.n, st));
    a = gemm_args(s->pooled, q.E, d->up_w, q.E, d->up_b, out, q.O, q.n, q.O, q.E);
    gemm_set_scratch(a, sk, w.sk_bytes);
    return gemm_bf16_launch(EPI_BIAS, a, st);
}

extern "C" int vllm_region_encoder_backward(const VllmRegionEncoder *d, const float *points, const uint8_t *valid, const uint16_t *grad_out,
                                            const VllmRegionEncoderSaved *s, const VllmRegionEncoderGrads *g, void *workspace, long ws_bytes,
                                            vllm_stream_t stream)
{
    const char *who = "region_encoder_backward";
    Dims q;
    TRY(check_desc(d, &q, who));
    VLLM_REQUIRE(g, "%s: grads missing", who);
    uint16_t *const gr[12] = {g->conv1_w, g->conv1_b, g->ln1_w, g->ln1_b, g->conv2_w, g->conv2_b, g->ln2_w, g->ln2_b, g->conv3_w, g->conv3_b, g->up_w, g->up_b};
    for (int i = 0; i < 12; ++i) VLLM_REQUIRE(aligned16(gr[i]), "%s: gradient %d not 16-byte aligned", who, i);
    for (int l = 0; l < REGION_MAX_LEVELS; ++l)
        VLLM_REQUIRE(aligned16(g->level[l]) && (l < q.L || !g->level[l]), "%s: grad level %d not 16-byte aligned, or beyond the levels", who, l);
    VLLM_REQUIRE((!g->conv1_b || g->conv1_w) && (!g->conv2_b || g->conv2_w) && (!g->conv3_b || g->conv3_w) && (!g->up_b || g->up_w),
                 "%s: a bias gradient comes out of its weight gradient's launch and needs the weight's pointer too", who);
    hipStream_t st = (hipStream_t)stream;
    if (q.n == 0)   // no regions: every parameter gradient is an empty sum
        return zero_bf16(st, who, {{g->conv1_w, (long)q.C1 * q.K}, {g->conv1_b, q.C1}, {g->ln1_w, q.C1}, {g->ln1_b, q.C1}, {g->conv2_w, (long)q.hid * 4 * q.C1},
                                   {g->conv2_b, q.hid}, {g->ln2_w, q.hid}, {g->ln2_b, q.hid}, {g->conv3_w, (long)q.E * q.hid}, {g->conv3_b, q.E},
                                   {g->up_w, (long)q.O * q.E}, {g->up_b, q.O}});
    const Ws w = ws_layout(q);
    TRY(check_common(d, q, points, valid, s, workspace, ws_bytes, w, who));
    VLLM_REQUIRE(grad_out && aligned16(grad_out), "%s: grad_out must be a 16-byte aligned device pointer", who);
    // how deep the chain has to go: 0 nothing behind up_dim, 1 the pooling's gradients, 2 conv3, 3 LayerNorm 2 / conv2, 4 LayerNorm 1 / conv1
    const bool lv = g->level[0] || g->level[1] || g->level[2] || g->level[3];
    const int depth = (g->conv1_w || g->ln1_w || g->ln1_b) ? 4 : (g->conv2_w || g->ln2_w || g->ln2_b) ? 3 : g->conv3_w ? 2 : lv ? 1 : 0;
    __atomic_fetch_add(&g_calls, 1, __ATOMIC_RELAXED);
    char *ws = (char *)workspace;
    void *sk = w.sk_bytes ? ws + w.sk : nullptr;
    TRY(sk_scratch_reset(sk, st, who));
    uint16_t *wt = (uint16_t *)(ws + w.wt);
    if (g->up_w) TRY(wgrad(st, grad_out, q.O, s->pooled, q.E, q.n, q.O, q.E, g->up_w, g->up_b, ws, w));
    if (depth == 0) return VLLM_OK;
    uint16_t *dpool = (uint16_t *)(ws + w.dpool), *dstem = (uint16_t *)(ws + w.dstem);
    float *pw = (float *)(ws + w.pw);
    TRY(linear_dgrad(st, EPI_BIAS, grad_out, d->up_w, q.O, q.E, q.n, wt, dpool, nullptr, sk, w.sk_bytes));
    TRY(region_pool_weights_launch(points, valid, pw, q.n, q.L, q.h, q.w, q.P, st));   // (the forward's weights, bit for bit)
    for (int l = 0; l < q.L; ++l)
        if (g->level[l]) TRY(region_outer_launch(pw + (long)l * q.M2, dpool, g->level[l], q.n, q.HW, q.E, st));
    if (depth < 2) return VLLM_OK;
    TRY(region_outer_launch(pw, dpool, dstem, q.n, q.HW, q.E, st));
    if (g->conv3_w) TRY(wgrad(st, dstem, q.E, s->g2, q.hid, q.M2, q.E, q.hid, g->conv3_w, g->conv3_b, ws, w));
    if (depth < 3) return VLLM_OK;
    uint16_t *d2 = (uint16_t *)(ws + w.d2), *d1 = (uint16_t *)(ws + w.d1);
    TRY(linear_dgrad(st, EPI_GELU_BWD, dstem, d->conv3_w, q.E, q.hid, q.M2, wt, d2, s->pre2, sk, w.sk_bytes));
    TRY(ln_res_bwd_launch(s->y2, q.hid, d2, q.hid, d->ln2_w, d->eps, q.M2, q.hid, d2, q.hid, nullptr, 0, g->ln2_w, g->ln2_b, ws + w.lnp, w.lnp_bytes, st));
    const int K2 = 4 * q.C1;
    if (g->conv2_w) {
        uint16_t *dw2p = (uint16_t *)(ws + w.dw2p);
        TRY(wgrad(st, d2, q.hid, s->g1, K2, q.M2, q.hid, K2, dw2p, g->conv2_b, ws, w));
        TRY(region_wperm_launch(dw2p, g->conv2_w, q.hid, K2, 1, st));
    }
    if (depth < 4) return VLLM_OK;
    uint16_t *w2p = (uint16_t *)(ws + w.w2p);
    TRY(region_wperm_launch(d->conv2_w, w2p, q.hid, K2, 0, st));
    TRY(linear_dgrad(st, EPI_GELU_BWD, d2, w2p, q.hid, K2, q.M2, wt, d1, s->pre1, sk, w.sk_bytes));
    TRY(ln_res_bwd_launch(s->y1, q.C1, d1, q.C1, d->ln1_w, d->eps, q.M1, q.C1, d1, q.C1, nullptr, 0, g->ln1_w, g->ln1_b, ws + w.lnp, w.lnp_bytes, st));
    if (g->conv1_w) {
        uint16_t *dw1p = (uint16_t *)(ws + w.w1p);
        TRY(wgrad(st, d1, q.C1, s->a1, q.kpad, q.M1, q.C1, q.kpad, dw1p, g->conv1_b, ws, w));
        TRY(unpad_weight_launch(dw1p, g->conv1_w, q.C1, q.K, q.kpad, st));
    }
    return VLLM_OK;
}
