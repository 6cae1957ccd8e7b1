// Training the embeddings of the vision tower behind the C ABI (InternVisionEmbeddings.forward, modeling_intern_vit.py:82-90; HF
// CLIPVisionEmbeddings with no conv bias; trained with freeze_vis_encoder=False, visionllmv2/train/train.py:163, 534).
//   forward : the embedding step of vit.cpp with the same kernels (im2col_patches -> GEMM with the EPI_EMBED epilogue -> cls_rows), in
//             front of it embed_pad_weight_kernel: the Conv2d weight [C, 3 ps^2] as the module stores it -> [C, kpad] zero padded.
//   backward, from G = grad_out [n, S = 1 + P, C]:
//       embed_tile_sum_kernel      one pass over G.  A thread owns a 16-byte column chunk of one position s and adds the n tiles in fp32 in
//                                  tile order (tile stride S C: a wave's 64 loads are 1 KiB contiguous, four tiles in flight per lane);
//                                  writes grad_pos[s] once, for s == 0 also grad_cls (the same sum: the same bits); for the conv bias a
//                                  block leaves the fp32 column sums over its s >= 1 positions in the workspace and
//       embed_bias_reduce_kernel   adds the blocks' partials in block order (ln_bwd / rms_bwd's scheme: no atomics, run-to-run identical).
//       embed_im2col_cls_kernel    im2col into [n S, kpad] with an all-zero row in every tile's CLS slot, so that G viewed as [n S, C] and
//                                  this matrix are both contiguous operands of gemm_wgrad (the CLS rows add exact zeros to dW; they would
//                                  NOT add zeros to a db taken from that launch, which is why the bias comes from the tile sums).
//       gemm_wgrad                 dW [C, kpad] into the workspace, then
//       embed_unpad_weight_kernel  [C, kpad] -> grad_patch_w [C, 3 ps^2]: 4-byte stores (2-byte for an odd row length) -- the row pitch
//                                  of 588 elements is not 16-byte aligned, and no element past the tensor is written.
// The backward keeps nothing from the forward: the im2col matrix is rebuilt from the pixels.  No allocation, no synchronisation, one stream.
#include <algorithm>
#include "common.hpp"
#include "orchestrate.hpp"

namespace vllm {
namespace {

constexpr int TS_ROWS = 8;   // positions per block of the tile-sum kernel: two per wave

// [C, K] -> [C, kpad], zero padded.  V = 2: K even, 4-byte moves (a row starts 4-byte aligned); V = 1: 2-byte moves.
template <int V>
__global__ __launch_bounds__(256) void embed_pad_weight_kernel(const uint16_t *__restrict__ w, uint16_t *__restrict__ wp, int C, int K, int kpad)
{
    const int per = kpad / V;
    const long n_el = (long)C * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % per) * V;
        const long c = i / per;
        if (V == 2) {
            uint32_t v = 0u;
            if (k < K) v = *reinterpret_cast<const uint32_t *>(w + c * K + k);
            *reinterpret_cast<uint32_t *>(wp + c * kpad + k) = v;
        } else {
            wp[c * kpad + k] = k < K ? w[c * K + k] : (uint16_t)0;
        }
    }
}

// [C, kpad] -> [C, K]: only the K live elements of a row are stored
template <int V>
__global__ __launch_bounds__(256) void embed_unpad_weight_kernel(const uint16_t *__restrict__ wp, uint16_t *__restrict__ w, int C, int K, int kpad)
{
    const int per = K / V;
    const long n_el = (long)C * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % per) * V;
        const long c = i / per;
        if (V == 2) *reinterpret_cast<uint32_t *>(w + c * K + k) = *reinterpret_cast<const uint32_t *>(wp + c * kpad + k);
        else w[c * K + k] = wp[c * kpad + k];
    }
}

// im2col_kernel (embed.hip) with the rows of tile n at n S + 1 + p and row n S zeroed.  Items [0, nseg): one (patch, channel, ky) row
// segment of `ps` pixels; items behind them: one 16-byte chunk of a CLS row.
template <typename PIX>
__global__ __launch_bounds__(256) void embed_im2col_cls_kernel(const PIX *__restrict__ px, uint16_t *__restrict__ A, int N, int img, int ps,
                                                               int g /*patches per side*/, int Kpad)
{
    const int P = g * g, S = P + 1;
    const long nseg = (long)N * P * 3 * ps;
    const int K = 3 * ps * ps, kch = Kpad / 8;
    const long nitem = nseg + (long)N * kch;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nitem; i += (long)gridDim.x * blockDim.x) {
        if (i >= nseg) {
            const long q = i - nseg;
            const long n = q / kch;
            const int ch = (int)(q - n * kch);
            *reinterpret_cast<uint4_t *>(A + n * S * Kpad + ch * 8) = (uint4_t){0u, 0u, 0u, 0u};
            continue;
        }
        const int ky = (int)(i % ps);
        long t = i / ps;
        const int c = (int)(t % 3);
        t /= 3;
        const int p = (int)(t % P);
        const int n = (int)(t / P);
        const int pyy = p / g, pxx = p % g;
        const PIX *src = px + (((long)n * 3 + c) * img + (pyy * ps + ky)) * img + pxx * ps;
        uint16_t *row = A + ((long)n * S + 1 + p) * Kpad;
        uint16_t *dst = row + c * ps * ps + ky * ps;
        for (int kx = 0; kx < ps; ++kx) {
            if constexpr (sizeof(PIX) == 2) dst[kx] = (uint16_t)src[kx];
            else dst[kx] = f32_to_bf16((float)src[kx]);
        }
        if (c == 2 && ky == ps - 1)
            for (int k = K; k < Kpad; ++k) row[k] = 0;
    }
}

__device__ __forceinline__ void add_bf16x8(const uint4_t &v, float (&a)[8])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[2 * e] += bf16lo_to_f32(v[e]); a[2 * e + 1] += bf16hi_to_f32(v[e]); }
}

// grid (ceil(C / 8 / 64), ceil(S / TS_ROWS)); 4 waves.  Lane l of every wave owns column chunk blockIdx.x * 64 + l; wave w owns the
// positions s0 + w, s0 + w + 4 of the block's TS_ROWS.  gpos / gcls / part may each be NULL (block-uniform).
__global__ __launch_bounds__(256) void embed_tile_sum_kernel(const uint16_t *__restrict__ G, int n, int S, int C, uint16_t *__restrict__ gpos,
                                                             uint16_t *__restrict__ gcls, float *__restrict__ part)
{
    __shared__ float red[4][8][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ck = blockIdx.x * 64 + lane;
    const bool live = ck < (C >> 3);
    const long tile = (long)S * C;
    const int s0 = blockIdx.y * TS_ROWS, s1 = s0 + TS_ROWS < S ? s0 + TS_ROWS : S;
    float b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = s0 + wave; s < s1; s += 4) {
        if (!live) continue;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const uint16_t *p = G + (long)s * C + ck * 8;
        int t = 0;
        for (; t + 4 <= n; t += 4) {   // four tiles in flight, added in tile order
            const uint4_t v0 = *reinterpret_cast<const uint4_t *>(p + (t + 0) * tile), v1 = *reinterpret_cast<const uint4_t *>(p + (t + 1) * tile);
            const uint4_t v2 = *reinterpret_cast<const uint4_t *>(p + (t + 2) * tile), v3 = *reinterpret_cast<const uint4_t *>(p + (t + 3) * tile);
            add_bf16x8(v0, acc); add_bf16x8(v1, acc); add_bf16x8(v2, acc); add_bf16x8(v3, acc);
        }
        for (; t < n; ++t) add_bf16x8(*reinterpret_cast<const uint4_t *>(p + t * tile), acc);
        const uint4_t o = {pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]), pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7])};
        if (gpos) *reinterpret_cast<uint4_t *>(gpos + (long)s * C + ck * 8) = o;
        if (s == 0) {
            if (gcls) *reinterpret_cast<uint4_t *>(gcls + ck * 8) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) b[e] += acc[e];
        }
    }
    if (!part) return;   // (block-uniform: no barrier is skipped by a part of the block)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][e][lane] = b[e];
    __syncthreads();
    if (wave == 0 && live) {
        float *pp = part + (size_t)blockIdx.y * C + ck * 8;
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((red[0][e][lane] + red[1][e][lane]) + red[2][e][lane]) + red[3][e][lane];
        *reinterpret_cast<float4_t *>(pp) = (float4_t){o[0], o[1], o[2], o[3]};
        *reinterpret_cast<float4_t *>(pp + 4) = (float4_t){o[4], o[5], o[6], o[7]};
    }
}

// gb[c] = bf16(part[0][c] + part[1][c] + ...), in block order
__global__ __launch_bounds__(256) void embed_bias_reduce_kernel(const float *__restrict__ part, int nb, int C, uint16_t *__restrict__ gb)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int b = 0; b < nb; ++b) s += part[(size_t)b * C + c];
    gb[c] = f32_to_bf16(s);
}

inline unsigned grid_for(long n)
{
    long b = (n + 255) / 256;
    if (b > 256L * 16) b = 256L * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

struct Dims { int C, ps, img, g, P, S, K, kpad; };

int check_embed(const VllmVitEmbed *d, int n, Dims *o, const char *who)
{
    VLLM_REQUIRE(d, "%s: null descriptor", who);
    VLLM_REQUIRE(d->hidden > 0 && d->hidden % 64 == 0 && d->hidden <= 8192, "%s: hidden %d must be a positive multiple of 64, <= 8192", who, d->hidden);
    VLLM_REQUIRE(d->patch > 0 && d->patch <= 64 && d->image > 0 && d->image % d->patch == 0, "%s: image %d not divisible by patch %d (patch <= 64)", who,
                 d->image, d->patch);
    VLLM_REQUIRE(d->pixel_is_f32 == 0 || d->pixel_is_f32 == 1, "%s: pixel_is_f32 %d", who, d->pixel_is_f32);
    VLLM_REQUIRE(d->patch_w && d->cls && d->pos, "%s: embedding parameters missing", who);
    VLLM_REQUIRE(aligned16(d->patch_w) && aligned16(d->patch_b) && aligned16(d->cls) && aligned16(d->pos), "%s: parameters must be 16-byte aligned", who);
    o->C = d->hidden; o->ps = d->patch; o->img = d->image; o->g = d->image / d->patch;
    VLLM_REQUIRE(o->g <= 1024, "%s: more than 1024 patches per side", who);
    o->P = o->g * o->g; o->S = o->P + 1; o->K = 3 * d->patch * d->patch; o->kpad = (o->K + 63) / 64 * 64;
    VLLM_REQUIRE(n >= 0 && (long)n * o->S < (1L << 31) / 4, "%s: n_tiles %d (too many tokens)", who, n);
    return VLLM_OK;
}

// [sk: the forward GEMM's stream-K scratch, as vit.cpp reserves it][wp: the padded weight (forward) / dW (backward)]
// [col: the im2col matrix, n P rows (forward) / n S rows (backward)][wg: gemm_wgrad's split partials][bp: the bias partials]
struct Ws { long sk, wp, col, wg, wg_bytes, bp, nb, total; };
Ws ws_layout(const Dims &q, int n)
{
    Ws w;
    Carver cv;
    w.sk = cv.take(SK_SCRATCH_BYTES);
    w.wp = cv.take((long)q.C * q.kpad * 2);
    w.col = cv.take((long)n * q.S * q.kpad * 2);
    w.wg_bytes = std::max(0L, gemm_wgrad_workspace_bytes((int)((long)n * q.S), q.C, q.kpad));
    w.wg = cv.take(w.wg_bytes);
    w.nb = (q.S + TS_ROWS - 1) / TS_ROWS;
    w.bp = cv.take(w.nb * q.C * 4);
    w.total = cv.off;
    return w;
}

}  // namespace

// A Conv2d weight [C, K] as the module stores it <-> the K-padded copy [C, kpad] a GEMM reads (also the region encoder's first conv)
int pad_weight_launch(const uint16_t *w, uint16_t *wp, int C, int K, int kpad, hipStream_t st)
{
    if (K % 2 == 0) VLLM_LAUNCH((embed_pad_weight_kernel<2>), dim3(grid_for((long)C * kpad / 2)), dim3(256), 0, st, w, wp, C, K, kpad);
    else VLLM_LAUNCH((embed_pad_weight_kernel<1>), dim3(grid_for((long)C * kpad)), dim3(256), 0, st, w, wp, C, K, kpad);
    VLLM_CHECK_LAUNCH("embed_pad_weight_kernel");
    return VLLM_OK;
}
int unpad_weight_launch(const uint16_t *wp, uint16_t *w, int C, int K, int kpad, hipStream_t st)
{
    if (K % 2 == 0) VLLM_LAUNCH((embed_unpad_weight_kernel<2>), dim3(grid_for((long)C * K / 2)), dim3(256), 0, st, wp, w, C, K, kpad);
    else VLLM_LAUNCH((embed_unpad_weight_kernel<1>), dim3(grid_for((long)C * K)), dim3(256), 0, st, wp, w, C, K, kpad);
    VLLM_CHECK_LAUNCH("embed_unpad_weight_kernel");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_vit_embed_sizeof(void) { return (int)sizeof(VllmVitEmbed); }

extern "C" long vllm_vit_embed_workspace_bytes(const VllmVitEmbed *d, int n_tiles)
{
    Dims q;
    if (check_embed(d, n_tiles, &q, "vit_embed_workspace_bytes") != VLLM_OK) return -1;
    return ws_layout(q, n_tiles).total;
}

extern "C" int vllm_vit_embed_forward(const VllmVitEmbed *d, const void *pixels, int n, uint16_t *out, void *workspace, long ws_bytes,
                                      vllm_stream_t stream)
{
    Dims q;
    TRY(check_embed(d, n, &q, "vit_embed_forward"));
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(pixels && out && aligned16(out), "vit_embed_forward: null pixels / out, or out not 16-byte aligned");
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(pixels) & (d->pixel_is_f32 ? 3u : 1u)) == 0, "vit_embed_forward: pixels not element aligned");
    const Ws w = ws_layout(q, n);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "vit_embed_forward: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    void *sk = ws + w.sk;
    uint16_t *wp = (uint16_t *)(ws + w.wp), *col = (uint16_t *)(ws + w.col);
    const int C = q.C;
    TRY(sk_scratch_reset(sk, st, "vit_embed_forward"));
    TRY(pad_weight_launch(d->patch_w, wp, C, q.K, q.kpad, st));
    // the statements of vllm_vit_forward's embedding step
    TRY(im2col_launch(pixels, d->pixel_is_f32, col, n, q.img, q.ps, q.kpad, st));
    TRY(gemm(st, EPI_EMBED, col, q.kpad, wp, q.kpad, d->patch_b, out, C, n * q.P, C, q.kpad, nullptr, d->pos, C, q.P, 0, sk, SK_SCRATCH_BYTES));
    TRY(cls_rows_launch(d->cls, d->pos, out, n, q.S, C, st));
    return VLLM_OK;
}

extern "C" int vllm_vit_embed_backward(const VllmVitEmbed *d, const void *pixels, int n, const uint16_t *grad_out, uint16_t *grad_patch_w,
                                       uint16_t *grad_patch_b, uint16_t *grad_cls, uint16_t *grad_pos, void *workspace, long ws_bytes,
                                       vllm_stream_t stream)
{
    Dims q;
    TRY(check_embed(d, n, &q, "vit_embed_backward"));
    VLLM_REQUIRE(!grad_patch_b || d->patch_b, "vit_embed_backward: grad_patch_b for a convolution that has no bias");
    VLLM_REQUIRE(aligned16(grad_patch_w) && aligned16(grad_patch_b) && aligned16(grad_cls) && aligned16(grad_pos),
                 "vit_embed_backward: gradients must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int C = q.C, S = q.S;
    if (n == 0) {   // no tiles: every gradient is an empty sum
        return zero_bf16(st, "vit_embed_backward", {{grad_patch_w, (long)C * q.K}, {grad_patch_b, C}, {grad_cls, C}, {grad_pos, (long)S * C}});
    }
    const bool sums = grad_patch_b || grad_cls || grad_pos;
    if (!sums && !grad_patch_w) return VLLM_OK;
    VLLM_REQUIRE(grad_out && aligned16(grad_out), "vit_embed_backward: grad_out must be a 16-byte aligned device pointer");
    VLLM_REQUIRE(!grad_patch_w || (pixels && (reinterpret_cast<uintptr_t>(pixels) & (d->pixel_is_f32 ? 3u : 1u)) == 0),
                 "vit_embed_backward: null pixels, or not element aligned");
    const Ws w = ws_layout(q, n);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "vit_embed_backward: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.total);
    char *ws = (char *)workspace;
    if (sums) {
        float *part = grad_patch_b ? (float *)(ws + w.bp) : nullptr;
        const dim3 grid((unsigned)ceil_div(C / 8, 64), (unsigned)w.nb);
        VLLM_LAUNCH(embed_tile_sum_kernel, grid, dim3(256), 0, st, grad_out, n, S, C, grad_pos, grad_cls, part);
        VLLM_CHECK_LAUNCH("embed_tile_sum_kernel");
        if (grad_patch_b) {
            VLLM_LAUNCH(embed_bias_reduce_kernel, dim3((unsigned)ceil_div(C, 256)), dim3(256), 0, st, part, (int)w.nb, C, grad_patch_b);
            VLLM_CHECK_LAUNCH("embed_bias_reduce_kernel");
        }
    }
    if (!grad_patch_w) return VLLM_OK;
    uint16_t *dw = (uint16_t *)(ws + w.wp), *col = (uint16_t *)(ws + w.col);
    const long nitem = (long)n * q.P * 3 * q.ps + (long)n * (q.kpad / 8);
    if (d->pixel_is_f32)
        VLLM_LAUNCH((embed_im2col_cls_kernel<float>), dim3(grid_for(nitem)), dim3(256), 0, st, (const float *)pixels, col, n, q.img, q.ps, q.g, q.kpad);
    else
        VLLM_LAUNCH((embed_im2col_cls_kernel<uint16_t>), dim3(grid_for(nitem)), dim3(256), 0, st, (const uint16_t *)pixels, col, n, q.img, q.ps, q.g, q.kpad);
    VLLM_CHECK_LAUNCH("embed_im2col_cls_kernel");
    TRY(gemm_wgrad_launch(grad_out, C, col, q.kpad, (int)((long)n * S), C, q.kpad, dw, q.kpad, nullptr, ws + w.wg, w.wg_bytes, st));
    return unpad_weight_launch(dw, grad_patch_w, C, q.K, q.kpad, st);
}
