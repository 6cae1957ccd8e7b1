// Region encoder, native route (visionllmv2/model/region_encoder.py:76-84, 99-147 with mask_pool_type='grid_sample'): the kernels that
// tie the mask stem and the level pooling into one channels-last chain (orchestrated by region_train.cpp).
//   region_im2col_kernel        images [n,3,H,W] + masks [n,1,H,W] -> A1 [n (H/k)(W/k), Kpad] bf16, rows ordered (n, y2, x2, dy, dx): the
//                               four stage-1 pixels of one stage-2 patch are adjacent, so the second conv's im2col is a reshape of the
//                               first conv's output.  Columns (c, ky, kx) as the Conv2d weight stores them; pad columns are zeros.
//   ln_gelu_kernel              LayerNorm over short rows (C = 64: eight rows per wave, C = 256: two) + erf GELU of the ROUNDED value.
//   region_wperm_kernel         the second conv's weight [hid, C1, 2, 2] <-> [hid, (dy, dx, c)] (the first conv's is padded / unpadded by
//                               the embeddings' kernels, embed_train.hip).
//   region_pool_weights_kernel  w_k[n, pix] = (1/L) sum_{l >= k} A_l[n, pix] / cnt_l, A_l the corner-weight sums of point_sample.hip.
//   region_pool_kernel          pooled[n, c] = sum_pix (w_0 stem + sum_k w_k level_k)[n, pix, c]: fp32, one bf16 rounding, fixed order.
//   region_outer_kernel         grad_map[n, pix, c] = bf16(w_k[n, pix] g[n, c]): every element written once.
// No atomics on any output (the 64-bit integer LDS atomics of the scatter commute exactly): the same bits on every run.
#include "common.hpp"
#include "kernels.hpp"
#include "point_sample_geo.hpp"
#include "region_stem.hpp"

namespace vllm {
namespace {

inline unsigned grid_for(long n)
{
    long b = (n + 255) / 256;
    if (b > 256L * 16) b = 256L * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// one thread per (row, 8-column chunk): a 16-byte store, every element of A1 written exactly once
template <typename PIX>
__global__ __launch_bounds__(256) void region_im2col_kernel(const PIX *__restrict__ img, const PIX *__restrict__ msk, uint16_t *__restrict__ A,
                                                            int n, int H, int W, int k, int Kpad)
{
    const int h2 = H / (2 * k), w2 = W / (2 * k), kk = k * k, K = 4 * kk, kch = Kpad / 8;
    const long items = (long)n * h2 * w2 * 4 * kch;
    const long plane = (long)H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % kch);
        long r = i / kch;                       // row = (((img_n * h2 + y2) * w2 + x2) * 2 + dy) * 2 + dx
        const int dx = (int)(r & 1), dy = (int)((r >> 1) & 1);
        long t = r >> 2;
        const int x2 = (int)(t % w2);
        t /= w2;
        const int y2 = (int)(t % h2);
        const long in = t / h2;
        const int py = (2 * y2 + dy) * k, px = (2 * x2 + dx) * k;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = ch * 8 + e;
            v[e] = 0.f;
            if (col < K) {
                const int c = col / kk, rem = col - c * kk, ky = rem / k, kx = rem - ky * k;
                const long off = (long)(py + ky) * W + px + kx;
                PIX s = c < 3 ? img[(in * 3 + c) * plane + off] : msk[in * plane + off];
                if constexpr (sizeof(PIX) == 2) v[e] = bf16_to_f32((uint16_t)s);
                else v[e] = (float)s;
            }
        }
        const uint4_t o = pack8(v);
        *reinterpret_cast<uint4_t *>(A + r * Kpad + ch * 8) = o;
    }
}

// G lanes share a row (G a power of two, 8 .. 64), lane j of the group owns the 16-byte chunks j, j + G, ... (nch <= LG_NCH of them);
// 64 / G rows per wave, four waves per block.  Reductions are xor shuffles inside the lane group: fixed order.
constexpr int LG_NCH = 8;
template <int G>
__global__ __launch_bounds__(256) void ln_gelu_kernel(const uint16_t *__restrict__ x, int ldx, const uint16_t *__restrict__ w,
                                                      const uint16_t *__restrict__ b, uint16_t *__restrict__ pre, uint16_t *__restrict__ y,
                                                      long rows, int C, float eps)
{
    constexpr int R = 64 / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % G;
    const long row = ((long)blockIdx.x * 4 + wave) * R + lane / G;
    const bool live = row < rows;
    const int nch = C / (8 * G);
    float v[LG_NCH][8];
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < LG_NCH; ++q) {
        if (q < nch) {
            uint4_t ld = {0u, 0u, 0u, 0u};
            if (live) ld = *reinterpret_cast<const uint4_t *>(x + row * ldx + (q * G + j) * 8);
            unpack8(ld, v[q]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[q][e];
        }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float m2 = 0.f;
#pragma unroll
    for (int q = 0; q < LG_NCH; ++q) {
        if (q < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[q][e] -= mean; m2 += v[q][e] * v[q][e]; }
        }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) m2 += __shfl_xor(m2, o);
    const float r = 1.0f / sqrtf(m2 / (float)C + eps);
    if (!live) return;
#pragma unroll
    for (int q = 0; q < LG_NCH; ++q) {
        if (q < nch) {
            const int c0 = (q * G + j) * 8;
            float gw[8], gb[8], p[8], a[8];
            unpack8(*reinterpret_cast<const uint4_t *>(w + c0), gw);
            unpack8(*reinterpret_cast<const uint4_t *>(b + c0), gb);
#pragma unroll
            for (int e = 0; e < 8; ++e) p[e] = v[q][e] * r * gw[e] + gb[e];
            const uint4_t po = pack8(p);
            if (pre) *reinterpret_cast<uint4_t *>(pre + row * C + c0) = po;
            float pr[8];
            unpack8(po, pr);   // the GELU of the ROUNDED value: what the backward's gelu'(saved pre) differentiates
#pragma unroll
            // 0.5 x erfc(-x / sqrt 2) = 0.5 x (1 + erf(x / sqrt 2)) without the cancellation of 1 + erf in the negative tail
            for (int e = 0; e < 8; ++e) a[e] = 0.5f * pr[e] * erfcf(pr[e] * -0.70710678118654752440f);
            const uint4_t yo = pack8(a);
            *reinterpret_cast<uint4_t *>(y + row * C + c0) = yo;
        }
    }
}

// The 2 x 2 conv's weight [R, C1, 2, 2].  inverse = 0: dst [R, (q, c)] = src [R, (c, q)], q = 2 dy + dx, K = 4 C1 columns;  1: back.
__global__ __launch_bounds__(256) void region_wperm_kernel(const uint16_t *__restrict__ src, uint16_t *__restrict__ dst, int R, int K, int inverse)
{
    const long n_el = (long)R * K;
    const int C1 = K / 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % K);
        const long r = i / K;
        dst[i] = src[r * K + (inverse ? (col % 4) * C1 + col / 4 : (col % C1) * 4 + col / C1)];
    }
}

// grid (n), RPW_THREADS threads: a region's 2304 points of a level in three rounds (the kernel is one latency chain per level).
// LDS: [HW] 64-bit sums, [HW] running suffix sums.  Levels are walked from the last to the first, so that the running sum at level k is
// A_{L-1}/cnt_{L-1} + ... + A_k/cnt_k  (added in that order); w_k = that / L.
constexpr int RPW_THREADS = 1024;
__global__ __launch_bounds__(RPW_THREADS) void region_pool_weights_kernel(const float *__restrict__ coords, const uint8_t *__restrict__ valid,
                                                                  float *__restrict__ wout, int n_img, int L, int H, int W, int P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long rp_acc[];
    __shared__ int s_cnt;
    const int HW = H * W, tid = threadIdx.x, lane = tid & 63;
    float *run = reinterpret_cast<float *>(rp_acc + ((HW + 1) & ~1));
    const long n = blockIdx.x;
    for (int i = tid; i < HW; i += RPW_THREADS) run[i] = 0.f;
    for (int l = L - 1; l >= 0; --l) {
        for (int i = tid; i < HW; i += RPW_THREADS) rp_acc[i] = 0ull;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        int cnt = 0;
        const long base = ((long)l * n_img + n) * P;
        for (int p = tid; p < P; p += RPW_THREADS) {
            if (!valid[base + p]) continue;
            const float2_t xy = *reinterpret_cast<const float2_t *>(coords + (base + p) * 2);
            const PsGeo g = ps_geo(xy.x, xy.y, H, W);
            ++cnt;
            if (g.w00 != 0.f) atomicAdd(rp_acc + g.o00, (unsigned long long)(g.w00 * PS_FIX_SCALE));
            if (g.w01 != 0.f) atomicAdd(rp_acc + g.o01, (unsigned long long)(g.w01 * PS_FIX_SCALE));
            if (g.w10 != 0.f) atomicAdd(rp_acc + g.o10, (unsigned long long)(g.w10 * PS_FIX_SCALE));
            if (g.w11 != 0.f) atomicAdd(rp_acc + g.o11, (unsigned long long)(g.w11 * PS_FIX_SCALE));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        const int tc = s_cnt;
        float *wl = wout + ((long)l * n_img + n) * HW;
        for (int i = tid; i < HW; i += RPW_THREADS) {
            const float a = (float)((double)rp_acc[i] * (1.0 / 1099511627776.0));
            const float s = run[i] + (tc > 0 ? a / (float)tc : 0.f);   // (a region without a valid point at this level adds 0)
            run[i] = s;
            wl[i] = s / (float)L;
        }
        __syncthreads();
    }
}

// grid (C / 64, n), 256 threads: thread (pg = tid / 8, ck = tid % 8) adds pixels pg, pg + 32, ... of the 16-byte channel chunk ck of the
// block's 64 channels; the 32 pixel groups meet in LDS and are added in group order.
__global__ __launch_bounds__(256) void region_pool_kernel(RegionPoolArgs a)
{
    __shared__ float red[32][64];
    const int tid = threadIdx.x, ck = tid & 7, pg = tid >> 3;
    const long n = blockIdx.y;
    const int c0 = blockIdx.x * 64 + ck * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int pix = pg; pix < a.HW; pix += 32) {
#pragma unroll
        for (int m = 0; m < REGION_MAX_MAPS; ++m) {
            if (m < a.maps) {
                const float wv = a.w[m][n * a.HW + pix];
                const uint4_t q = *reinterpret_cast<const uint4_t *>(a.x[m] + n * a.img_stride[m] + (long)pix * a.row_stride[m] + c0);
                float v[8];
                unpack8(q, v);
                // (a non-finite value at a pixel no valid point touches must not get through its zero weight)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += wv != 0.f ? wv * v[e] : 0.f;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pg][ck * 8 + e] = acc[e];
    __syncthreads();
    if (tid < 64) {
        float s = 0.f;
#pragma unroll 8
        for (int g = 0; g < 32; ++g) s += red[g][tid];
        a.out[n * a.C + blockIdx.x * 64 + tid] = f32_to_bf16(s);
    }
}

// one thread per (n, pix, 8-channel chunk): a 16-byte store
__global__ __launch_bounds__(256) void region_outer_kernel(const float *__restrict__ w, const uint16_t *__restrict__ g, uint16_t *__restrict__ out,
                                                           long n, int HW, int C)
{
    const int cch = C / 8;
    const long items = n * HW * cch;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % cch);
        const long np = i / cch;            // n * HW + pix
        const long in = np / HW;
        const float wv = w[np];
        float v[8];
        unpack8(*reinterpret_cast<const uint4_t *>(g + in * C + ch * 8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = wv != 0.f ? wv * v[e] : 0.f;   // (a zero weight stays zero whatever g holds)
        const uint4_t o = pack8(v);
        *reinterpret_cast<uint4_t *>(out + np * C + ch * 8) = o;
    }
}

inline int ln_gelu_group(int C)
{
    if (C <= 0 || C % 64 != 0) return 0;
    const int chunks = C / 8;
    for (int g = 64; g >= 8; g >>= 1)
        if (chunks % g == 0 && chunks / g <= LG_NCH) return g;
    return 0;
}

}  // namespace

int region_im2col_launch(const void *images, const void *masks, int is_f32, uint16_t *A, int n, int H, int W, int k, int Kpad, hipStream_t st)
{
    VLLM_REQUIRE(n >= 0 && k > 0 && H > 0 && W > 0 && H % (2 * k) == 0 && W % (2 * k) == 0, "region_im2col: H=%d, W=%d must be multiples of 2 k = %d", H, W, 2 * k);
    VLLM_REQUIRE(Kpad % 64 == 0 && Kpad >= 4 * k * k && Kpad < 4 * k * k + 64, "region_im2col: Kpad=%d is not 4 k^2 = %d rounded up to 64", Kpad, 4 * k * k);
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(images && masks && A && aligned16(A), "region_im2col: null pointer, or A not 16-byte aligned");
    VLLM_REQUIRE(((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(masks)) & (is_f32 ? 3u : 1u)) == 0, "region_im2col: pixels not element aligned");
    const long rows = (long)n * (H / k) * (W / k);
    VLLM_REQUIRE(rows < (1L << 31) / 4, "region_im2col: %ld rows (too many)", rows);
    const long items = rows * (Kpad / 8);
    if (is_f32)
        VLLM_LAUNCH((region_im2col_kernel<float>), dim3(grid_for(items)), dim3(256), 0, st, (const float *)images, (const float *)masks, A, n, H, W, k, Kpad);
    else
        VLLM_LAUNCH((region_im2col_kernel<uint16_t>), dim3(grid_for(items)), dim3(256), 0, st, (const uint16_t *)images, (const uint16_t *)masks, A, n, H, W, k, Kpad);
    VLLM_CHECK_LAUNCH("region_im2col_kernel");
    return VLLM_OK;
}

bool ln_gelu_takes(int C) { return ln_gelu_group(C) != 0; }

int ln_gelu_launch(const uint16_t *x, int ldx, const uint16_t *w, const uint16_t *b, uint16_t *pre, uint16_t *y, long rows, int C, float eps,
                   hipStream_t st)
{
    const int G = ln_gelu_group(C);
    VLLM_REQUIRE(G != 0, "layernorm_gelu: C=%d must be a multiple of 64 whose 16-byte chunks split over 8, 16, 32 or 64 lanes, at most 8 each (64 .. 512 in steps of 64; 4096 at most)", C);
    VLLM_REQUIRE(rows >= 0 && rows < (1L << 31) && ldx >= C && ldx % 8 == 0, "layernorm_gelu: rows=%ld, ldx=%d (a multiple of 8, >= C)", rows, ldx);
    if (rows == 0) return VLLM_OK;
    VLLM_REQUIRE(x && w && b && y && aligned16(x) && aligned16(w) && aligned16(b) && aligned16(y) && aligned16(pre),
                 "layernorm_gelu: x, weight, bias, y (and pre_out) must be 16-byte aligned device pointers");
    const int R = 64 / G;
    const dim3 grid((unsigned)ceil_div(rows, 4L * R));
#define LG_GO(g) VLLM_LAUNCH((ln_gelu_kernel<g>), grid, dim3(256), 0, st, x, ldx, w, b, pre, y, rows, C, eps)
    if (G == 8) LG_GO(8); else if (G == 16) LG_GO(16); else if (G == 32) LG_GO(32); else LG_GO(64);
#undef LG_GO
    VLLM_CHECK_LAUNCH("ln_gelu_kernel");
    return VLLM_OK;
}

int region_wperm_launch(const uint16_t *src, uint16_t *dst, int R, int K, int inverse, hipStream_t st)
{
    VLLM_REQUIRE(src && dst && R > 0 && K > 0 && K % 4 == 0, "region_wperm: bad arguments");
    VLLM_LAUNCH(region_wperm_kernel, dim3(grid_for((long)R * K)), dim3(256), 0, st, src, dst, R, K, inverse);
    VLLM_CHECK_LAUNCH("region_wperm_kernel");
    return VLLM_OK;
}

bool region_pool_weights_fit(long HW) { return (size_t)((HW + 1) & ~1L) * 8 + (size_t)HW * 4 <= (size_t)PS_LDS_MAX; }

int region_pool_weights_launch(const float *coords, const uint8_t *valid, float *w, int n, int L, int H, int W, int P, hipStream_t st)
{
    VLLM_REQUIRE(n >= 0 && L >= 1 && L <= REGION_MAX_LEVELS && H > 0 && W > 0 && P >= 0, "region_pool_weights: bad sizes");
    VLLM_REQUIRE(region_pool_weights_fit((long)H * W), "region_pool_weights: a map of %d x %d does not fit the LDS accumulators (at most 4096 positions)", H, W);
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(w && aligned16(w) && (P == 0 || (coords && valid)), "region_pool_weights: null pointer, or weights not 16-byte aligned");
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(coords) & 7u) == 0, "region_pool_weights: points must be 8-byte aligned");
    const long HW = (long)H * W;
    const size_t lds = (size_t)((HW + 1) & ~1L) * 8 + (size_t)HW * 4;
    VLLM_LAUNCH(region_pool_weights_kernel, dim3((unsigned)n), dim3(RPW_THREADS), lds, st, coords, valid, w, n, L, H, W, P);
    VLLM_CHECK_LAUNCH("region_pool_weights_kernel");
    return VLLM_OK;
}

int region_pool_launch(const RegionPoolArgs &a, int n, hipStream_t st)
{
    VLLM_REQUIRE(a.maps >= 1 && a.maps <= REGION_MAX_MAPS && a.C > 0 && a.C % 64 == 0 && a.HW > 0 && n >= 0 && n <= 65535, "region_pool: bad sizes");
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(a.out, "region_pool: null output");
    for (int m = 0; m < a.maps; ++m)
        VLLM_REQUIRE(a.x[m] && a.w[m] && aligned16(a.x[m]) && a.row_stride[m] % 8 == 0 && a.img_stride[m] % 8 == 0 && a.row_stride[m] >= a.C,
                     "region_pool: map %d must be 16-byte aligned with row and image strides that are multiples of 8 elements", m);
    VLLM_LAUNCH(region_pool_kernel, dim3((unsigned)(a.C / 64), (unsigned)n), dim3(256), 0, st, a);
    VLLM_CHECK_LAUNCH("region_pool_kernel");
    return VLLM_OK;
}

int region_outer_launch(const float *w, const uint16_t *g, uint16_t *out, int n, int HW, int C, hipStream_t st)
{
    VLLM_REQUIRE(n >= 0 && HW > 0 && C > 0 && C % 8 == 0, "region_outer: bad sizes");
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(w && g && out && aligned16(g) && aligned16(out), "region_outer: null pointer, or g / out not 16-byte aligned");
    VLLM_LAUNCH(region_outer_kernel, dim3(grid_for((long)n * HW * (C / 8))), dim3(256), 0, st, w, g, out, (long)n, HW, C);
    VLLM_CHECK_LAUNCH("region_outer_kernel");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_layernorm_gelu_bf16(const uint16_t *x, int ldx, const uint16_t *weight, const uint16_t *bias, uint16_t *pre_out, uint16_t *y,
                                        long rows, int C, float eps, vllm_stream_t stream)
{
    return ln_gelu_launch(x, ldx, weight, bias, pre_out, y, rows, C, eps, (hipStream_t)stream);
}

extern "C" int vllm_region_im2col_bf16(const void *images, const void *masks, int pixel_is_f32, uint16_t *A, int n, int H, int W, int patch,
                                       int Kpad, vllm_stream_t stream)
{
    VLLM_REQUIRE(patch > 0 && patch % 2 == 0, "vllm_region_im2col_bf16: patch=%d must be even", patch);
    VLLM_REQUIRE(pixel_is_f32 == 0 || pixel_is_f32 == 1, "vllm_region_im2col_bf16: pixel_is_f32 %d", pixel_is_f32);
    return region_im2col_launch(images, masks, pixel_is_f32, A, n, H, W, patch / 2, Kpad, (hipStream_t)stream);
}

extern "C" int vllm_region_pool_weights_f32(const float *points, const uint8_t *valid, float *weights, int n, int levels, int h, int w, int P,
                                            vllm_stream_t stream)
{
    return region_pool_weights_launch(points, valid, weights, n, levels, h, w, P, (hipStream_t)stream);
}

extern "C" int vllm_region_pool_bf16(const float *weights, const uint16_t *stem, const uint16_t *const *levels, const long *level_row_stride,
                                     const long *level_image_stride, int n, int n_levels, int hw, int C, uint16_t *pooled, vllm_stream_t stream)
{
    VLLM_REQUIRE(n_levels >= 1 && n_levels <= REGION_MAX_LEVELS && weights && stem && levels && level_row_stride && level_image_stride && hw > 0 && n >= 0,
                 "vllm_region_pool_bf16: bad arguments (1 .. 4 levels)");
    RegionPoolArgs a;
    a.maps = n_levels + 1; a.HW = hw; a.C = C; a.out = pooled;
    a.x[0] = stem; a.w[0] = weights; a.row_stride[0] = C; a.img_stride[0] = (long)hw * C;
    for (int l = 0; l < n_levels; ++l) {
        a.x[l + 1] = levels[l]; a.w[l + 1] = weights + (long)l * n * hw;
        a.row_stride[l + 1] = level_row_stride[l]; a.img_stride[l + 1] = level_image_stride[l];
    }
    return region_pool_launch(a, n, (hipStream_t)stream);
}

extern "C" int vllm_region_outer_bf16(const float *weights, const uint16_t *g, uint16_t *grad_map, int n, int hw, int C, vllm_stream_t stream)
{
    return region_outer_launch(weights, g, grad_map, n, hw, C, (hipStream_t)stream);
}
