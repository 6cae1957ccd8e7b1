// The DCNv3 LAYER around the sampling operator for bf16 modules at inference:
//   input_proj -> depth-wise conv + LayerNorm + GELU -> offset / mask / centre-feature-scale linears -> softmax over the 9 logits ->
//   operator -> centre-feature blend -> output_proj.
// Reference: DCNv3.forward  visionllmv2/model/ops_dcnv3/modules/dcnv3.py:313-351, CenterFeatureScaleModule :206-219.
//
// Five launches (include/vllm_hip.h, section f3b): three bf16 MFMA GEMMs and the two kernels of this file between them.
//   dwconv_ln_gelu_kernel       x1 = GELU(LayerNorm(dwconv(input))), channels-last, one read of the input rows (through L2) and one write
//   dcnv3_sample_fused_kernel   softmax + the gather of dcnv3.hip on a bf16 value + the centre-feature blend, bf16 result
// Offsets, logits and centre logits are the fp32 rows of ONE GEMM over x1 (EPI_F32), so the sampling geometry never passes through bf16.
#include "common.hpp"
#include "orchestrate.hpp"
#include "gemm_epilogue.hpp"
#include "dcnv3_geo.hpp"

namespace vllm {
namespace {

__device__ __forceinline__ void widen8(const uint4_t v, float *f)
{
    f[0] = bf16lo_to_f32(v.x); f[1] = bf16hi_to_f32(v.x); f[2] = bf16lo_to_f32(v.y); f[3] = bf16hi_to_f32(v.y);
    f[4] = bf16lo_to_f32(v.z); f[5] = bf16hi_to_f32(v.z); f[6] = bf16lo_to_f32(v.w); f[7] = bf16hi_to_f32(v.w);
}
__device__ __forceinline__ uint4_t narrow8(const float *f)
{
    uint4_t o;
    o.x = pack_bf16x2(f[0], f[1]); o.y = pack_bf16x2(f[2], f[3]); o.z = pack_bf16x2(f[4], f[5]); o.w = pack_bf16x2(f[6], f[7]);
    return o;
}

// ---- depth-wise conv + LayerNorm + GELU ------------------------------------------------------------------------------------------
// A block owns a strip of DW_TW consecutive pixels of one image row; thread c (< C / 8) owns channels 8c .. 8c+7 of every pixel of the
// strip, so a tap is one 16-byte load and the DW_TW + dwk - 1 input columns of a tap row are loaded once for the whole strip (the
// horizontal re-reads stay in registers).  The dwk tap rows are re-read by the blocks of the neighbouring image rows: those blocks are
// neighbours in the grid as well (the strip index runs fastest, then the row), so the re-reads are served by L2 -- a row of the
// largest stage (168 x 640 bf16) is 210 KiB, dwk of them sit in every XCD's 4 MiB many times over.  The 8 x dwk weights of a tap row
// are widened once per row and used for the DW_TW pixels.  LayerNorm: per pixel, DPP sum inside a wave, LDS across the block's waves,
// mean first, then the squared deviations from the accumulators themselves.
constexpr int DW_TW = 8;
constexpr int DW_MAX_THREADS = 512;   // C <= 4096; ~200 VGPRs per lane: two waves per SIMD at most, which 512 threads need

template <int DWK>
__global__ __launch_bounds__(DW_MAX_THREADS) void dwconv_ln_gelu_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ dw_w,
                                                                        const uint16_t *__restrict__ dw_b, const uint16_t *__restrict__ ln_w,
                                                                        const uint16_t *__restrict__ ln_b, uint16_t *__restrict__ out,
                                                                        int H, int W, int C, int strips, float eps)
{
    constexpr int R = DWK / 2, KK = DWK * DWK;
    __shared__ float red[DW_MAX_THREADS / 64][DW_TW];
    const int L = C >> 3, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const bool live = tid < L;
    const int c = live ? tid : L - 1;   // idle lanes of the last wave repeat the last chunk's loads and store nothing
    const int strip = blockIdx.x % strips;
    const long t = blockIdx.x / strips;
    const int h = (int)(t % H);
    const long n = t / H;
    const int w0 = strip * DW_TW;
    const uint16_t *img = x + n * H * (long)W * C + c * 8;
    const uint16_t *wp = dw_w + (long)c * 8 * KK;

    float acc[DW_TW][8];
#pragma unroll
    for (int p = 0; p < DW_TW; ++p)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[p][i] = 0.f;

#pragma unroll 1
    for (int dy = 0; dy < DWK; ++dy) {
        const int yy = h + dy - R;
        const bool rowok = yy >= 0 && yy < H;
        const uint16_t *rowp = img + (long)min(max(yy, 0), H - 1) * W * C;
        float wt[DWK][8];
#pragma unroll
        for (int dx = 0; dx < DWK; ++dx)
#pragma unroll
            for (int i = 0; i < 8; ++i) wt[dx][i] = bf16_to_f32(wp[i * KK + dy * DWK + dx]);
#pragma unroll
        for (int j = 0; j < DW_TW + DWK - 1; ++j) {
            const int xx = w0 + j - R;
            const bool ok = rowok && xx >= 0 && xx < W;
            // a tap outside the image: the load goes to a clamped (valid) address and the select drops what it returns
            const uint4_t v = *reinterpret_cast<const uint4_t *>(rowp + (long)min(max(xx, 0), W - 1) * C);
            float f[8];
            widen8(v, f);
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = ok ? f[i] : 0.f;
#pragma unroll
            for (int dx = 0; dx < DWK; ++dx) {
                const int p = j - dx;
                if (p >= 0 && p < DW_TW) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[p][i] = fmaf(wt[dx][i], f[i], acc[p][i]);
                }
            }
        }
    }
    {
        float b[8];
        widen8(*reinterpret_cast<const uint4_t *>(dw_b + c * 8), b);
#pragma unroll
        for (int p = 0; p < DW_TW; ++p)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[p][i] += b[i];
    }

    // LayerNorm over the C channels of each pixel: mean, then the sum of squared deviations
    const float inv_c = 1.f / (float)C;
    float mean[DW_TW], rstd[DW_TW];
#pragma unroll
    for (int p = 0; p < DW_TW; ++p) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += acc[p][i];
        mean[p] = wave_sum(live ? s : 0.f);
    }
    if (nw > 1) {
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < DW_TW; ++p) red[wave][p] = mean[p];
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < DW_TW; ++p) {
            float s = 0.f;
            for (int k = 0; k < nw; ++k) s += red[k][p];
            mean[p] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < DW_TW; ++p) {
        mean[p] *= inv_c;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = acc[p][i] - mean[p]; q = fmaf(d, d, q); }
        rstd[p] = wave_sum(live ? q : 0.f);
    }
    if (nw > 1) {
        if (lane == 0) {
#pragma unroll
            for (int p = 0; p < DW_TW; ++p) red[wave][p] = rstd[p];
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < DW_TW; ++p) {
            float s = 0.f;
            for (int k = 0; k < nw; ++k) s += red[k][p];
            rstd[p] = s;
        }
    }
    if (!live) return;
    float g[8], b[8];
    widen8(*reinterpret_cast<const uint4_t *>(ln_w + c * 8), g);
    widen8(*reinterpret_cast<const uint4_t *>(ln_b + c * 8), b);
    uint16_t *op = out + ((n * H + h) * (long)W + w0) * C + c * 8;
#pragma unroll
    for (int p = 0; p < DW_TW; ++p) {
        if (w0 + p < W) {
            const float r = rsqrtf(rstd[p] * inv_c + eps);
            float y[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = gelu_erf(fmaf((acc[p][i] - mean[p]) * r, g[i], b[i]));
            *reinterpret_cast<uint4_t *>(op + (long)p * C) = narrow8(y);
        }
    }
}

int dwconv_launch(const uint16_t *x, const uint16_t *dw_w, const uint16_t *dw_b, const uint16_t *ln_w, const uint16_t *ln_b, int N, int H,
                  int W, int C, int dwk, float eps, uint16_t *out, hipStream_t st)
{
    const int strips = ceil_div(W, DW_TW);
    const long blocks = (long)N * H * strips;
    VLLM_REQUIRE(blocks < (1L << 31), "dwconv_ln_gelu: too many pixel strips for one launch");
    const dim3 grid((unsigned)blocks), block((unsigned)(((C >> 3) + 63) & ~63));
#define GO(K) VLLM_LAUNCH(dwconv_ln_gelu_kernel<K>, grid, block, 0, st, x, dw_w, dw_b, ln_w, ln_b, out, H, W, C, strips, eps)
    if (dwk == 1) GO(1);
    else if (dwk == 3) GO(3);
    else if (dwk == 5) GO(5);
    else GO(7);
#undef GO
    VLLM_CHECK_LAUNCH("dwconv_ln_gelu_kernel");
    return VLLM_OK;
}

// ---- softmax + sampling + centre-feature blend -------------------------------------------------------------------------------------
// dcnv3_fwd_kernel's structure (dcnv3.hip): a lane owns 8 channels of one (pixel, group), the CPL = D / 8 lanes of a group sit next to
// each other, the 3 x 3 loop is unrolled (36 independent 16-byte corner loads from clamped addresses, selects decide what counts).  The
// value is the bf16 x_proj; the group's 18 offsets, 9 logits and centre logit are broadcast loads from the pixel's fp32 GEMM row.
template <int CPL, bool CFS>
__global__ __launch_bounds__(256) void dcnv3_sample_fused_kernel(const uint16_t *__restrict__ xp, const float *__restrict__ om, long ld_om,
                                                                 uint16_t *__restrict__ out, long total, int H, int W, int G, int dil,
                                                                 float offset_scale)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cc = (int)(idx % CPL);
    const long sidx = idx / CPL;                      // row * G + g
    const int g = (int)(sidx % G);
    const long row = sidx / G;                        // (b * H + y) * W + x
    const int x = (int)(row % W);
    const long t = row / W;
    const int y = (int)(t % H);
    const long b = t / H;
    const long ws = (long)G * CPL * 8, hs = (long)W * ws;
    const uint16_t *im = xp + b * H * hs + ((long)g * CPL + cc) * 8;
    const float *orow = om + row * ld_om;
    const float *op = orow + g * 18, *lp = orow + G * 18 + g * 9;

    float e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = lp[k];
    float mx = e[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, e[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) { e[k] = __expf(e[k] - mx); sum += e[k]; }
    const float inv = 1.f / sum;

    // stride 1, pad == dilation, 3 x 3: p0 = (dil * 2 >> 1) - pad + x = x (dcnv3_im2col_cuda.cuh:236-241)
    const float p0_w_ = (float)x - dcn_mul_rn<float>((float)dil, offset_scale);
    const float p0_h_ = (float)y - dcn_mul_rn<float>((float)dil, offset_scale);
    float acc[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) acc[v] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)         // kernel_w outer
#pragma unroll
        for (int j = 0; j < 3; ++j) {   // kernel_h inner
            const int k = i * 3 + j;
            const float2_t o2 = *reinterpret_cast<const float2_t *>(op + 2 * k);   // (x, y): 8-byte aligned, rows are 16-byte aligned
            const float off_w = o2[0], off_h = o2[1], wgt = e[k] * inv;
            const float loc_w = dcn_loc<float>(p0_w_, (float)(i * dil), off_w, offset_scale);
            const float loc_h = dcn_loc<float>(p0_h_, (float)(j * dil), off_h, offset_scale);
            const bool ok = loc_h > -1.f && loc_w > -1.f && loc_h < (float)H && loc_w < (float)W;
            // a rejected location (possibly NaN / inf) never reaches the address arithmetic
            const int h_low = ok ? (int)floorf(loc_h) : 0, w_low = ok ? (int)floorf(loc_w) : 0;
            const float lh = loc_h - (float)h_low, lw = loc_w - (float)w_low, hh = 1.f - lh, hw = 1.f - lw;
            const bool u0 = ok && h_low >= 0, u1 = ok && h_low + 1 <= H - 1, l0 = w_low >= 0, l1 = w_low + 1 <= W - 1;
            const int y0 = min(max(h_low, 0), H - 1), y1 = min(max(h_low + 1, 0), H - 1);
            const int x0 = min(max(w_low, 0), W - 1), x1 = min(max(w_low + 1, 0), W - 1);
            const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
            // the predicates act on the packed words (a NaN at a clamped address is dropped before it is widened) and on the four weights
            // (a rejected point's may be NaN: its location is), so that a value costs one widening and four FMAs
            const uint4_t z = {0u, 0u, 0u, 0u};
            uint4_t q1 = *reinterpret_cast<const uint4_t *>(im + y0 * hs + x0 * ws), q2 = *reinterpret_cast<const uint4_t *>(im + y0 * hs + x1 * ws);
            uint4_t q3 = *reinterpret_cast<const uint4_t *>(im + y1 * hs + x0 * ws), q4 = *reinterpret_cast<const uint4_t *>(im + y1 * hs + x1 * ws);
            q1 = (u0 && l0) ? q1 : z; q2 = (u0 && l1) ? q2 : z; q3 = (u1 && l0) ? q3 : z; q4 = (u1 && l1) ? q4 : z;
            const float a1 = ok ? w1 * wgt : 0.f, a2 = ok ? w2 * wgt : 0.f, a3 = ok ? w3 * wgt : 0.f, a4 = ok ? w4 * wgt : 0.f;
            float v1[8], v2[8], v3[8], v4[8];
            widen8(q1, v1); widen8(q2, v2); widen8(q3, v3); widen8(q4, v4);
#pragma unroll
            for (int v = 0; v < 8; ++v) acc[v] = fmaf(a4, v4[v], fmaf(a3, v3[v], fmaf(a2, v2[v], fmaf(a1, v1[v], acc[v]))));
        }
    if (CFS) {
        const float s = 1.f / (1.f + __expf(-orow[G * 27 + g]));
        float c[8];
        widen8(*reinterpret_cast<const uint4_t *>(im + y * hs + x * ws), c);
#pragma unroll
        for (int v = 0; v < 8; ++v) acc[v] = acc[v] * (1.f - s) + c[v] * s;
    }
    *reinterpret_cast<uint4_t *>(out + row * ws + ((long)g * CPL + cc) * 8) = narrow8(acc);
}

int sample_launch(const uint16_t *xp, const float *om, int ld_om, long R, int H, int W, int G, int D, int dil, float offset_scale, int cfs,
                  uint16_t *out, hipStream_t st)
{
    const long total = R * G * (D / 8), blocks = (total + 255) / 256;
    VLLM_REQUIRE(blocks < (1L << 31), "dcnv3_sample_fused: too many lanes for one launch");
    const dim3 grid((unsigned)blocks), block(256);
#define GO(CPL)                                                                                                                     \
    do {                                                                                                                            \
        if (cfs) VLLM_LAUNCH((dcnv3_sample_fused_kernel<CPL, true>), grid, block, 0, st, xp, om, (long)ld_om, out, total, H, W, G, dil, \
                             offset_scale);                                                                                         \
        else VLLM_LAUNCH((dcnv3_sample_fused_kernel<CPL, false>), grid, block, 0, st, xp, om, (long)ld_om, out, total, H, W, G, dil,    \
                         offset_scale);                                                                                             \
    } while (0)
    if (D == 8) GO(1);
    else if (D == 16) GO(2);
    else if (D == 32) GO(4);
    else GO(8);
#undef GO
    VLLM_CHECK_LAUNCH("dcnv3_sample_fused_kernel");
    return VLLM_OK;
}

int check_desc(const VllmDcnv3LayerDesc *d)
{
    VLLM_REQUIRE(d, "dcnv3_layer: null descriptor");
    VLLM_REQUIRE(d->channels > 0 && d->group > 0 && d->channels % d->group == 0, "dcnv3_layer: channels=%d must be divisible by group=%d",
                 d->channels, d->group);
    VLLM_REQUIRE(d->channels % 64 == 0, "dcnv3_layer: channels=%d must be a multiple of 64 (GEMM K tile)", d->channels);
    const int D = d->channels / d->group;
    VLLM_REQUIRE(D == 8 || D == 16 || D == 32 || D == 64, "dcnv3_layer: group channels=%d must be 8, 16, 32 or 64", D);
    VLLM_REQUIRE(d->channels <= DW_MAX_THREADS * 8, "dcnv3_layer: channels=%d above %d", d->channels, DW_MAX_THREADS * 8);
    VLLM_REQUIRE(d->kernel_size == 3, "dcnv3_layer: kernel_size=%d must be 3", d->kernel_size);
    VLLM_REQUIRE(d->dw_kernel_size >= 1 && d->dw_kernel_size <= 7 && d->dw_kernel_size % 2 == 1,
                 "dcnv3_layer: dw_kernel_size=%d must be odd, 1 .. 7", d->dw_kernel_size);
    VLLM_REQUIRE(d->dilation >= 1, "dcnv3_layer: dilation=%d must be >= 1", d->dilation);
    VLLM_REQUIRE(d->center_feature_scale == 0 || d->center_feature_scale == 1, "dcnv3_layer: center_feature_scale must be 0 or 1");
    const int used = (d->center_feature_scale ? 28 : 27) * d->group;
    VLLM_REQUIRE(d->n_proj % 8 == 0 && d->n_proj >= used, "dcnv3_layer: n_proj=%d must be a multiple of 8 and at least %d", d->n_proj, used);
    VLLM_REQUIRE(d->ln_eps >= 0.f && d->offset_scale == d->offset_scale, "dcnv3_layer: bad ln_eps / offset_scale");
    return VLLM_OK;
}

struct Dcnv3LayerWs {
    long x_proj, x1, om, total;
};
Dcnv3LayerWs layer_ws(const VllmDcnv3LayerDesc *d, long R)
{
    Dcnv3LayerWs w;
    Carver cv;
    w.x_proj = cv.take(R * d->channels * 2);
    w.x1 = cv.take(R * d->channels * 2);   // x1, and behind the projection GEMM the blended core (output_proj's operand)
    w.om = cv.take(R * d->n_proj * 4);
    w.total = cv.off;
    return w;
}

long g_layer_calls = 0;

}  // namespace
}  // namespace vllm

using namespace vllm;

extern "C" unsigned long vllm_dcnv3_layer_desc_sizeof(void) { return sizeof(VllmDcnv3LayerDesc); }
extern "C" long vllm_dcnv3_layer_calls(void) { return __atomic_load_n(&g_layer_calls, __ATOMIC_RELAXED); }

extern "C" long vllm_dcnv3_layer_workspace_bytes(const VllmDcnv3LayerDesc *d, int N, int H, int W)
{
    if (check_desc(d) != VLLM_OK) return -1;
    if (N < 0 || H < 0 || W < 0 || (long)N * H * W >= (1L << 31)) { set_error("dcnv3_layer: N, H, W must be >= 0 and N H W < 2^31"); return -1; }
    return layer_ws(d, (long)N * H * W).total;
}

extern "C" int vllm_dwconv_ln_gelu_bf16(const uint16_t *x, const uint16_t *dw_w, const uint16_t *dw_b, const uint16_t *ln_w,
                                        const uint16_t *ln_b, int N, int H, int W, int C, int dwk, float eps, uint16_t *out,
                                        vllm_stream_t stream)
{
    VLLM_REQUIRE(N >= 0 && H >= 0 && W >= 0 && (long)N * H * W < (1L << 31), "dwconv_ln_gelu: N, H, W must be >= 0 and N H W < 2^31");
    VLLM_REQUIRE(C > 0 && C % 8 == 0 && C <= DW_MAX_THREADS * 8, "dwconv_ln_gelu: C=%d must be a multiple of 8, at most %d", C, DW_MAX_THREADS * 8);
    VLLM_REQUIRE(dwk >= 1 && dwk <= 7 && dwk % 2 == 1, "dwconv_ln_gelu: dwk=%d must be odd, 1 .. 7", dwk);
    if ((long)N * H * W == 0) return VLLM_OK;
    VLLM_REQUIRE(x && dw_w && dw_b && ln_w && ln_b && out, "dwconv_ln_gelu: null pointer");
    VLLM_REQUIRE(aligned16(x) && aligned16(dw_w) && aligned16(dw_b) && aligned16(ln_w) && aligned16(ln_b) && aligned16(out),
                 "dwconv_ln_gelu: misaligned pointer (16 bytes)");
    return dwconv_launch(x, dw_w, dw_b, ln_w, ln_b, N, H, W, C, dwk, eps, out, (hipStream_t)stream);
}

extern "C" int vllm_dcnv3_sample_fused_bf16(const uint16_t *x_proj, const float *om, int ld_om, int N, int H, int W, int G, int D,
                                            int dilation, float offset_scale, int center_feature_scale, uint16_t *out, vllm_stream_t stream)
{
    VLLM_REQUIRE(N >= 0 && H >= 0 && W >= 0 && (long)N * H * W < (1L << 31), "dcnv3_sample_fused: N, H, W must be >= 0 and N H W < 2^31");
    VLLM_REQUIRE(G > 0 && G <= (1 << 20) && (D == 8 || D == 16 || D == 32 || D == 64), "dcnv3_sample_fused: G=%d, D=%d (D must be 8, 16, 32 or 64)", G, D);
    VLLM_REQUIRE(dilation >= 1 && (center_feature_scale == 0 || center_feature_scale == 1), "dcnv3_sample_fused: bad dilation / flag");
    VLLM_REQUIRE(ld_om % 4 == 0 && ld_om >= (center_feature_scale ? 28 : 27) * G, "dcnv3_sample_fused: ld_om=%d must be a multiple of 4 and >= %d",
                 ld_om, (center_feature_scale ? 28 : 27) * G);
    if ((long)N * H * W == 0) return VLLM_OK;
    VLLM_REQUIRE(x_proj && om && out, "dcnv3_sample_fused: null pointer");
    VLLM_REQUIRE(aligned16(x_proj) && aligned16(om) && aligned16(out), "dcnv3_sample_fused: misaligned pointer (16 bytes)");
    return sample_launch(x_proj, om, ld_om, (long)N * H * W, H, W, G, D, dilation, offset_scale, center_feature_scale, out, (hipStream_t)stream);
}

extern "C" int vllm_dcnv3_layer_forward(const VllmDcnv3LayerDesc *d, const uint16_t *input, int N, int H, int W, uint16_t *out,
                                        void *workspace, long ws_bytes, vllm_stream_t stream)
{
    TRY(check_desc(d));
    VLLM_REQUIRE(N >= 0 && H >= 0 && W >= 0, "dcnv3_layer: negative size");
    VLLM_REQUIRE((long)N * H * W < (1L << 31), "dcnv3_layer: N H W = %ld must be below 2^31", (long)N * H * W);
    const long R = (long)N * H * W;
    if (R == 0) return VLLM_OK;
    VLLM_REQUIRE(input && out, "dcnv3_layer: null pointer (input / out)");
    VLLM_REQUIRE(d->input_proj_w && d->input_proj_b && d->dw_w && d->dw_b && d->ln_w && d->ln_b && d->proj_w && d->proj_b &&
                 d->output_proj_w && d->output_proj_b, "dcnv3_layer: null pointer in the descriptor (missing weights)");
    VLLM_REQUIRE(aligned16(input) && aligned16(out), "dcnv3_layer: misaligned input / out (16 bytes)");
    VLLM_REQUIRE(aligned16(d->input_proj_w) && aligned16(d->input_proj_b) && aligned16(d->dw_w) && aligned16(d->dw_b) && aligned16(d->ln_w) &&
                 aligned16(d->ln_b) && aligned16(d->proj_w) && aligned16(d->proj_b) && aligned16(d->output_proj_w) && aligned16(d->output_proj_b),
                 "dcnv3_layer: misaligned weight or bias in the descriptor (16 bytes)");
    const Dcnv3LayerWs w = layer_ws(d, R);
    VLLM_REQUIRE(workspace && aligned16(workspace) && ws_bytes >= w.total, "dcnv3_layer: workspace too small (%ld < %ld bytes) or misaligned",
                 ws_bytes, w.total);
    VLLM_REQUIRE((long)H * (W / DW_TW + 1) * N < (1L << 31) && R * (d->channels / 8) / 256 + 1 < (1L << 31),
                 "dcnv3_layer: too many pixels for one launch of its kernels");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    uint16_t *x_proj = (uint16_t *)(ws + w.x_proj), *x1 = (uint16_t *)(ws + w.x1);
    float *om = (float *)(ws + w.om);
    const int C = d->channels, G = d->group, NP = d->n_proj;
    __atomic_fetch_add(&g_layer_calls, 1, __ATOMIC_RELAXED);
    // x_proj = input_proj(input)                                               (dcnv3.py:321-322)
    TRY(gemm(st, EPI_BIAS, input, C, d->input_proj_w, C, d->input_proj_b, x_proj, C, (int)R, C, C));
    // x1 = GELU(LayerNorm(dw_conv(input))), channels-last throughout            (:325-326)
    TRY(dwconv_launch(input, d->dw_w, d->dw_b, d->ln_w, d->ln_b, N, H, W, C, d->dw_kernel_size, d->ln_eps, x1, st));
    // offsets | logits | centre logits of every pixel, fp32                     (:327-329, :344-346)
    TRY(gemm(st, EPI_F32, x1, C, d->proj_w, C, d->proj_b, (uint16_t *)om, NP, (int)R, NP, C));
    // softmax, operator, centre-feature blend; the bf16 result takes x1's place  (:328-349)
    TRY(sample_launch(x_proj, om, NP, R, H, W, G, C / G, d->dilation, d->offset_scale, d->center_feature_scale, x1, st));
    // output_proj                                                              (:350)
    TRY(gemm(st, EPI_BIAS, x1, C, d->output_proj_w, C, d->output_proj_b, out, C, (int)R, C, C));
    return VLLM_OK;
}
