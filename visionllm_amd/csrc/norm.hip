// Row normalisations (bf16 in/out, fp32 statistics) for gfx950.  HBM-bound: 16-byte vector loads, one pass over
// memory (rows are cached in registers), wave-shuffle reductions, optional multi-wave rows for wide C.
//
// Replaces:
//   InternRMSNorm / apex FusedRMSNorm   VisionLLMv2/visionllmv2/model/internvit/modeling_intern_vit.py:33-58
//       y = weight * bf16( x * rsqrt(mean(x^2) + eps) )      (fp32 statistics, cast, THEN multiply: kept)
//   QK-RMSNorm over the flattened H*D    :131-134 (applied in place on the q / k column blocks of the qkv buffer)
//   nn.LayerNorm (CLIP pre_layrnorm / layer_norm1/2, vl_bridge LayerNorm)  transformers CLIPEncoderLayer;
//       visionllmv2/model/modeling_visionllmv2.py:166-167
#include <algorithm>
#include "common.hpp"
#include "kernels.hpp"

namespace vllm {

constexpr int NORM_THREADS = 256;
constexpr int NORM_MAX_CHUNKS = 8;  // upper bound of 16-byte chunks cached per lane (template MAXCH picks 1/2/4/8)

// (wave_sum: common.hpp)

// WPR = waves per row (1, 2 or 4).  A 256-thread block handles 4 / WPR rows.
template <bool RMS, int WPR, int MAXCH>
__global__ __launch_bounds__(NORM_THREADS) void norm_bf16_kernel(const uint16_t *__restrict__ x, int ldx,
                                                                 const uint16_t *__restrict__ w,
                                                                 const uint16_t *__restrict__ b, uint16_t *__restrict__ y,
                                                                 int ldy, long rows, int C, float eps,
                                                                 const uint16_t *__restrict__ w2, int G, NormGather ps)
{
    // G column groups of C elements per memory row (G = 2: the q and k blocks of a qkv row, weights w / w2): the kernel's
    // "rows" are (memory row, group) pairs
    __shared__ float red[4][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rows_per_block = 4 / WPR;
    const int rloc = wave / WPR, wsub = wave % WPR;
    const long row = (long)blockIdx.x * rows_per_block + rloc;
    const bool live = row < rows;
    const long rv = live ? row : rows - 1;
    const long r = G == 1 ? rv : rv / G;
    const int grp = G == 1 ? 0 : (int)(rv - r * G);
    if (grp) w = w2;
    const int nchunk = C >> 3;
    const uint16_t *xr = x + r * (long)ldx + (long)grp * C;
    // pixel-shuffled rows (ps.hw > 0; G == 1): chunk c of the row lives in token (2 i2 + a) * hw + 2 j2 + b of tile n, quad = c / cseg
    const int ps_h2 = ps.hw >> 1;
    const long ps_n = ps.hw ? r / ((long)ps_h2 * ps_h2) : 0;
    const int ps_ij = ps.hw ? (int)(r - ps_n * ps_h2 * ps_h2) : 0;
    const int ps_i2 = ps.hw ? ps_ij / ps_h2 : 0, ps_j2 = ps.hw ? ps_ij - ps_i2 * ps_h2 : 0;
    auto chunk_src = [&](int c) -> const uint16_t * {
        if (!ps.hw) return xr + c * 8;
        const int quad = (c >= ps.cseg) + (c >= 2 * ps.cseg) + (c >= 3 * ps.cseg);
        const long tok = ps.tok0 + (long)(2 * ps_i2 + (quad >> 1)) * ps.hw + (2 * ps_j2 + (quad & 1));
        return x + ps_n * ps.tile_stride + tok * (long)ldx + (c - quad * ps.cseg) * 8;
    };

    // (weight / bias are requested behind the statistics, in the store loop: asking for them together with the row -- they do not
    //  depend on the statistics -- measured 22.8 instead of 21.5 us per launch inside the ViT-L step, same box, round 3)
    uint4_t v[MAXCH];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = (i * WPR + wsub) * 64 + lane;
        if (c < nchunk) {
            v[i] = *reinterpret_cast<const uint4_t *>(chunk_src(c));
            const uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = bf16lo_to_f32(u[k]), bb = bf16hi_to_f32(u[k]);
                s += a + bb;
                ss += a * a + bb * bb;
            }
        }
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (WPR > 1) {
        if (lane == 0) { red[wave][0] = s; red[wave][1] = ss; }
        __syncthreads();
        s = 0.f; ss = 0.f;
#pragma unroll
        for (int k = 0; k < WPR; ++k) { s += red[rloc * WPR + k][0]; ss += red[rloc * WPR + k][1]; }
    }
    float mean = 0.f, rstd;
    if (RMS) {
        rstd = rsqrtf(ss / (float)C + eps);
    } else {
        mean = s / (float)C;
        // second moment about the mean from the cached registers (no cancellation): one more cheap pass
        float var = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c = (i * WPR + wsub) * 64 + lane;
            if (c < nchunk) {
                const uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float a = bf16lo_to_f32(u[k]) - mean, bb = bf16hi_to_f32(u[k]) - mean;
                    var += a * a + bb * bb;
                }
            }
        }
        var = wave_sum(var);
        if (WPR > 1) {
            __syncthreads();
            if (lane == 0) red[wave][0] = var;
            __syncthreads();
            var = 0.f;
#pragma unroll
            for (int k = 0; k < WPR; ++k) var += red[rloc * WPR + k][0];
        }
        rstd = rsqrtf(var / (float)C + eps);
    }
    if (!live) return;
    uint16_t *yr = y + r * (long)ldy + (long)grp * C;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = (i * WPR + wsub) * 64 + lane;
        if (c < nchunk) {
            const uint4_t wv = *reinterpret_cast<const uint4_t *>(w + c * 8);
            uint4_t bv = {0, 0, 0, 0};
            if (!RMS && b) bv = *reinterpret_cast<const uint4_t *>(b + c * 8);
            const uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            const uint32_t uw[4] = {wv.x, wv.y, wv.z, wv.w};
            const uint32_t ub[4] = {bv.x, bv.y, bv.z, bv.w};
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float a = bf16lo_to_f32(u[k]), bb = bf16hi_to_f32(u[k]);
                if (RMS) {
                    // reference order: normalise in fp32, cast to bf16, THEN multiply by the bf16 weight
                    a = bf16_to_f32(f32_to_bf16(a * rstd)) * bf16lo_to_f32(uw[k]);
                    bb = bf16_to_f32(f32_to_bf16(bb * rstd)) * bf16hi_to_f32(uw[k]);
                } else {
                    a = (a - mean) * rstd * bf16lo_to_f32(uw[k]) + bf16lo_to_f32(ub[k]);
                    bb = (bb - mean) * rstd * bf16hi_to_f32(uw[k]) + bf16hi_to_f32(ub[k]);
                }
                o[k] = pack_bf16x2(a, bb);
            }
            uint4_t ov; ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
            *reinterpret_cast<uint4_t *>(yr + c * 8) = ov;
        }
    }
}

int norm_bf16_launch(bool rms, const uint16_t *x, int ldx, const uint16_t *w, const uint16_t *b, uint16_t *y, int ldy,
                     long rows, int C, float eps, hipStream_t st, const uint16_t *w2, int G, const NormGather *psp)
{
    if (rows == 0) return VLLM_OK;
    NormGather ps = {0, 0, 0, 0};
    if (psp) {
        ps = *psp;
        VLLM_REQUIRE(G == 1 && ps.hw > 0 && ps.hw % 2 == 0 && ps.cseg > 0 && ps.cseg * 4 * 8 == C && rows % ((long)(ps.hw / 2) * (ps.hw / 2)) == 0,
                     "norm: pixel-shuffled rows need an even token grid, C = 4 segments, whole tiles");
    }
    VLLM_REQUIRE(x && w && y, "norm: null pointer");
    VLLM_REQUIRE(G == 1 || (G == 2 && w2 && aligned16(w2) && !b), "norm: column groups: G = 2 with a second weight and no bias");
    rows *= G;
    VLLM_REQUIRE(C > 0 && C % 8 == 0 && ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(w) &&
                     (!b || aligned16(b)),
                 "norm: C and row strides must be multiples of 8 elements and pointers 16-byte aligned (C=%d)", C);
    const int nchunk = C / 8;
    int wpr = 1;
    while (wpr < 4 && nchunk > 64 * NORM_MAX_CHUNKS * wpr) wpr <<= 1;
    VLLM_REQUIRE(nchunk <= 64 * NORM_MAX_CHUNKS * wpr, "norm: C=%d too wide (max %d)", C, 64 * NORM_MAX_CHUNKS * 4 * 8);
    // prefer <= 4 cached chunks per lane (58 VGPRs, full occupancy) by spreading wide rows over 2 or 4 waves
    while (wpr < 4 && nchunk > 64 * 4 * wpr) wpr <<= 1;
    const int per_lane = (nchunk + 64 * wpr - 1) / (64 * wpr);
    const int maxch = per_lane <= 1 ? 1 : per_lane <= 2 ? 2 : per_lane <= 4 ? 4 : 8;
    const int rpb = 4 / wpr;
    const dim3 grid((unsigned)((rows + rpb - 1) / rpb)), block(NORM_THREADS);
#define L3(R, W, M) VLLM_LAUNCH((norm_bf16_kernel<R, W, M>), grid, block, 0, st, x, ldx, w, b, y, ldy, rows, C, eps, w2, G, ps)
#define L2(R, W) do { if (maxch == 1) L3(R, W, 1); else if (maxch == 2) L3(R, W, 2); else if (maxch == 4) L3(R, W, 4); else L3(R, W, 8); } while (0)
    if (rms) { if (wpr == 1) L2(true, 1); else if (wpr == 2) L2(true, 2); else L2(true, 4); }
    else     { if (wpr == 1) L2(false, 1); else if (wpr == 2) L2(false, 2); else L2(false, 4); }
#undef L2
#undef L3
    VLLM_CHECK_LAUNCH("norm_bf16_kernel");
    return VLLM_OK;
}


// ---- backward of the row-wise pieces of an InternViT layer (layer_train.cpp) -----------------------------------------------
//   rms_bwd_kernel   InternRMSNorm backward (modeling_intern_vit.py:33-44 under autograd; q_norm / k_norm :131-134 with G = 2): per row
//                    the statistic is recomputed from x in fp32;  xhat = x r,  g = grad_y w,
//                    grad_x = r (g - xhat mean(g xhat)) [+ grad_res]  (one rounding),  grad_w = sum_rows grad_y xhat  (xhat NOT rounded).
//   ls_bwd_kernel    LayerScale + residual backward (out = res + y * ls, :206-208):  grad_y = bf16(grad_out ls),  grad_ls = sum_rows grad_out y.
// Both: a block walks ranges of rows; the 64 / 128 / 256 threads that share a row own its 16-byte chunks and keep their column sums in
// registers; the next row's loads are requested before the current row's reductions.  The fp32 partial sums of every row range go to
// the caller's workspace and colsum_reduce_kernel adds them in a fixed tree (ln_bwd_kernel's scheme: no atomics, run-to-run identical).
constexpr int RB_THREADS = 256;
constexpr int RB_MAX_C = 8192;   // 4 chunks of 8 columns per thread

// sum over the TPR threads that share a row, the same value in each of them: DPP tree inside the wave, then the row's waves in a
// fixed order.  `par` alternates between two LDS slots, so one barrier per sum is enough (a slot is rewritten two sums later, behind
// the barrier in between).  Every thread of the block must call it (TPR > 64: a block-wide barrier).
template <int TPR> __device__ __forceinline__ float rb_row_sum(float v, float (*red)[4], int par)
{
    v = wave_sum(v);
    if (TPR == 64) return v;
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[par][wave] = v;
    __syncthreads();
    if (TPR == 128) return red[par][wave & 2] + red[par][(wave & 2) + 1];
    return (red[par][0] + red[par][1]) + (red[par][2] + red[par][3]);
}

// TPR threads (64 / 128 / 256: whole waves) share a row and own its 16-byte chunks tl, tl + TPR, ...; a block works on 256 / TPR row
// ranges at once, each a "virtual block" vb with its own partial sums (narrow rows would otherwise leave most of the block idle).
template <int MAXCH, int TPR, bool DX>
__global__ __launch_bounds__(RB_THREADS) void rms_bwd_kernel(const uint16_t *__restrict__ x, int ldx, const uint16_t *gy, int ldgy,
                                                             const uint16_t *__restrict__ w, const uint16_t *__restrict__ w2, uint16_t *gx,
                                                             int ldgx, const uint16_t *__restrict__ gres, int ldgr, float *__restrict__ part,
                                                             long rows, int C, int rpb, int nbv, float eps)
{
    __shared__ float red[2][4];
    constexpr int RG = RB_THREADS / TPR;
    const int tl = threadIdx.x % TPR, grp = blockIdx.y, nchunk = C >> 3;
    const int vb = blockIdx.x * RG + threadIdx.x / TPR;
    if (grp) w = w2;
    const long coff = (long)grp * C;   // column group of this block (G = 2: the q / k block of a qkv row)
    float wf[MAXCH][8], acc[MAXCH][8];
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = i * TPR + tl;
        uint4_t wv = {0, 0, 0, 0};
        if (c < nchunk) wv = *reinterpret_cast<const uint4_t *>(w + c * 8);
        unpack8(wv, wf[i]);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[i][k] = 0.f;
    }
    const float invC = 1.f / (float)C;
    const long r0 = (long)vb * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;   // (vb >= nbv: an empty range)
    uint4_t nx[MAXCH], ng[MAXCH], nr[MAXCH];
    auto request = [&](long r) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c = i * TPR + tl;
            nx[i] = ng[i] = nr[i] = (uint4_t){0, 0, 0, 0};
            if (c < nchunk && r < r1) {
                nx[i] = *reinterpret_cast<const uint4_t *>(x + r * ldx + coff + c * 8);
                ng[i] = *reinterpret_cast<const uint4_t *>(gy + r * ldgy + coff + c * 8);
                if (DX && gres) nr[i] = *reinterpret_cast<const uint4_t *>(gres + r * ldgr + c * 8);
            }
        }
    };
    request(r0);
    int par = 0;
    for (int it = 0; it < rpb; ++it) {   // (the same trip count in every thread: the row sums are block-wide barriers)
        const long r = r0 + it;
        float xv[MAXCH][8], gv[MAXCH][8];
        uint4_t rv[MAXCH];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            unpack8(nx[i], xv[i]);
            unpack8(ng[i], gv[i]);
            rv[i] = nr[i];
#pragma unroll
            for (int k = 0; k < 8; ++k) ss = fmaf(xv[i][k], xv[i][k], ss);
        }
        request(r + 1);   // (another row than the one stored below: grad_x may alias grad_y)
        const float rstd = rsqrtf(rb_row_sum<TPR>(ss, red, par) * invC + eps);
        par ^= 1;
        float sgx = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float xh = xv[i][k] * rstd;
                xv[i][k] = xh;
                acc[i][k] = fmaf(gv[i][k], xh, acc[i][k]);   // (a row past the range was requested as zeros)
                gv[i][k] *= wf[i][k];
                sgx = fmaf(gv[i][k], xh, sgx);
            }
        if (DX) {
            const float mgx = rb_row_sum<TPR>(sgx, red, par) * invC;
            par ^= 1;
#pragma unroll
            for (int i = 0; i < MAXCH; ++i) {
                const int c = i * TPR + tl;
                if (c < nchunk && r < r1) {
                    float rf[8], o[8];
                    unpack8(rv[i], rf);
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = rstd * (gv[i][k] - xv[i][k] * mgx) + rf[k];
                    const uint4_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
                    *reinterpret_cast<uint4_t *>(gx + r * ldgx + coff + c * 8) = ov;
                }
            }
        }
    }
    if (vb >= nbv) return;
    float *pp = part + ((size_t)grp * nbv + vb) * C;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = i * TPR + tl;
        if (c < nchunk) {
            *reinterpret_cast<float4_t *>(pp + c * 8) = (float4_t){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
            *reinterpret_cast<float4_t *>(pp + c * 8 + 4) = (float4_t){acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
        }
    }
}

// nn.LayerNorm backward inside the CLIP layer's chain (layer_train.cpp): rms_bwd_kernel's walk with a mean.  Per row the mean and the
// second moment about it are recomputed from x in fp32 (two passes over the registers: no cancellation);  xhat = (x - mean) r,
// g = grad_y gamma,  grad_x = r (g - mean(g) - xhat mean(g xhat)) [+ grad_res]  (one rounding),  grad_w = sum_rows grad_y xhat  (xhat NOT
// rounded),  grad_b = sum_rows grad_y.  The partials are [2][nbv][C]: grad_w's, then grad_b's.  A chunk past the row's end (a thread
// without work at this C) must stay out of the second moment: its x - mean is masked to zero, and everything behind it is zero too.
template <int MAXCH, int TPR, bool DX>
__global__ __launch_bounds__(RB_THREADS) void ln_res_bwd_kernel(const uint16_t *__restrict__ x, int ldx, const uint16_t *gy, int ldgy,
                                                                const uint16_t *__restrict__ w, uint16_t *gx, int ldgx,
                                                                const uint16_t *__restrict__ gres, int ldgr, float *__restrict__ part,
                                                                long rows, int C, int rpb, int nbv, float eps)
{
    __shared__ float red[2][4];
    constexpr int RG = RB_THREADS / TPR;
    const int tl = threadIdx.x % TPR, nchunk = C >> 3;
    const int vb = blockIdx.x * RG + threadIdx.x / TPR;
    float wf[MAXCH][8], accw[MAXCH][8], accb[MAXCH][8];
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = i * TPR + tl;
        uint4_t wv = {0, 0, 0, 0};
        if (c < nchunk) wv = *reinterpret_cast<const uint4_t *>(w + c * 8);
        unpack8(wv, wf[i]);
#pragma unroll
        for (int k = 0; k < 8; ++k) accw[i][k] = accb[i][k] = 0.f;
    }
    const float invC = 1.f / (float)C;
    const long r0 = (long)vb * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;   // (vb >= nbv: an empty range)
    uint4_t nx[MAXCH], ng[MAXCH], nr[MAXCH];
    auto request = [&](long r) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c = i * TPR + tl;
            nx[i] = ng[i] = nr[i] = (uint4_t){0, 0, 0, 0};
            if (c < nchunk && r < r1) {
                nx[i] = *reinterpret_cast<const uint4_t *>(x + r * ldx + c * 8);
                ng[i] = *reinterpret_cast<const uint4_t *>(gy + r * ldgy + c * 8);
                if (DX && gres) nr[i] = *reinterpret_cast<const uint4_t *>(gres + r * ldgr + c * 8);
            }
        }
    };
    request(r0);
    int par = 0;
    for (int it = 0; it < rpb; ++it) {   // (the same trip count in every thread: the row sums are block-wide barriers)
        const long r = r0 + it;
        float xv[MAXCH][8], gv[MAXCH][8];
        uint4_t rv[MAXCH];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            unpack8(nx[i], xv[i]);
            unpack8(ng[i], gv[i]);
            rv[i] = nr[i];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += xv[i][k];
        }
        request(r + 1);   // (another row than the one stored below: grad_x may alias grad_y)
        const float mean = rb_row_sum<TPR>(s, red, par) * invC;
        par ^= 1;
        float vs = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const bool own = i * TPR + tl < nchunk;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float dlt = own ? xv[i][k] - mean : 0.f;
                xv[i][k] = dlt;
                vs = fmaf(dlt, dlt, vs);
            }
        }
        const float rstd = rsqrtf(rb_row_sum<TPR>(vs, red, par) * invC + eps);
        par ^= 1;
        float sg = 0.f, sgx = 0.f;
#pragma unroll
        for (int i = 0; i < MAXCH; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float xh = xv[i][k] * rstd;
                xv[i][k] = xh;
                accw[i][k] = fmaf(gv[i][k], xh, accw[i][k]);   // (a row past the range was requested as zeros)
                accb[i][k] += gv[i][k];
                gv[i][k] *= wf[i][k];
                sg += gv[i][k];
                sgx = fmaf(gv[i][k], xh, sgx);
            }
        if (DX) {
            const float mg = rb_row_sum<TPR>(sg, red, par) * invC;
            par ^= 1;
            const float mgx = rb_row_sum<TPR>(sgx, red, par) * invC;
            par ^= 1;
#pragma unroll
            for (int i = 0; i < MAXCH; ++i) {
                const int c = i * TPR + tl;
                if (c < nchunk && r < r1) {
                    float rf[8], o[8];
                    unpack8(rv[i], rf);
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = rstd * (gv[i][k] - mg - xv[i][k] * mgx) + rf[k];
                    const uint4_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
                    *reinterpret_cast<uint4_t *>(gx + r * ldgx + c * 8) = ov;
                }
            }
        }
    }
    if (vb >= nbv) return;
    float *pw = part + (size_t)vb * C, *pb = part + ((size_t)nbv + vb) * C;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = i * TPR + tl;
        if (c < nchunk) {
            *reinterpret_cast<float4_t *>(pw + c * 8) = (float4_t){accw[i][0], accw[i][1], accw[i][2], accw[i][3]};
            *reinterpret_cast<float4_t *>(pw + c * 8 + 4) = (float4_t){accw[i][4], accw[i][5], accw[i][6], accw[i][7]};
            *reinterpret_cast<float4_t *>(pb + c * 8) = (float4_t){accb[i][0], accb[i][1], accb[i][2], accb[i][3]};
            *reinterpret_cast<float4_t *>(pb + c * 8 + 4) = (float4_t){accb[i][4], accb[i][5], accb[i][6], accb[i][7]};
        }
    }
}

template <int MAXCH, int TPR, bool DY>
__global__ __launch_bounds__(RB_THREADS) void ls_bwd_kernel(const uint16_t *__restrict__ go, int ldgo, const uint16_t *__restrict__ y, int ldy,
                                                            const uint16_t *__restrict__ ls, uint16_t *__restrict__ gy, int ldgy,
                                                            float *__restrict__ part, long rows, int C, int rpb, int nbv)
{
    constexpr int RG = RB_THREADS / TPR;
    const int tl = threadIdx.x % TPR, nchunk = C >> 3;
    const int vb = blockIdx.x * RG + threadIdx.x / TPR;
    if (vb >= nbv) return;   // (no barrier in this kernel)
    float sf[MAXCH][8], acc[MAXCH][8];
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = i * TPR + tl;
        uint4_t sv = {0, 0, 0, 0};
        if (c < nchunk) sv = *reinterpret_cast<const uint4_t *>(ls + c * 8);
        unpack8(sv, sf[i]);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[i][k] = 0.f;
    }
    const long r0 = (long)vb * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    uint4_t ng[2][MAXCH], ny[2][MAXCH];   // the two rows after the one at hand are in flight
    auto request = [&](long r, int slot) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c = i * TPR + tl;
            ng[slot][i] = ny[slot][i] = (uint4_t){0, 0, 0, 0};
            if (c < nchunk && r < r1) {
                ng[slot][i] = *reinterpret_cast<const uint4_t *>(go + r * ldgo + c * 8);
                if (part) ny[slot][i] = *reinterpret_cast<const uint4_t *>(y + r * ldy + c * 8);
            }
        }
    };
    request(r0, 0);
    request(r0 + 1, 1);
    for (long rr = r0; rr < r1; rr += 2) {
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {
            const long r = rr + slot;
            uint4_t cg[MAXCH], cy[MAXCH];
#pragma unroll
            for (int i = 0; i < MAXCH; ++i) { cg[i] = ng[slot][i]; cy[i] = ny[slot][i]; }
            request(r + 2, slot);
#pragma unroll
            for (int i = 0; i < MAXCH; ++i) {
                const int c = i * TPR + tl;
                float gf[8], yf[8];
                unpack8(cg[i], gf);
                unpack8(cy[i], yf);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[i][k] = fmaf(gf[k], yf[k], acc[i][k]);   // (rows past the range were requested as zeros)
                if (DY && c < nchunk && r < r1) {
                    float o[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = gf[k] * sf[i][k];
                    const uint4_t ov = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]), pack_bf16x2(o[4], o[5]), pack_bf16x2(o[6], o[7])};
                    *reinterpret_cast<uint4_t *>(gy + r * ldgy + c * 8) = ov;
                }
            }
        }
    }
    if (!part) return;
    float *pp = part + (size_t)vb * C;
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int c = i * TPR + tl;
        if (c < nchunk) {
            *reinterpret_cast<float4_t *>(pp + c * 8) = (float4_t){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
            *reinterpret_cast<float4_t *>(pp + c * 8 + 4) = (float4_t){acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
        }
    }
}

// out_g[c] = sum_b part[g][b][c] (group g = blockIdx.y; a NULL output is skipped).  A block owns 32 columns; its 8 slices each add a
// contiguous eighth of the nb partials in order, then slice 0 adds the 8 sums in order: a fixed tree, the same bits on every run.
__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float *__restrict__ part, int nb, int C, uint16_t *g0, uint16_t *g1)
{
    __shared__ float sl[8][32];
    const int cl = threadIdx.x & 31, sidx = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    uint16_t *out = blockIdx.y ? g1 : g0;
    if (!out) return;   // (block-uniform)
    const int per = (nb + 7) / 8, b0 = sidx * per, b1 = b0 + per < nb ? b0 + per : nb;
    float s = 0.f;
    if (c < C) {
        const float *p = part + (size_t)blockIdx.y * nb * C + c;
#pragma unroll 8
        for (int b = b0; b < b1; ++b) s += p[(size_t)b * C];
    }
    sl[sidx][cl] = s;
    __syncthreads();
    if (sidx == 0 && c < C) {
        float tot = sl[0][cl];
#pragma unroll
        for (int k = 1; k < 8; ++k) tot += sl[k][cl];
        out[c] = f32_to_bf16(tot);
    }
}

// threads per row (whole waves), chunks per thread, and the row ranges ("virtual blocks": 256 / tpr per block, two blocks per compute
// unit, each keeping one row in flight beside the one it works on)
struct RbPlan { int tpr, maxch, nbv, rpb, grid; };
static RbPlan rb_plan(long rows, int C)
{
    RbPlan p;
    const int nchunk = C / 8;
    p.tpr = nchunk <= 64 ? 64 : nchunk <= 128 ? 128 : 256;
    const int per = (nchunk + p.tpr - 1) / p.tpr;
    p.maxch = per <= 1 ? 1 : per <= 2 ? 2 : 4;
    const int rg = RB_THREADS / p.tpr;
    const long b = std::max(1L, std::min<long>(rows, 2L * device_cus() * rg));
    p.rpb = (int)((rows + b - 1) / b);
    p.nbv = p.rpb > 0 ? (int)((rows + p.rpb - 1) / p.rpb) : 1;
    p.grid = (p.nbv + rg - 1) / rg;
    return p;
}

long rms_bwd_workspace_bytes(long rows, int C, int G)
{
    if (rows < 0 || C <= 0 || C % 8 != 0 || C > RB_MAX_C || (G != 1 && G != 2)) return -1;
    return (long)G * rb_plan(rows, C).nbv * C * 4;
}

int rms_bwd_launch(const uint16_t *x, int ldx, const uint16_t *gy, int ldgy, const uint16_t *w, const uint16_t *w2, int G, float eps, long rows,
                   int C, uint16_t *gx, int ldgx, const uint16_t *gres, int ldgr, uint16_t *gw, uint16_t *gw2, void *ws, long ws_bytes,
                   hipStream_t st)
{
    VLLM_REQUIRE(rows >= 0 && C > 0 && C % 8 == 0 && C <= RB_MAX_C, "rmsnorm_backward: C=%d must be a multiple of 8 and <= %d", C, RB_MAX_C);
    VLLM_REQUIRE(G == 1 || (G == 2 && w2 && aligned16(w2) && !gres), "rmsnorm_backward: column groups: G = 2 with a second weight and no grad_res");
    VLLM_REQUIRE(G == 2 || !gw2, "rmsnorm_backward: grad_w2 belongs to G = 2");
    VLLM_REQUIRE((!gw || (reinterpret_cast<uintptr_t>(gw) & 1u) == 0) && (!gw2 || (reinterpret_cast<uintptr_t>(gw2) & 1u) == 0), "rmsnorm_backward: misaligned weight gradient");
    if (rows == 0) {   // no rows: the weight gradients are empty sums
        if (gw) VLLM_REQUIRE(hipMemsetAsync(gw, 0, (size_t)C * 2, st) == hipSuccess, "rmsnorm_backward: memset failed");
        if (gw2) VLLM_REQUIRE(hipMemsetAsync(gw2, 0, (size_t)C * 2, st) == hipSuccess, "rmsnorm_backward: memset failed");
        return VLLM_OK;
    }
    VLLM_REQUIRE(x && gy && w && aligned16(x) && aligned16(gy) && aligned16(w), "rmsnorm_backward: x, grad_y and weight must be 16-byte aligned device pointers");
    VLLM_REQUIRE(ldx >= G * C && ldgy >= G * C && ldx % 8 == 0 && ldgy % 8 == 0 && (!gx || (aligned16(gx) && ldgx >= G * C && ldgx % 8 == 0)) &&
                     (!gres || (gx && aligned16(gres) && ldgr >= C && ldgr % 8 == 0)),
                 "rmsnorm_backward: row strides must cover the row and be multiples of 8 elements, pointers 16-byte aligned (grad_res needs grad_x)");
    if (!gx && !gw && !gw2) return VLLM_OK;
    const RbPlan p = rb_plan(rows, C);
    const long need = (long)G * p.nbv * C * 4;
    VLLM_REQUIRE(ws && aligned16(ws) && ws_bytes >= need, "rmsnorm_backward: workspace too small or misaligned (%ld < %ld bytes)", ws_bytes, need);
    float *part = reinterpret_cast<float *>(ws);
    const dim3 grid((unsigned)p.grid, (unsigned)G), block(RB_THREADS);
#define L2(M, T, D) VLLM_LAUNCH((rms_bwd_kernel<M, T, D>), grid, block, 0, st, x, ldx, gy, ldgy, w, w2, gx, ldgx, gres, ldgr, part, rows, C, p.rpb, p.nbv, eps)
#define L1(M, T) do { if (gx) L2(M, T, true); else L2(M, T, false); } while (0)
    if (p.tpr == 64) L1(1, 64); else if (p.tpr == 128) L1(1, 128); else if (p.maxch == 1) L1(1, 256); else if (p.maxch == 2) L1(2, 256); else L1(4, 256);
#undef L1
#undef L2
    VLLM_CHECK_LAUNCH("rms_bwd_kernel");
    if (gw || gw2) {
        VLLM_LAUNCH(colsum_reduce_kernel, dim3((unsigned)ceil_div(C, 32), (unsigned)G), dim3(256), 0, st, part, p.nbv, C, gw, gw2);
        VLLM_CHECK_LAUNCH("colsum_reduce_kernel");
    }
    return VLLM_OK;
}

long ln_res_bwd_workspace_bytes(long rows, int C)
{
    if (rows < 0 || C <= 0 || C % 64 != 0 || C > RB_MAX_C) return -1;
    return 2L * rb_plan(rows, C).nbv * C * 4;
}

int ln_res_bwd_launch(const uint16_t *x, int ldx, const uint16_t *gy, int ldgy, const uint16_t *w, float eps, long rows, int C, uint16_t *gx,
                      int ldgx, const uint16_t *gres, int ldgr, uint16_t *gw, uint16_t *gb, void *ws, long ws_bytes, hipStream_t st)
{
    VLLM_REQUIRE(rows >= 0 && C > 0 && C % 64 == 0 && C <= RB_MAX_C, "layernorm_backward_res: C=%d must be a multiple of 64 and <= %d", C, RB_MAX_C);
    VLLM_REQUIRE((!gw || (reinterpret_cast<uintptr_t>(gw) & 1u) == 0) && (!gb || (reinterpret_cast<uintptr_t>(gb) & 1u) == 0),
                 "layernorm_backward_res: misaligned weight / bias gradient");
    if (rows == 0) {   // no rows: the column sums are empty sums
        if (gw) VLLM_REQUIRE(hipMemsetAsync(gw, 0, (size_t)C * 2, st) == hipSuccess, "layernorm_backward_res: memset failed");
        if (gb) VLLM_REQUIRE(hipMemsetAsync(gb, 0, (size_t)C * 2, st) == hipSuccess, "layernorm_backward_res: memset failed");
        return VLLM_OK;
    }
    VLLM_REQUIRE(x && gy && w && aligned16(x) && aligned16(gy) && aligned16(w), "layernorm_backward_res: x, grad_y and weight must be 16-byte aligned device pointers");
    VLLM_REQUIRE(ldx >= C && ldgy >= C && ldx % 8 == 0 && ldgy % 8 == 0 && (!gx || (aligned16(gx) && ldgx >= C && ldgx % 8 == 0)) &&
                     (!gres || (gx && aligned16(gres) && ldgr >= C && ldgr % 8 == 0)),
                 "layernorm_backward_res: row strides must cover the row and be multiples of 8 elements, pointers 16-byte aligned (grad_res needs grad_x)");
    if (!gx && !gw && !gb) return VLLM_OK;
    const RbPlan p = rb_plan(rows, C);
    const long need = 2L * p.nbv * C * 4;
    VLLM_REQUIRE(ws && aligned16(ws) && ws_bytes >= need, "layernorm_backward_res: workspace too small or misaligned (%ld < %ld bytes)", ws_bytes, need);
    float *part = reinterpret_cast<float *>(ws);
    const dim3 grid((unsigned)p.grid), block(RB_THREADS);
#define L2(M, T, D) VLLM_LAUNCH((ln_res_bwd_kernel<M, T, D>), grid, block, 0, st, x, ldx, gy, ldgy, w, gx, ldgx, gres, ldgr, part, rows, C, p.rpb, p.nbv, eps)
#define L1(M, T) do { if (gx) L2(M, T, true); else L2(M, T, false); } while (0)
    if (p.tpr == 64) L1(1, 64); else if (p.tpr == 128) L1(1, 128); else if (p.maxch == 1) L1(1, 256); else if (p.maxch == 2) L1(2, 256); else L1(4, 256);
#undef L1
#undef L2
    VLLM_CHECK_LAUNCH("ln_res_bwd_kernel");
    if (gw || gb) {
        VLLM_LAUNCH(colsum_reduce_kernel, dim3((unsigned)ceil_div(C, 32), 2u), dim3(256), 0, st, part, p.nbv, C, gw, gb);
        VLLM_CHECK_LAUNCH("colsum_reduce_kernel");
    }
    return VLLM_OK;
}

long ls_bwd_workspace_bytes(long rows, int C) { return rms_bwd_workspace_bytes(rows, C, 1); }

int ls_bwd_launch(const uint16_t *go, int ldgo, const uint16_t *y, int ldy, const uint16_t *ls, long rows, int C, uint16_t *gy, int ldgy,
                  uint16_t *gls, void *ws, long ws_bytes, hipStream_t st)
{
    VLLM_REQUIRE(rows >= 0 && C > 0 && C % 8 == 0 && C <= RB_MAX_C, "layerscale_backward: C=%d must be a multiple of 8 and <= %d", C, RB_MAX_C);
    VLLM_REQUIRE(!gls || (reinterpret_cast<uintptr_t>(gls) & 1u) == 0, "layerscale_backward: misaligned grad_ls");
    if (rows == 0) {
        if (gls) VLLM_REQUIRE(hipMemsetAsync(gls, 0, (size_t)C * 2, st) == hipSuccess, "layerscale_backward: memset failed");
        return VLLM_OK;
    }
    if (!gy && !gls) return VLLM_OK;
    VLLM_REQUIRE(go && aligned16(go) && ldgo >= C && ldgo % 8 == 0, "layerscale_backward: grad_out must be 16-byte aligned, row stride >= C and a multiple of 8");
    VLLM_REQUIRE(!gy || (ls && aligned16(ls) && aligned16(gy) && ldgy >= C && ldgy % 8 == 0), "layerscale_backward: grad_y needs ls; 16-byte aligned, row stride >= C and a multiple of 8");
    VLLM_REQUIRE(!gls || (y && aligned16(y) && ldy >= C && ldy % 8 == 0), "layerscale_backward: grad_ls needs y (16-byte aligned, row stride >= C and a multiple of 8)");
    const RbPlan p = rb_plan(rows, C);
    const long need = gls ? (long)p.nbv * C * 4 : 0;
    VLLM_REQUIRE(!gls || (ws && aligned16(ws) && ws_bytes >= need), "layerscale_backward: workspace too small or misaligned (%ld < %ld bytes)", ws_bytes, need);
    float *part = gls ? reinterpret_cast<float *>(ws) : nullptr;
    const uint16_t *lsp = gy ? ls : go;   // (never read without grad_y; any aligned address)
    const dim3 grid((unsigned)p.grid), block(RB_THREADS);
#define L2(M, T, D) VLLM_LAUNCH((ls_bwd_kernel<M, T, D>), grid, block, 0, st, go, ldgo, y, ldy, lsp, gy, ldgy, part, rows, C, p.rpb, p.nbv)
#define L1(M, T) do { if (gy) L2(M, T, true); else L2(M, T, false); } while (0)
    if (p.tpr == 64) L1(1, 64); else if (p.tpr == 128) L1(1, 128); else if (p.maxch == 1) L1(1, 256); else if (p.maxch == 2) L1(2, 256); else L1(4, 256);
#undef L1
#undef L2
    VLLM_CHECK_LAUNCH("ls_bwd_kernel");
    if (gls) {
        VLLM_LAUNCH(colsum_reduce_kernel, dim3((unsigned)ceil_div(C, 32), 1u), dim3(256), 0, st, part, p.nbv, C, gls, (uint16_t *)nullptr);
        VLLM_CHECK_LAUNCH("colsum_reduce_kernel");
    }
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_rmsnorm_bf16(const uint16_t *x, int ldx, const uint16_t *weight, uint16_t *y, int ldy, long rows,
                                 int C, float eps, vllm_stream_t stream)
{
    return norm_bf16_launch(true, x, ldx, weight, nullptr, y, ldy, rows, C, eps, (hipStream_t)stream);
}

extern "C" int vllm_layernorm_bf16(const uint16_t *x, int ldx, const uint16_t *weight, const uint16_t *bias,
                                   uint16_t *y, int ldy, long rows, int C, float eps, vllm_stream_t stream)
{
    return norm_bf16_launch(false, x, ldx, weight, bias, y, ldy, rows, C, eps, (hipStream_t)stream);
}

extern "C" long vllm_rmsnorm_backward_workspace_bytes(long rows, int C, int G) { return rms_bwd_workspace_bytes(rows, C, G); }

extern "C" int vllm_rmsnorm_backward_bf16(const uint16_t *x, int ldx, const uint16_t *grad_y, int ldg, const uint16_t *weight,
                                          const uint16_t *weight2, int G, float eps, long rows, int C, uint16_t *grad_x, int ldgx,
                                          const uint16_t *grad_res, int ldgr, uint16_t *grad_w, uint16_t *grad_w2, void *workspace,
                                          long workspace_bytes, vllm_stream_t stream)
{
    return rms_bwd_launch(x, ldx, grad_y, ldg, weight, weight2, G, eps, rows, C, grad_x, ldgx, grad_res, ldgr, grad_w, grad_w2, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

extern "C" long vllm_layernorm_backward_res_workspace_bytes(long rows, int C) { return ln_res_bwd_workspace_bytes(rows, C); }

extern "C" int vllm_layernorm_backward_res_bf16(const uint16_t *x, int ldx, const uint16_t *grad_y, int ldg, const uint16_t *weight, float eps,
                                                long rows, int C, uint16_t *grad_x, int ldgx, const uint16_t *grad_res, int ldgr,
                                                uint16_t *grad_w, uint16_t *grad_b, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    return ln_res_bwd_launch(x, ldx, grad_y, ldg, weight, eps, rows, C, grad_x, ldgx, grad_res, ldgr, grad_w, grad_b, workspace, workspace_bytes,
                             (hipStream_t)stream);
}

extern "C" long vllm_layerscale_backward_workspace_bytes(long rows, int C) { return ls_bwd_workspace_bytes(rows, C); }

extern "C" int vllm_layerscale_backward_bf16(const uint16_t *grad_out, int ldgo, const uint16_t *y, int ldy, const uint16_t *ls, long rows,
                                             int C, uint16_t *grad_y, int ldgy, uint16_t *grad_ls, void *workspace, long workspace_bytes,
                                             vllm_stream_t stream)
{
    return ls_bwd_launch(grad_out, ldgo, y, ldy, ls, rows, C, grad_y, ldgy, grad_ls, workspace, workspace_bytes, (hipStream_t)stream);
}
