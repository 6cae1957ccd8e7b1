// The INPUTS of the Grounding-DINO encoder for bf16 modules at inference: input_proj_vision (Conv2d + GroupNorm per level), the mask
// pyramid, the sine position embedding + level_embed, valid_ratios, all written in the encoder's [B, S, C] layout by one call.
// Reference: grounding_dino/modeling_ov_grounding_dino_mask_dn.py -- GroundingDinoSinePositionEmbedding :529-564, the mask down-sampling
//            :502 / :2406, input_proj_vision :2080-2111, level_embed :2164, get_valid_ratio :2200-2209, forward :2388-2439.
//
// One call, one stream, a caller workspace (include/vllm_hip.h, section f2h).  Per level:
//   nchw_to_rows_kernel     a contiguous NCHW map -> rows [B HW, Cin] (a channels-last map is the GEMM's operand in place), or
//   im2col3x3s2_kernel      the patch matrix [B Ho Wo, 9 Cin] of an extra level, from the last map's rows or the previous level's output
//   GEMM (EPI_BIAS)         the conv, bf16 out (the bf16 module's rounding)
//   gn_stats_kernel         {count, mean, M2} per (image, group, slab of 32 rows), M2 about the slab's own mean
//   gn_finalize_kernel      Chan's combination in a fixed order -> {mean, 1 / std} per (image, group)
//   gn_apply_kernel         (x - mean) rstd gamma + beta, one rounding, into the level's rows of out_source
// and once: pixel_mask_levels_kernel (masks, prefix counts, valid_ratios), sine_pos_embed_kernel (position embedding + level_embed).
// No kernel walks rows in a loop over the grid: a thread's work is fixed by its index.  No atomics: the same bits on every run.
#include <math.h>
#include "common.hpp"
#include "orchestrate.hpp"
#include "gdino_inputs.hpp"

namespace vllm {
namespace {

// ---- the transpose -------------------------------------------------------------------------------------------------------------------------
// One workgroup per 64 channels x 64 pixels of one image.  The tile lies in LDS as [channel][pixel] with 66 elements (33 dwords) per
// channel: the gather of 8 channels of one pixel then reads dwords 33 (8 k + e) + p / 2, which for the 8 chunks k and 4 pixel pairs of a
// wave are 32 different banks (8 k + p / 2 + const), each read by the two lanes of a pixel pair (one dword: a broadcast).
// VEC: HW a multiple of 8, so every 8-pixel run of a channel is one aligned 16-byte load; otherwise 2-byte loads.
constexpr int TR_LD = 66;
template <bool VEC>
__global__ __launch_bounds__(256) void nchw_to_rows_kernel(const uint16_t *__restrict__ in, int Cin, int HW, uint16_t *__restrict__ out, int ld_out)
{
    __shared__ uint32_t tile32[64 * TR_LD / 2];
    uint16_t *tile = reinterpret_cast<uint16_t *>(tile32);
    const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const long b = blockIdx.z;
    const uint16_t *src = in + (b * Cin + c0) * (long)HW;
    if (VEC) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = threadIdx.x + 256 * it, q = idx & 7, c = idx >> 3, p = p0 + 8 * q;
            if (p < HW) {
                const uint4_t v = *reinterpret_cast<const uint4_t *>(src + (long)c * HW + p);
#pragma unroll
                for (int i = 0; i < 4; ++i) tile32[c * (TR_LD / 2) + 4 * q + i] = v[i];
            }
        }
    } else {
#pragma unroll 4
        for (int it = 0; it < 16; ++it) {
            const int idx = threadIdx.x + 256 * it, p = idx & 63, c = idx >> 6;
            if (p0 + p < HW) tile[c * TR_LD + p] = src[(long)c * HW + p0 + p];
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = threadIdx.x + 256 * it, k = idx & 7, p = idx >> 3;
        if (p0 + p < HW) {
            uint32_t o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = (uint32_t)tile[(8 * k + 2 * e) * TR_LD + p] | ((uint32_t)tile[(8 * k + 2 * e + 1) * TR_LD + p] << 16);
            *reinterpret_cast<uint4_t *>(out + (b * HW + p0 + p) * ld_out + c0 + 8 * k) = (uint4_t){o[0], o[1], o[2], o[3]};
        }
    }
}

// ---- im2col ----------------------------------------------------------------------------------------------------------------------------------
// One thread per 16-byte chunk of the patch matrix: row (b, oy, ox), tap (ky, kx), 8 channels.
__global__ __launch_bounds__(256) void im2col3x3s2_kernel(const uint16_t *__restrict__ src, long src_bs, int ld, int Hi, int Wi, int Ho, int Wo,
                                                          int Cin, long chunks, uint16_t *__restrict__ out)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= chunks) return;
    const int cpr = Cin >> 3;
    const int j = (int)(t % cpr);
    const long rt = t / cpr;
    const int tap = (int)(rt % 9);
    const long orow = rt / 9;
    const int ox = (int)(orow % Wo);
    const long rb = orow / Wo;
    const int oy = (int)(rb % Ho);
    const long b = rb / Ho;
    const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
    uint4_t v = {0u, 0u, 0u, 0u};
    if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) v = *reinterpret_cast<const uint4_t *>(src + b * src_bs + ((long)iy * Wi + ix) * ld + j * 8);
    *reinterpret_cast<uint4_t *>(out + t * 8) = v;
}

// ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------------
// Thread (row, group) owns the C / 32 channels of one group in one row: hd = C / 64 dwords (1 .. 8).
// sum over the 8 threads of a workgroup that share a group (lanes g and g + 32 of each of the four waves), in every thread, in a fixed order
__device__ __forceinline__ float gn_block_sum(float s, float (*lds)[GN_GROUPS], int g)
{
    s += __shfl_xor(s, 32);
    if ((threadIdx.x & 63) < 32) lds[threadIdx.x >> 6][g] = s;
    __syncthreads();
    const float t = ((lds[0][g] + lds[1][g]) + lds[2][g]) + lds[3][g];
    __syncthreads();
    return t;
}

// grid (slabs, B): the slab's 32 rows x C channels once into registers; the group's mean over the slab, then M2 about that mean
__global__ __launch_bounds__(256) void gn_stats_kernel(const uint16_t *__restrict__ x, int ldx, int HW, int C, float *__restrict__ partials)
{
    __shared__ float lds[4][GN_GROUPS];
    const int hd = C >> 6;
    const int g = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    const int row_base = blockIdx.x * GN_SLAB_ROWS;
    const long b = blockIdx.y;
    uint32_t w[4][8];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = row_base + r0 + 8 * it;
        const uint32_t *p = reinterpret_cast<const uint32_t *>(x + (b * HW + row) * ldx) + g * hd;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            w[it][d] = (row < HW && d < hd) ? p[d] : 0u;
            s += bf16lo_to_f32(w[it][d]) + bf16hi_to_f32(w[it][d]);
        }
    }
    const int rows = HW - row_base < GN_SLAB_ROWS ? HW - row_base : GN_SLAB_ROWS;
    const float count = (float)(rows * 2 * hd);
    const float mean = __fdiv_rn(gn_block_sum(s, lds, g), count);
    float m2 = 0.f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int row = row_base + r0 + 8 * it;
#pragma unroll
        for (int d = 0; d < 8; ++d)
            if (row < HW && d < hd) {
                const float a = bf16lo_to_f32(w[it][d]) - mean, c = bf16hi_to_f32(w[it][d]) - mean;
                m2 += a * a + c * c;
            }
    }
    m2 = gn_block_sum(m2, lds, g);
    if (threadIdx.x < GN_GROUPS) {
        float *o = partials + ((b * gridDim.x + blockIdx.x) * GN_GROUPS + g) * 3;
        o[0] = count; o[1] = mean; o[2] = m2;
    }
}

// Chan et al.: {n, mean, M2} of the union of two sets from those of the sets
struct GnMoments { float n, mean, m2; };
__device__ __forceinline__ GnMoments gn_combine(const GnMoments &a, const GnMoments &b)
{
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float n = a.n + b.n, d = b.mean - a.mean;
    return {n, a.mean + d * __fdiv_rn(b.n, n), a.m2 + b.m2 + d * d * __fdiv_rn(a.n * b.n, n)};
}

// grid B: thread (part, g) combines slabs part, part + 8, ... in ascending order, thread (0, g) the eight parts in ascending order
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float *__restrict__ partials, int nslabs, float eps, float *__restrict__ stats)
{
    __shared__ float lds[8][GN_GROUPS][3];
    const int g = threadIdx.x & 31, part = threadIdx.x >> 5;
    const long b = blockIdx.x;
    GnMoments m = {0.f, 0.f, 0.f};
    for (int s = part; s < nslabs; s += 8) {
        const float *p = partials + ((b * nslabs + s) * GN_GROUPS + g) * 3;
        m = gn_combine(m, {p[0], p[1], p[2]});
    }
    lds[part][g][0] = m.n; lds[part][g][1] = m.mean; lds[part][g][2] = m.m2;
    __syncthreads();
    if (part == 0) {
        for (int k = 1; k < 8; ++k) m = gn_combine(m, {lds[k][g][0], lds[k][g][1], lds[k][g][2]});
        stats[(b * GN_GROUPS + g) * 2] = m.mean;
        stats[(b * GN_GROUPS + g) * 2 + 1] = 1.0f / sqrtf(__fdiv_rn(m.m2, m.n) + eps);   // the biased variance, as nn.GroupNorm
    }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const uint16_t *__restrict__ x, int ldx, const uint16_t *__restrict__ gamma,
                                                       const uint16_t *__restrict__ beta, const float *__restrict__ stats, long units, int HW, int C,
                                                       uint16_t *__restrict__ out, long out_bs, int ldo)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= units) return;
    const int hd = C >> 6;
    const int g = (int)(t & 31);
    const long row = t >> 5, b = row / HW, p = row - b * HW;
    const float mean = stats[(b * GN_GROUPS + g) * 2], rstd = stats[(b * GN_GROUPS + g) * 2 + 1];
    const uint32_t *xi = reinterpret_cast<const uint32_t *>(x + row * ldx) + g * hd;
    const uint32_t *gw = reinterpret_cast<const uint32_t *>(gamma) + g * hd, *gb = reinterpret_cast<const uint32_t *>(beta) + g * hd;
    uint32_t *o = reinterpret_cast<uint32_t *>(out + b * out_bs + p * ldo) + g * hd;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if (d < hd) {
            const uint32_t v = xi[d], wv = gw[d], bv = gb[d];
            const float lo = (bf16lo_to_f32(v) - mean) * rstd * bf16lo_to_f32(wv) + bf16lo_to_f32(bv);
            const float hi = (bf16hi_to_f32(v) - mean) * rstd * bf16hi_to_f32(wv) + bf16hi_to_f32(bv);
            o[d] = pack_bf16x2(lo, hi);
        }
}

// ---- the mask pyramid ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mask_at(const void *mask, int eb, long i)
{
    return eb == 8 ? reinterpret_cast<const int64_t *>(mask)[i] != 0 : reinterpret_cast<const uint8_t *>(mask)[i] != 0;
}
// F.interpolate(mode="nearest"): min(floor(dst * scale), in - 1), scale = float(in) / out, the product in fp32
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) { const int s = (int)floorf((float)dst * scale); return s < in - 1 ? s : in - 1; }

// One thread per (image, level, column) and per (image, level, row): a column thread walks down its column, writes the mask and the
// inclusive count along y; a row thread walks along its row and writes the count along x.  Column 0 and row 0 also give get_valid_ratio's
// sums, count * (1 / extent) in fp32: what torch's division of a device tensor by a host scalar computes (:2206-2207).
__global__ __launch_bounds__(256) void pixel_mask_levels_kernel(const void *__restrict__ mask, int eb, long units, int H, int W, LevelGeo geo,
                                                                int per_image, uint8_t *__restrict__ om, int32_t *__restrict__ yc,
                                                                int32_t *__restrict__ xc, float *__restrict__ vr)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= units) return;
    const long b = t / per_image;
    int u = (int)(t - b * per_image), l = 0;
    while (l + 1 < geo.L && u >= geo.h[l] + geo.w[l]) { u -= geo.h[l] + geo.w[l]; ++l; }
    const int hl = geo.h[l], wl = geo.w[l];
    const float sy = __fdiv_rn((float)H, (float)hl), sx = __fdiv_rn((float)W, (float)wl);
    const long base = b * geo.S + geo.start[l];
    const void *img = reinterpret_cast<const char *>(mask) + b * H * W * eb;
    int cnt = 0;
    if (u < wl) {
        const int x = u, px = nearest_src(x, sx, W);
        for (int y = 0; y < hl; ++y) {
            const int m = mask_at(img, eb, (long)nearest_src(y, sy, H) * W + px);
            cnt += m;
            om[base + (long)y * wl + x] = (uint8_t)m;
            yc[base + (long)y * wl + x] = cnt;
        }
        if (x == 0) vr[(b * geo.L + l) * 2 + 1] = (float)cnt * __fdiv_rn(1.0f, (float)hl);
    } else {
        const int y = u - wl, py = nearest_src(y, sy, H);
        for (int x = 0; x < wl; ++x) {
            cnt += mask_at(img, eb, (long)py * W + nearest_src(x, sx, W));
            xc[base + (long)y * wl + x] = cnt;
        }
        if (y == 0) vr[(b * geo.L + l) * 2] = (float)cnt * __fdiv_rn(1.0f, (float)wl);
    }
}

// ---- the position embedding ----------------------------------------------------------------------------------------------------------------
// One thread per 8 consecutive channels of a row (one 16-byte store): the first C / 2 channels from the count along y and the count in the
// column's last row, the others from the count along x and the row's last column.
__global__ __launch_bounds__(256) void sine_pos_embed_kernel(const int32_t *__restrict__ yc, const int32_t *__restrict__ xc, LevelGeo geo, long chunks,
                                                             int C, const uint16_t *__restrict__ level_embed, const float *__restrict__ dim_t,
                                                             uint16_t *__restrict__ out)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= chunks) return;
    const int cpr = C >> 3, half = C >> 1;
    const long row = t / cpr;
    const int c0 = (int)(t - row * cpr) * 8;
    const long b = row / geo.S;
    const int s = (int)(row - b * geo.S);
    int l = 0;
    for (int i = 1; i < geo.L; ++i)
        if (geo.start[i] <= s) l = i;
    const int wl = geo.w[l], idx = s - geo.start[l], y = idx / wl, x = idx - y * wl;
    const long base = b * geo.S + geo.start[l];
    const bool ypart = c0 < half;
    const int k0 = ypart ? c0 : c0 - half;
    const float cnt = (float)(ypart ? yc[base + idx] : xc[base + idx]);
    const float last = (float)(ypart ? yc[base + (long)(geo.h[l] - 1) * wl + x] : xc[base + (long)y * wl + wl - 1]);
    const float e = __fdiv_rn(cnt, last + 1e-6f) * 6.283185307179586f;
    const float4_t d0 = *reinterpret_cast<const float4_t *>(dim_t + k0), d1 = *reinterpret_cast<const float4_t *>(dim_t + k0 + 4);
    float le[8], o[8];
    unpack8(*reinterpret_cast<const uint4_t *>(level_embed + (long)l * C + c0), le);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a0 = __fdiv_rn(e, d0[i]), a1 = __fdiv_rn(e, d1[i]);
        o[i] = ((i & 1) ? cosf(a0) : sinf(a0)) + le[i];
        o[4 + i] = ((i & 1) ? cosf(a1) : sinf(a1)) + le[4 + i];
    }
    *reinterpret_cast<uint4_t *>(out + row * C + c0) = pack8(o);
}

// ---- launches (operands already checked) ------------------------------------------------------------------------------------------------------
unsigned blocks_of(long threads) { return (unsigned)((threads + 255) / 256); }

int nchw_to_rows_launch(const uint16_t *in, int B, int Cin, int HW, uint16_t *out, int ld_out, hipStream_t st)
{
    const dim3 grid((unsigned)((HW + 63) / 64), (unsigned)(Cin / 64), (unsigned)B);
    if (HW % 8 == 0) VLLM_LAUNCH(nchw_to_rows_kernel<true>, grid, dim3(256), 0, st, in, Cin, HW, out, ld_out);
    else VLLM_LAUNCH(nchw_to_rows_kernel<false>, grid, dim3(256), 0, st, in, Cin, HW, out, ld_out);
    VLLM_CHECK_LAUNCH("nchw_to_rows_kernel");
    return VLLM_OK;
}

int im2col3x3s2_launch(const uint16_t *src, long src_bs, int ld, int B, int Hi, int Wi, int Cin, uint16_t *out, hipStream_t st)
{
    const int Ho = conv3s2_extent(Hi), Wo = conv3s2_extent(Wi);
    const long chunks = (long)B * Ho * Wo * 9 * (Cin / 8);
    VLLM_LAUNCH(im2col3x3s2_kernel, dim3(blocks_of(chunks)), dim3(256), 0, st, src, src_bs, ld, Hi, Wi, Ho, Wo, Cin, chunks, out);
    VLLM_CHECK_LAUNCH("im2col3x3s2_kernel");
    return VLLM_OK;
}

struct GnWs { long partials, stats, total; };
GnWs gn_ws(long B, long HW)
{
    GnWs w;
    Carver cv;
    w.partials = cv.take(B * gn_slabs(HW) * GN_GROUPS * 3 * 4);
    w.stats = cv.take(B * GN_GROUPS * 2 * 4);
    w.total = cv.off;
    return w;
}

int groupnorm_launch(const uint16_t *x, int ldx, const uint16_t *gamma, const uint16_t *beta, float eps, int B, int HW, int C, uint16_t *out,
                     long out_bs, int ldo, void *workspace, hipStream_t st)
{
    const GnWs w = gn_ws(B, HW);
    float *partials = (float *)((char *)workspace + w.partials), *stats = (float *)((char *)workspace + w.stats);
    const int nslabs = (int)gn_slabs(HW);
    VLLM_LAUNCH(gn_stats_kernel, dim3((unsigned)nslabs, (unsigned)B), dim3(256), 0, st, x, ldx, HW, C, partials);
    VLLM_CHECK_LAUNCH("gn_stats_kernel");
    VLLM_LAUNCH(gn_finalize_kernel, dim3((unsigned)B), dim3(256), 0, st, partials, nslabs, eps, stats);
    VLLM_CHECK_LAUNCH("gn_finalize_kernel");
    const long units = (long)B * HW * GN_GROUPS;
    VLLM_LAUNCH(gn_apply_kernel, dim3(blocks_of(units)), dim3(256), 0, st, x, ldx, gamma, beta, stats, units, HW, C, out, out_bs, ldo);
    VLLM_CHECK_LAUNCH("gn_apply_kernel");
    return VLLM_OK;
}

int pixel_mask_levels_launch(const void *mask, int eb, int B, int H, int W, const LevelGeo &geo, uint8_t *om, int32_t *yc, int32_t *xc, float *vr,
                             hipStream_t st)
{
    int per_image = 0;
    for (int l = 0; l < geo.L; ++l) per_image += geo.h[l] + geo.w[l];
    const long units = (long)B * per_image;
    VLLM_LAUNCH(pixel_mask_levels_kernel, dim3(blocks_of(units)), dim3(256), 0, st, mask, eb, units, H, W, geo, per_image, om, yc, xc, vr);
    VLLM_CHECK_LAUNCH("pixel_mask_levels_kernel");
    return VLLM_OK;
}

int sine_pos_embed_launch(const int32_t *yc, const int32_t *xc, const LevelGeo &geo, int B, int C, const uint16_t *level_embed, const float *dim_t,
                          uint16_t *out, hipStream_t st)
{
    const long chunks = (long)B * geo.S * (C / 8);
    VLLM_LAUNCH(sine_pos_embed_kernel, dim3(blocks_of(chunks)), dim3(256), 0, st, yc, xc, geo, chunks, C, level_embed, dim_t, out);
    VLLM_CHECK_LAUNCH("sine_pos_embed_kernel");
    return VLLM_OK;
}

// ---- refusals shared by the entries ------------------------------------------------------------------------------------------------------------
constexpr long GRID_MAX = (1L << 31) - 1;

bool d_model_ok(int C) { return C >= 64 && C <= 512 && C % 64 == 0; }

// level_h / level_w (host) -> geo; B S below 2^31
int level_geo(const char *who, const int *level_h, const int *level_w, int L, int B, LevelGeo *geo)
{
    VLLM_REQUIRE(L >= 1 && L <= GI_MAX_LEVELS, "%s: L=%d (1 .. %d)", who, L, GI_MAX_LEVELS);
    VLLM_REQUIRE(level_h && level_w, "%s: null pointer (level_h / level_w)", who);
    VLLM_REQUIRE(B >= 0 && B <= 65535, "%s: B=%d (0 .. 65535)", who, B);
    long S = 0;
    geo->L = L;
    for (int l = 0; l < GI_MAX_LEVELS; ++l) { geo->h[l] = geo->w[l] = 1; geo->start[l] = 0; }
    for (int l = 0; l < L; ++l) {
        VLLM_REQUIRE(level_h[l] >= 1 && level_w[l] >= 1 && level_h[l] <= 32768 && level_w[l] <= 32768, "%s: level %d is %d x %d (1 .. 32768 each)", who,
                     l, level_h[l], level_w[l]);
        geo->h[l] = level_h[l]; geo->w[l] = level_w[l]; geo->start[l] = (int)S;
        S += (long)level_h[l] * level_w[l];
        VLLM_REQUIRE(S * (B > 0 ? B : 1) < (1L << 31), "%s: B=%d with %ld cells up to level %d (B S below 2^31)", who, B, S, l);
    }
    geo->S = (int)S;
    return VLLM_OK;
}

int mask_operand_ok(const char *who, const void *pixel_mask, int eb, int H, int W)
{
    VLLM_REQUIRE(eb == 1 || eb == 8, "%s: mask_elem_bytes=%d (1: bool / uint8, 8: int64)", who, eb);
    VLLM_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: pixel mask %d x %d (1 .. 32768 each)", who, H, W);
    VLLM_REQUIRE(pixel_mask, "%s: null pointer (pixel_mask)", who);
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(pixel_mask) & (uintptr_t)(eb - 1)) == 0, "%s: misaligned pixel_mask (%d bytes)", who, eb);
    return VLLM_OK;
}

int groupnorm_check(const char *who, const uint16_t *x, int ldx, const uint16_t *gamma, const uint16_t *beta, float eps, int B, int HW, int C,
                    const uint16_t *out, long out_bs, int ldo)
{
    VLLM_REQUIRE(d_model_ok(C), "%s: C=%d (a multiple of 64 in 64 .. 512)", who, C);
    VLLM_REQUIRE(B >= 0 && B <= 65535 && HW >= 0 && (long)B * HW * GN_GROUPS < GRID_MAX * 256 && (long)B * HW < (1L << 31),
                 "%s: B=%d HW=%d (B 0 .. 65535, B HW below 2^31)", who, B, HW);
    VLLM_REQUIRE(eps >= 0.f, "%s: negative eps", who);
    if ((long)B * HW == 0) return VLLM_OK;
    VLLM_REQUIRE(x && gamma && beta && out, "%s: null pointer (x / gamma / beta / out)", who);
    VLLM_REQUIRE(row_operand_ok(x, ldx, C) && row_operand_ok(out, ldo, C) && aligned16(gamma) && aligned16(beta) && out_bs % 8 == 0 &&
                     out_bs >= (long)(HW - 1) * ldo + C,
                 "%s: misaligned operand (x, gamma, beta, out 16 bytes) or ldx=%d / ldo=%d / out_batch_stride=%ld (multiples of 8, rows of C "
                 "elements, an image's rows inside its batch stride)", who, ldx, ldo, out_bs);
    return VLLM_OK;
}

// ---- the orchestrator ------------------------------------------------------------------------------------------------------------------------
const char *const GI = "gdino_inputs";

struct GiPlan {
    LevelGeo geo;
    long rows, conv, col, gn, ycnt, xcnt, total;   // offsets: the transposed map; the conv output; the patch matrix; GroupNorm's scratch; the counts
};

int gi_check_desc(const VllmGdinoInputsDesc *d)
{
    VLLM_REQUIRE(d, "%s: null descriptor", GI);
    VLLM_REQUIRE(d_model_ok(d->d_model), "%s: d_model=%d (a multiple of 64 in 64 .. 512)", GI, d->d_model);
    VLLM_REQUIRE(d->n_levels >= 1 && d->n_levels <= GI_MAX_LEVELS && d->n_maps >= 1 && d->n_maps <= d->n_levels,
                 "%s: n_levels=%d n_maps=%d (1 <= n_maps <= n_levels <= %d)", GI, d->n_levels, d->n_maps, GI_MAX_LEVELS);
    for (int l = 0; l < d->n_levels; ++l) {
        const int want = l < d->n_maps ? d->c_in[l] : l == d->n_maps ? d->c_in[d->n_maps - 1] : d->d_model;
        VLLM_REQUIRE(d->c_in[l] >= 64 && d->c_in[l] <= 16384 && d->c_in[l] % 64 == 0 && d->c_in[l] == want,
                     "%s: c_in[%d]=%d (a multiple of 64 in 64 .. 16384; an extra level reads the last map or d_model channels)", GI, l, d->c_in[l]);
        VLLM_REQUIRE(d->gn_eps[l] >= 0.f, "%s: negative eps (level %d)", GI, l);
        VLLM_REQUIRE(d->conv_w[l] && d->conv_b[l] && d->gn_w[l] && d->gn_b[l], "%s: missing weights (level %d)", GI, l);
        VLLM_REQUIRE(aligned16(d->conv_w[l]) && aligned16(d->conv_b[l]) && aligned16(d->gn_w[l]) && aligned16(d->gn_b[l]),
                     "%s: misaligned weight or bias (16 bytes; level %d)", GI, l);
    }
    VLLM_REQUIRE(d->level_embed && d->dim_t, "%s: missing level_embed / dim_t", GI);
    VLLM_REQUIRE(aligned16(d->level_embed) && aligned16(d->dim_t), "%s: misaligned level_embed / dim_t (16 bytes)", GI);
    return VLLM_OK;
}

// the levels' extents, every size rule, the workspace's pieces (B > 0)
int gi_plan(const VllmGdinoInputsDesc *d, int B, const int *map_h, const int *map_w, const int *map_format, GiPlan *p)
{
    VLLM_REQUIRE(map_h && map_w && map_format, "%s: null pointer (map_h / map_w / map_format)", GI);
    int h[GI_MAX_LEVELS], w[GI_MAX_LEVELS];
    for (int l = 0; l < d->n_levels; ++l) {
        if (l < d->n_maps) {
            VLLM_REQUIRE(map_format[l] == 0 || map_format[l] == 1, "%s: map_format[%d]=%d (0: contiguous NCHW, 1: channels-last)", GI, l, map_format[l]);
            h[l] = map_h[l]; w[l] = map_w[l];
            VLLM_REQUIRE(h[l] >= 1 && w[l] >= 1 && h[l] <= 32768 && w[l] <= 32768, "%s: map %d is %d x %d (1 .. 32768 each)", GI, l, h[l], w[l]);
        } else {
            h[l] = conv3s2_extent(h[l - 1]); w[l] = conv3s2_extent(w[l - 1]);
        }
    }
    TRY(level_geo(GI, h, w, d->n_levels, B, &p->geo));
    const long C = d->d_model;
    long rows = 0, conv = 0, col = 0, gn = 0;
    for (int l = 0; l < d->n_levels; ++l) {
        const long M = (long)B * h[l] * w[l], K = l < d->n_maps ? d->c_in[l] : 9L * d->c_in[l];
        // (the GEMMs address an operand with 32-bit byte offsets)
        VLLM_REQUIRE(M * (K > C ? K : C) * 2 < (1L << 31), "%s: level %d has %ld rows of %ld elements (a GEMM operand below 2^31 bytes)", GI, l, M, K);
        if (l < d->n_maps && map_format[l] == 0 && M * K * 2 > rows) rows = M * K * 2;
        if (l >= d->n_maps && M * K * 2 > col) col = M * K * 2;
        if (M * C * 2 > conv) conv = M * C * 2;
        const long g = gn_ws(B, (long)h[l] * w[l]).total;
        if (g > gn) gn = g;
    }
    Carver cv;
    p->rows = cv.take(rows);
    p->conv = cv.take(conv);
    p->col = cv.take(col);
    p->gn = cv.take(gn);
    p->ycnt = cv.take((long)B * p->geo.S * 4);
    p->xcnt = cv.take((long)B * p->geo.S * 4);
    p->total = cv.off;
    return VLLM_OK;
}

long g_gi_calls = 0;

}  // namespace
}  // namespace vllm

using namespace vllm;

static_assert(sizeof(VllmGdinoInputsDesc) == (4 + 8) * sizeof(int32_t) + 8 * sizeof(float) + (4 * 8 + 2) * sizeof(void *),
              "VllmGdinoInputsDesc: 34 pointers behind 20 scalars");

extern "C" unsigned long vllm_gdino_inputs_desc_sizeof(void) { return sizeof(VllmGdinoInputsDesc); }
extern "C" long vllm_gdino_inputs_calls(void) { return g_gi_calls; }

extern "C" int vllm_nchw_to_rows_bf16(const uint16_t *in, int B, int Cin, int HW, uint16_t *out, int ld_out, vllm_stream_t stream)
{
    VLLM_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cin <= 64 * 65535, "nchw_to_rows: Cin=%d (a positive multiple of 64)", Cin);
    VLLM_REQUIRE(B >= 0 && B <= 65535 && HW >= 0 && (long)B * HW < (1L << 31), "nchw_to_rows: B=%d HW=%d (B 0 .. 65535, B HW below 2^31)", B, HW);
    if ((long)B * HW == 0) return VLLM_OK;
    VLLM_REQUIRE(in && out, "nchw_to_rows: null pointer (in / out)");
    VLLM_REQUIRE(aligned16(in) && row_operand_ok(out, ld_out, Cin), "nchw_to_rows: misaligned operand (in, out 16 bytes) or ld_out=%d (a multiple of 8, at least Cin)",
                 ld_out);
    return nchw_to_rows_launch(in, B, Cin, HW, out, ld_out, (hipStream_t)stream);
}

extern "C" int vllm_im2col3x3s2_bf16(const uint16_t *src, long src_batch_stride, int ld_src, int B, int Hi, int Wi, int Cin, uint16_t *out,
                                     vllm_stream_t stream)
{
    VLLM_REQUIRE(Cin >= 8 && Cin % 8 == 0, "im2col3x3s2: Cin=%d (a positive multiple of 8)", Cin);
    VLLM_REQUIRE(B >= 0 && Hi >= 0 && Wi >= 0 && Hi <= 32768 && Wi <= 32768, "im2col3x3s2: B=%d Hi=%d Wi=%d (non-negative, extents up to 32768)", B, Hi, Wi);
    if (B == 0 || Hi == 0 || Wi == 0) return VLLM_OK;
    const long chunks = (long)B * conv3s2_extent(Hi) * conv3s2_extent(Wi) * 9 * (Cin / 8);
    VLLM_REQUIRE(chunks < GRID_MAX * 256, "im2col3x3s2: %ld chunks of 16 bytes (below 2^39)", chunks);
    VLLM_REQUIRE(src && out, "im2col3x3s2: null pointer (src / out)");
    VLLM_REQUIRE(row_operand_ok(src, ld_src, Cin) && aligned16(out) && src_batch_stride % 8 == 0 && src_batch_stride >= 0,
                 "im2col3x3s2: misaligned operand (src, out 16 bytes) or ld_src=%d / src_batch_stride=%ld (multiples of 8, ld_src at least Cin)", ld_src,
                 src_batch_stride);
    return im2col3x3s2_launch(src, src_batch_stride, ld_src, B, Hi, Wi, Cin, out, (hipStream_t)stream);
}

extern "C" long vllm_groupnorm_rows_workspace_bytes(int B, int HW, int C)
{
    if (!d_model_ok(C)) { set_error("groupnorm_rows: C=%d (a multiple of 64 in 64 .. 512)", C); return -1; }
    if (B < 0 || HW < 0 || B > 65535 || (long)B * HW >= (1L << 31)) { set_error("groupnorm_rows: B=%d HW=%d (B 0 .. 65535, B HW below 2^31)", B, HW); return -1; }
    if ((long)B * HW == 0) return 0;
    return gn_ws(B, HW).total;
}

extern "C" int vllm_groupnorm_rows_bf16(const uint16_t *x, int ldx, const uint16_t *gamma, const uint16_t *beta, float eps, int B, int HW, int C,
                                        uint16_t *out, long out_batch_stride, int ldo, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    const char *who = "groupnorm_rows";
    TRY(groupnorm_check(who, x, ldx, gamma, beta, eps, B, HW, C, out, out_batch_stride, ldo));
    if ((long)B * HW == 0) return VLLM_OK;
    const long need = gn_ws(B, HW).total;
    VLLM_REQUIRE(workspace, "%s: null workspace (%ld bytes)", who, need);
    VLLM_REQUIRE(aligned16(workspace), "%s: misaligned workspace (16 bytes)", who);
    VLLM_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%ld < %ld bytes)", who, workspace_bytes, need);
    const long xbytes = ((long)B * HW - 1) * ldx * 2 + C * 2, obytes = ((long)(B - 1) * out_batch_stride + (long)(HW - 1) * ldo + C) * 2;
    VLLM_REQUIRE(!ranges_overlap(workspace, need, x, xbytes) && !ranges_overlap(workspace, need, out, obytes), "%s: workspace overlaps an operand", who);
    return groupnorm_launch(x, ldx, gamma, beta, eps, B, HW, C, out, out_batch_stride, ldo, workspace, (hipStream_t)stream);
}

extern "C" int vllm_pixel_mask_levels_u8(const void *pixel_mask, int mask_elem_bytes, int B, int H, int W, const int *level_h, const int *level_w,
                                         int L, uint8_t *out_mask, int32_t *out_ycnt, int32_t *out_xcnt, float *out_valid_ratios, vllm_stream_t stream)
{
    const char *who = "pixel_mask_levels";
    LevelGeo geo;
    TRY(level_geo(who, level_h, level_w, L, B, &geo));
    VLLM_REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 8, "%s: mask_elem_bytes=%d (1: bool / uint8, 8: int64)", who, mask_elem_bytes);
    VLLM_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: pixel mask %d x %d (1 .. 32768 each)", who, H, W);
    if (B == 0) return VLLM_OK;
    TRY(mask_operand_ok(who, pixel_mask, mask_elem_bytes, H, W));
    VLLM_REQUIRE(out_mask && out_ycnt && out_xcnt && out_valid_ratios, "%s: null pointer (out_mask / out_ycnt / out_xcnt / out_valid_ratios)", who);
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(out_ycnt) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_xcnt) & 3u) == 0 && aligned8(out_valid_ratios),
                 "%s: misaligned operand (out_ycnt, out_xcnt 4 bytes; out_valid_ratios 8)", who);
    return pixel_mask_levels_launch(pixel_mask, mask_elem_bytes, B, H, W, geo, out_mask, out_ycnt, out_xcnt, out_valid_ratios, (hipStream_t)stream);
}

extern "C" int vllm_sine_pos_embed_rows_bf16(const int32_t *ycnt, const int32_t *xcnt, const int *level_h, const int *level_w, int L, int B, int C,
                                             const uint16_t *level_embed, const float *dim_t, uint16_t *out, vllm_stream_t stream)
{
    const char *who = "sine_pos_embed_rows";
    VLLM_REQUIRE(d_model_ok(C), "%s: C=%d (a multiple of 64 in 64 .. 512)", who, C);
    LevelGeo geo;
    TRY(level_geo(who, level_h, level_w, L, B, &geo));
    if (B == 0) return VLLM_OK;
    VLLM_REQUIRE(ycnt && xcnt && level_embed && dim_t && out, "%s: null pointer (ycnt / xcnt / level_embed / dim_t / out)", who);
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(ycnt) & 3u) == 0 && (reinterpret_cast<uintptr_t>(xcnt) & 3u) == 0 && aligned16(level_embed) &&
                     aligned16(dim_t) && aligned16(out),
                 "%s: misaligned operand (level_embed, dim_t, out 16 bytes; ycnt, xcnt 4)", who);
    return sine_pos_embed_launch(ycnt, xcnt, geo, B, C, level_embed, dim_t, out, (hipStream_t)stream);
}

extern "C" long vllm_gdino_inputs_workspace_bytes(const VllmGdinoInputsDesc *d, int B, const int *map_h, const int *map_w, const int *map_format)
{
    GiPlan p;
    if (gi_check_desc(d) != VLLM_OK) return -1;
    if (B < 0) { set_error("%s: B=%d (0 .. 65535)", GI, B); return -1; }
    if (gi_plan(d, B, map_h, map_w, map_format, &p) != VLLM_OK) return -1;
    return B == 0 ? 0 : p.total;
}

extern "C" int vllm_gdino_inputs_forward(const VllmGdinoInputsDesc *d, const uint16_t *const *maps, const int *map_h, const int *map_w,
                                         const int *map_format, const void *pixel_mask, int mask_elem_bytes, int B, int H, int W,
                                         uint16_t *out_source, uint16_t *out_pos, uint8_t *out_mask, float *out_valid_ratios, void *workspace,
                                         long workspace_bytes, vllm_stream_t stream)
{
    GiPlan p;
    TRY(gi_check_desc(d));
    TRY(gi_plan(d, B, map_h, map_w, map_format, &p));
    VLLM_REQUIRE(mask_elem_bytes == 1 || mask_elem_bytes == 8, "%s: mask_elem_bytes=%d (1: bool / uint8, 8: int64)", GI, mask_elem_bytes);
    VLLM_REQUIRE(H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "%s: pixel mask %d x %d (1 .. 32768 each)", GI, H, W);
    if (B == 0) return VLLM_OK;
    const LevelGeo &geo = p.geo;
    const int C = d->d_model, NL = d->n_levels, NM = d->n_maps;
    const long S = geo.S, obytes = (long)B * S * C * 2;
    TRY(mask_operand_ok(GI, pixel_mask, mask_elem_bytes, H, W));
    VLLM_REQUIRE(maps && out_source && out_pos && out_mask && out_valid_ratios,
                 "%s: null pointer (maps / out_source / out_pos / out_mask / out_valid_ratios)", GI);
    for (int l = 0; l < NM; ++l) {
        VLLM_REQUIRE(maps[l], "%s: null pointer (map %d)", GI, l);
        VLLM_REQUIRE(aligned16(maps[l]), "%s: misaligned map %d (16 bytes)", GI, l);
    }
    VLLM_REQUIRE(aligned16(out_source) && aligned16(out_pos) && aligned8(out_valid_ratios),
                 "%s: misaligned out_source / out_pos (16 bytes) or out_valid_ratios (8)", GI);
    const struct { const void *p; long bytes; } outs[] = {{out_source, obytes}, {out_pos, obytes}, {out_mask, (long)B * S}, {out_valid_ratios, (long)B * NL * 8}};
    for (int i = 0; i < 4; ++i) {
        for (int j = i + 1; j < 4; ++j)
            VLLM_REQUIRE(!ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes), "%s: two outputs overlap", GI);
        for (int l = 0; l < NM; ++l)
            VLLM_REQUIRE(!ranges_overlap(outs[i].p, outs[i].bytes, maps[l], (long)B * geo.h[l] * geo.w[l] * d->c_in[l] * 2), "%s: an output overlaps map %d", GI, l);
        VLLM_REQUIRE(!ranges_overlap(outs[i].p, outs[i].bytes, pixel_mask, (long)B * H * W * mask_elem_bytes), "%s: an output overlaps pixel_mask", GI);
    }
    VLLM_REQUIRE(workspace, "%s: null workspace (%ld bytes)", GI, p.total);
    VLLM_REQUIRE(aligned16(workspace), "%s: misaligned workspace (16 bytes)", GI);
    VLLM_REQUIRE(workspace_bytes >= p.total, "%s: workspace too small (%ld < %ld bytes)", GI, workspace_bytes, p.total);
    for (int i = 0; i < 4; ++i)
        VLLM_REQUIRE(!ranges_overlap(workspace, p.total, outs[i].p, outs[i].bytes), "%s: workspace overlaps an operand", GI);
    for (int l = 0; l < NM; ++l)
        VLLM_REQUIRE(!ranges_overlap(workspace, p.total, maps[l], (long)B * geo.h[l] * geo.w[l] * d->c_in[l] * 2), "%s: workspace overlaps an operand", GI);
    VLLM_REQUIRE(!ranges_overlap(workspace, p.total, pixel_mask, (long)B * H * W * mask_elem_bytes), "%s: workspace overlaps an operand", GI);
    ++g_gi_calls;

    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    uint16_t *rows = (uint16_t *)(ws + p.rows), *conv = (uint16_t *)(ws + p.conv), *col = (uint16_t *)(ws + p.col);
    int32_t *yc = (int32_t *)(ws + p.ycnt), *xc = (int32_t *)(ws + p.xcnt);
    const uint16_t *last_rows = nullptr;   // the last map as channels-last rows: the first extra level's source
    for (int l = 0; l < NL; ++l) {
        const int hw = geo.h[l] * geo.w[l], Cin = d->c_in[l];
        const long M = (long)B * hw;
        const uint16_t *X;
        int K;
        if (l < NM) {
            // the 1 x 1 conv of :2089 / :2107 on the map's rows
            if (map_format[l] == 0) { TRY(nchw_to_rows_launch(maps[l], B, Cin, hw, rows, Cin, st)); X = rows; }
            else X = maps[l];
            K = Cin;
            last_rows = X;
        } else {
            // the 3 x 3 / stride 2 conv of :2097 on the last map (:2403) or on the level before (:2405), as a GEMM on its patch matrix
            if (l == NM) TRY(im2col3x3s2_launch(last_rows, (long)geo.h[l - 1] * geo.w[l - 1] * Cin, Cin, B, geo.h[l - 1], geo.w[l - 1], Cin, col, st));
            else TRY(im2col3x3s2_launch(out_source + (long)geo.start[l - 1] * C, S * C, C, B, geo.h[l - 1], geo.w[l - 1], Cin, col, st));
            X = col;
            K = 9 * Cin;
        }
        TRY(gemm(st, EPI_BIAS, X, K, d->conv_w[l], K, d->conv_b[l], conv, C, (int)M, C, K));
        // GroupNorm(32, C) (:2090 / :2098) into the level's rows of out_source (:2426, :2433)
        TRY(groupnorm_launch(conv, C, d->gn_w[l], d->gn_b[l], d->gn_eps[l], B, hw, C, out_source + (long)geo.start[l] * C, S * C, C, ws + p.gn, st));
    }
    // :502 / :2406, :549-550, :2438
    TRY(pixel_mask_levels_launch(pixel_mask, mask_elem_bytes, B, H, W, geo, out_mask, yc, xc, out_valid_ratios, st));
    // :551-563, :2429
    return sine_pos_embed_launch(yc, xc, geo, B, C, d->level_embed, d->dim_t, out_pos, st);
}
