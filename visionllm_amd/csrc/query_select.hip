// The two-stage QUERY SELECTION of Grounding-DINO for bf16 modules at inference, as one call: gen_encoder_output_proposals and the
// statements of OVGroundingDinoModel.forward between the encoder and the decoder
// (grounding_dino/modeling_ov_grounding_dino_mask_dn.py:2228-2276, :2503-2543, GroundingDinoContrastiveEmbedding :1410-1428).
//
// The selection depends only on the row maximum of the class logits, and the box head, the logit rows and the proposal logits are needed
// for the k selected rows only.  One call, one stream, a caller workspace, in order:
//   qs_extents_kernel      valid_height / valid_width per image and level (a fixed-order count)                           (:2248-2249)
//   GEMM + bias            enc_output on the raw memory rows, read in place                                               (:2275)
//   qs_norm_kernel         enc_output_norm in place; a row the reference zero-fills (padded, or an invalid proposal) is
//                          normalised from the bias itself -- Linear(0) is the bias bit for bit                           (:2266, :2273-2275)
//   rowmax_dot_kernel      score[b, s] = bf16(max over unmasked tokens of q . text), fp32 accumulation on the bf16 MFMA;
//                          the [B, S, Lt] logits are never written                                                        (:1421-1422, :2520)
//   topk_rows_kernel       the k largest per image: value descending, ties by ascending index, NaN greatest               (:2521)
//   qs_gather_kernel       the k object queries per image -> target                                                       (:2541)
//   GEMM + ReLU twice, qs_tail_kernel   the box head over B k rows; its last linear in fp32, plus the row's proposal logit
//                          recomputed from its index -> coords_logits, reference_points = sigmoid                         (:2515-2531)
//   rowmax_dot_kernel<LOGITS>   the selected rows' class logits, bf16-rounded, widened to fp32 [k, max_text_len]          (:2532-2534)
// No atomics on any output, a fixed order of operations: the same bits on every run.  (topk_rows_kernel counts with integer LDS
// atomics, which commute exactly, and orders what it has collected by a sort.)
#include <math.h>
#include "common.hpp"
#include "orchestrate.hpp"
#include "row_groups.hpp"

namespace vllm {
namespace {

constexpr int QS_MAX_LEVELS = 16;

// ---- proposals (:2244-2269) ----------------------------------------------------------------------------------------------------------
// extents [B, L, 2] int32 = {valid_height, valid_width}: the unpadded cells of column 0 / of row 0 of the level's map.  One wave per
// (image, level): lane i counts the cells i, i + 64, ..., the lanes' counts go through one xor tree (integers: any order is the same
// count).  A cell behind S (level tensors that do not describe S rows) is not read.
__global__ __launch_bounds__(64) void qs_extents_kernel(const uint8_t *__restrict__ pmask, const int64_t *__restrict__ shapes,
                                                        const int64_t *__restrict__ lsi, int L, int S, int *__restrict__ extents)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const int b = t / L, l = t - b * L;
    const long H = shapes[2 * l], W = shapes[2 * l + 1], s0 = lsi[l];
    const uint8_t *m = pmask + (long)b * S;
    int vh = 0, vw = 0;
    for (long y = lane; y < H; y += 64) {
        const long i = s0 + y * W;
        if (i >= 0 && i < S) vh += m[i] == 0;
    }
    for (long x = lane; x < W; x += 64) {
        const long i = s0 + x;
        if (i >= 0 && i < S) vw += m[i] == 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        vh += __shfl_xor(vh, o);
        vw += __shfl_xor(vw, o);
    }
    if (lane == 0) {
        extents[2 * t] = vh;
        extents[2 * t + 1] = vw;
    }
}

// The proposal of row s of image b, with the reference's fp32 operations: one add, one true division by the extent, 0.05 * 2^level; valid
// when all four values lie strictly inside (0.01, 0.99).
struct QsProposal { float v[4]; bool valid; };
__device__ __forceinline__ QsProposal qs_proposal(long s, int b, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi, int L,
                                                  const int *__restrict__ extents)
{
    int l = 0;
    for (int i = 1; i < L; ++i)
        if (lsi[i] <= s) l = i;
    const long r = s - lsi[l];
    long W = shapes[2 * l + 1];
    W = W < 1 ? 1 : W;
    const long y = r / W, x = r - y * W;
    const int *e = extents + ((long)b * L + l) * 2;
    QsProposal p;
    p.v[0] = __fdiv_rn((float)x + 0.5f, (float)e[1]);
    p.v[1] = __fdiv_rn((float)y + 0.5f, (float)e[0]);
    p.v[2] = p.v[3] = ldexpf(0.05f, l);
    p.valid = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) p.valid = p.valid && p.v[k] > 0.01f && p.v[k] < 0.99f;
    return p;
}

// ---- enc_output_norm with the zero-fill as a row override (:2273-2275) -------------------------------------------------------------------
// Row groups (row_groups.hpp).  A padded row or one with an invalid proposal takes its chunk from `lin_b`, the bias of the linear in
// front: what that linear gives for a zero row.  In place.
template <int G>
__global__ __launch_bounds__(ROWG_THREADS) void qs_norm_kernel(uint16_t *x, const uint16_t *__restrict__ lin_b, const uint16_t *__restrict__ w,
                                                             const uint16_t *__restrict__ b, const uint8_t *__restrict__ pmask,
                                                             const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
                                                             const int *__restrict__ extents, int L, int S, long rows, int C, float eps)
{
    const RowLanes<G> ln(rows, C);
    const bool act = ln.act;
    const int c0 = ln.c0;
    float gw[8], gb[8];
    load_affine<G>(w, b, ln, gw, gb);
    uint4_t zero_row = {0u, 0u, 0u, 0u};
    if (act) zero_row = *reinterpret_cast<const uint4_t *>(lin_b + c0);
    const float invC = 1.0f / (float)C;
    for (long g = ln.wave0; g < ln.ngroups; g += ln.nwaves) {
        const long row = ln.row(g);
        uint4_t xv = {0u, 0u, 0u, 0u};
        if (act && row < rows) {
            const long bi = row / S;
            const bool filled = pmask[row] != 0 || !qs_proposal(row - bi * S, (int)bi, shapes, lsi, L, extents).valid;
            xv = filled ? zero_row : *reinterpret_cast<const uint4_t *>(x + row * C + c0);
        }
        float v[8];
        unpack8(xv, v);
        const float rstd = layernorm_center<G>(v, act, invC, eps);
        if (act && row < rows) *reinterpret_cast<uint4_t *>(x + row * C + c0) = layernorm_chunk(v, rstd, gw, gb);
    }
}

// ---- scores: row maximum of q . text^T (:1421-1422, :2520), and the same tiles written out for the selected rows (:2532) ----------------
// gfx950, wave64, v_mfma_f32_16x16x32_bf16.  A workgroup belongs to one image: it stages that image's text rows in LDS once ([token][C + 8]
// bf16: the 16-byte pad of mha.hip's K tile) and walks the image's tiles of 128 rows; a wave owns 32 rows, whose q fragments live in
// registers (lane (row l & 15, g = l >> 4) holds q[row][32 c + 8 g .. + 7], the B operand).  The text rows are the A operand, so a lane
// ends up with tokens 4 g + r of its own row: the maximum is taken in the lane, then over the four g.  A text that does not fit the LDS
// budget goes through in chunks of Tc tokens; a later chunk's pass folds the score the same lane stored in the pass before.
// A masked token (and a token from Lt up) counts as -inf; a NaN logit makes the row's score NaN, as torch.max does.
constexpr int RMD_THREADS = 256, RMD_ROWS = 128;
constexpr long RMD_LDS_BUDGET = 144 * 1024;

struct RmdArgs {
    const uint16_t *q;        // [B, S, C] dense rows
    const uint16_t *text;     // [B, Lt, C] dense rows
    const uint8_t *tmask;     // [B, Lt], non-zero = a real token
    float *out;               // scores [B, S], or logits [B, S, ncols]
    int S, Lt, ncols;         // ncols: columns produced (Lt for the scores, max_text_len for the logits)
    int wpi, Tc;              // workgroups per image; tokens per chunk (a multiple of 16)
};

__device__ __forceinline__ float bf16_round(float x) { return bf16_to_f32(f32_to_bf16(x)); }
__device__ __forceinline__ float nan_max(float m, float x) { return (x > m || x != x) ? x : m; }   // (m NaN: stays, unless x is one too)

template <int KS, bool LOGITS>
__global__ __launch_bounds__(RMD_THREADS) void rowmax_dot_kernel(const RmdArgs a)
{
    constexpr int C = KS * 32, LD = C + 8, CPR = C / 8;
    extern __shared__ __attribute__((aligned(16))) uint16_t rmd_lds[];
    uint8_t *dead = reinterpret_cast<uint8_t *>(rmd_lds + (long)a.Tc * LD);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.wpi, wg = blockIdx.x - b * a.wpi;
    const uint16_t *qb = a.q + (long)b * a.S * C;
    const uint16_t *tb = a.text + (long)b * a.Lt * C;
    const uint8_t *tm = a.tmask + (long)b * a.Lt;

    for (int t0 = 0; t0 < a.ncols; t0 += a.Tc) {
        const int tn = a.ncols - t0 < a.Tc ? a.ncols - t0 : a.Tc;
        const int ntile = (tn + 15) >> 4;
        __syncthreads();   // every wave has read the chunk in front
        for (int i = tid; i < ntile * 16 * CPR; i += RMD_THREADS) {
            const int row = i / CPR, ch = i - row * CPR, tok = t0 + row;
            uint4_t v = {0u, 0u, 0u, 0u};
            if (tok < a.Lt) v = *reinterpret_cast<const uint4_t *>(tb + (long)tok * C + ch * 8);
            *reinterpret_cast<uint4_t *>(&rmd_lds[row * LD + ch * 8]) = v;
        }
        for (int i = tid; i < ntile * 16; i += RMD_THREADS) {
            const int tok = t0 + i;
            dead[i] = (uint8_t)(tok >= a.Lt || tm[tok] == 0);
        }
        __syncthreads();

        for (long tile = wg; tile * RMD_ROWS < a.S; tile += a.wpi) {
            const long row0 = tile * RMD_ROWS + wave * 32;
            if (row0 >= a.S) continue;   // (wave-uniform; no barrier inside the walk)
            bf16x8_t qf[2][KS];
            long row[2];
#pragma unroll
            for (int rg = 0; rg < 2; ++rg) {
                row[rg] = row0 + rg * 16 + l15;
                const long rl = row[rg] < a.S ? row[rg] : a.S - 1;   // rows behind S read the last row and are not stored
#pragma unroll
                for (int c = 0; c < KS; ++c) qf[rg][c] = *reinterpret_cast<const bf16x8_t *>(qb + rl * C + 32 * c + 8 * g);
            }
            float m[2] = {-INFINITY, -INFINITY};
            for (int tt = 0; tt < ntile; ++tt) {
                float4_t acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int c = 0; c < KS; ++c) {
                    const bf16x8_t tf = *reinterpret_cast<const bf16x8_t *>(&rmd_lds[(tt * 16 + l15) * LD + 32 * c + 8 * g]);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf, qf[0][c], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tf, qf[1][c], acc[1], 0, 0, 0);
                }
                const uint32_t dw = *reinterpret_cast<const uint32_t *>(&dead[tt * 16 + 4 * g]);
#pragma unroll
                for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float x = ((dw >> (8 * r)) & 0xffu) ? -INFINITY : acc[rg][r];
                        if (LOGITS) {
                            const int tok = t0 + tt * 16 + 4 * g + r;
                            if (row[rg] < a.S && tok < a.ncols) a.out[((long)b * a.S + row[rg]) * a.ncols + tok] = bf16_round(x);
                        } else {
                            m[rg] = nan_max(m[rg], x);
                        }
                    }
            }
            if (!LOGITS) {
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) {
                    float v = m[rg];
                    v = nan_max(v, __shfl_xor(v, 16));
                    v = nan_max(v, __shfl_xor(v, 32));
                    if (g == 0 && row[rg] < a.S) {
                        float *o = a.out + (long)b * a.S + row[rg];
                        v = bf16_round(v);   // (rounding is monotone: the maximum of the rounded logits)
                        if (t0 > 0) v = nan_max(*o, v);
                        *o = v;
                    }
                }
            }
        }
    }
}

struct RmdPlan { int Tc; long lds; };
RmdPlan rmd_plan(int C, int ncols)
{
    const long per = (long)(C + 8) * 2 + 1;
    int Tc = (ncols + 15) / 16 * 16;
    const int cap = (int)(RMD_LDS_BUDGET / per) / 16 * 16;
    if (Tc > cap) Tc = cap;
    return {Tc, ((long)Tc * per + 15) & ~15L};
}

template <int KS, bool LOGITS>
int rmd_launch_ks(const RmdArgs &a, long lds, dim3 grid, hipStream_t st)
{
    static unsigned long long attr_mask = 0;
    if (lds > 48 * 1024 && first_use_on_device(&attr_mask))
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&rowmax_dot_kernel<KS, LOGITS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)RMD_LDS_BUDGET);
    VLLM_LAUNCH((rowmax_dot_kernel<KS, LOGITS>), grid, dim3(RMD_THREADS), (size_t)lds, st, a);
    VLLM_CHECK_LAUNCH("rowmax_dot_kernel");
    return VLLM_OK;
}

// No checks: C a multiple of 64 in 64 .. 512, Lt >= 1, B S > 0, 16-byte aligned q and text.
template <bool LOGITS>
int rmd_launch(const uint16_t *q, const uint16_t *text, const uint8_t *tmask, int B, int S, int Lt, int C, int ncols, float *out, hipStream_t st)
{
    const RmdPlan p = rmd_plan(C, ncols);
    RmdArgs a;
    a.q = q; a.text = text; a.tmask = tmask; a.out = out;
    a.S = S; a.Lt = Lt; a.ncols = ncols; a.Tc = p.Tc;
    const long tiles = ((long)S + RMD_ROWS - 1) / RMD_ROWS;
    long wpi = device_cus() / B;
    wpi = wpi < 1 ? 1 : wpi;
    a.wpi = (int)(tiles < wpi ? tiles : wpi);
    const dim3 grid((unsigned)((long)B * a.wpi));
    switch (C / 64) {
    case 1: return rmd_launch_ks<2, LOGITS>(a, p.lds, grid, st);
    case 2: return rmd_launch_ks<4, LOGITS>(a, p.lds, grid, st);
    case 3: return rmd_launch_ks<6, LOGITS>(a, p.lds, grid, st);
    case 4: return rmd_launch_ks<8, LOGITS>(a, p.lds, grid, st);
    case 5: return rmd_launch_ks<10, LOGITS>(a, p.lds, grid, st);
    case 6: return rmd_launch_ks<12, LOGITS>(a, p.lds, grid, st);
    case 7: return rmd_launch_ks<14, LOGITS>(a, p.lds, grid, st);
    default: return rmd_launch_ks<16, LOGITS>(a, p.lds, grid, st);
    }
}

// ---- top-k per image (:2521) ---------------------------------------------------------------------------------------------------------------
// One workgroup per image.  Order-preserving 32-bit keys (NaN greatest, -0 == +0); a radix select of four 8-bit digits with integer LDS
// histograms finds the key T of the k-th largest; everything above T is collected in whatever order, the ties at T by an index-ordered
// compaction (as many as are still needed, lowest indices first); a bitonic sort of (key, ~index) puts the k survivors in the documented
// order: value descending, ties by ascending index -- torch.sort(descending=True, stable=True).indices[:k].
constexpr int TK_THREADS = 1024, TK_MAX = 2048;

__device__ __forceinline__ uint32_t tk_key(float x)
{
    if (x != x) return 0xffffffffu;
    uint32_t u = __float_as_uint(x);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long tk_item(uint32_t key, uint32_t i) { return ((unsigned long long)key << 32) | (0xffffffffu - i); }
// every thread's keys of one row, TK_UNROLL strided loads in flight at a time -> f(key, index)
constexpr int TK_UNROLL = 8;
template <class F>
__device__ __forceinline__ void tk_scan(const float *__restrict__ sc, int S, int tid, F f)
{
    for (long i0 = tid; i0 < S; i0 += (long)TK_THREADS * TK_UNROLL) {
        float v[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const long i = i0 + (long)u * TK_THREADS;
            v[u] = i < S ? sc[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const long i = i0 + (long)u * TK_THREADS;
            if (i < S) f(tk_key(v[u]), i);
        }
    }
}

__global__ __launch_bounds__(TK_THREADS) void topk_rows_kernel(const float *__restrict__ scores, int S, int k, int64_t *__restrict__ index)
{
    // scores crowd into a few digits (one exponent, one bf16 value): sixteen copies of every counter, one per lane & 15, keep a wave's
    // adds to one digit off one address
    __shared__ uint32_t hist[256], hist16[256 * 16];
    __shared__ uint32_t s_prefix, s_krem, s_cnt, s_wsum[TK_THREADS / 64];
    __shared__ unsigned long long cand[TK_MAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *sc = scores + (long)blockIdx.x * S;

    uint32_t prefix = 0u, mask = 0u, krem = (uint32_t)k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 256 * 16; i += TK_THREADS) hist16[i] = 0u;
        __syncthreads();
        tk_scan(sc, S, tid, [&](uint32_t key, long) {
            if ((key & mask) == prefix) atomicAdd(&hist16[((key >> shift) & 255u) * 16 + (lane & 15)], 1u);
        });
        __syncthreads();
        if (tid < 256) {
            uint32_t n = 0u;
#pragma unroll
            for (int c = 0; c < 16; ++c) n += hist16[tid * 16 + ((c + tid) & 15)];
            hist[tid] = n;
        }
        __syncthreads();
        // hist[d] <- the count of digits >= d
        for (int off = 1; off < 256; off <<= 1) {
            const uint32_t v = (tid + off < 256) ? hist[tid + off] : 0u;
            __syncthreads();
            if (tid < 256) hist[tid] += v;
            __syncthreads();
        }
        if (tid < 256) {
            const uint32_t ge = hist[tid], gt = tid < 255 ? hist[tid + 1] : 0u;
            if (ge >= krem && gt < krem) { s_prefix = prefix | ((uint32_t)tid << shift); s_krem = krem - gt; }   // exactly one digit
        }
        __syncthreads();
        prefix = s_prefix;
        krem = s_krem;
        mask |= 0xffu << shift;
        __syncthreads();
    }
    const uint32_t T = prefix, need = krem, n_gt = (uint32_t)k - krem;

    if (tid == 0) s_cnt = 0u;
    __syncthreads();
    tk_scan(sc, S, tid, [&](uint32_t key, long i) {
        if (key > T) {
            const uint32_t p = atomicAdd(&s_cnt, 1u);
            if (p < n_gt) cand[p] = tk_item(key, (uint32_t)i);
        }
    });
    // the ties in index order: a thread owns TK_UNROLL consecutive indices of a chunk, so an index's rank among the chunk's ties is the
    // ties of the lower waves, of the lower lanes and of the thread's own lower indices
    uint32_t base = 0u;
    for (long i0 = 0; i0 < S && base < need; i0 += (long)TK_THREADS * TK_UNROLL) {
        const long mine = i0 + (long)tid * TK_UNROLL;
        float v[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) v[u] = mine + u < S ? sc[mine + u] : 0.f;
        uint32_t lower = 0u, own = 0u, wtot = 0u;
        bool tie[TK_UNROLL];
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            tie[u] = mine + u < S && tk_key(v[u]) == T;
            const unsigned long long bal = __ballot(tie[u]);
            lower += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            wtot += (uint32_t)__popcll(bal);
        }
        if (lane == 0) s_wsum[wave] = wtot;
        __syncthreads();
        uint32_t before = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < TK_THREADS / 64; ++w) {
            const uint32_t c = s_wsum[w];
            before += w < wave ? c : 0u;
            total += c;
        }
#pragma unroll
        for (int u = 0; u < TK_UNROLL; ++u) {
            const uint32_t rank = base + before + lower + own;
            if (tie[u] && rank < need) cand[n_gt + rank] = tk_item(T, (uint32_t)(mine + u));
            own += tie[u] ? 1u : 0u;
        }
        base += total;
        __syncthreads();
    }
    int n = 1;
    while (n < k) n <<= 1;
    for (int jx = k + tid; jx < n; jx += TK_THREADS) cand[jx] = 0ull;   // below every item: a key is never 0
    __syncthreads();
    for (int sz = 2; sz <= n; sz <<= 1)
        for (int stp = sz >> 1; stp > 0; stp >>= 1) {
            for (int t = tid; t < (n >> 1); t += TK_THREADS) {
                const int i = ((t / stp) * 2 * stp) + (t % stp), jx = i + stp;
                const bool desc = (i & sz) == 0;
                const unsigned long long x = cand[i], y = cand[jx];
                if ((x < y) == desc) { cand[i] = y; cand[jx] = x; }
            }
            __syncthreads();
        }
    for (int jx = tid; jx < k; jx += TK_THREADS)
        index[(long)blockIdx.x * k + jx] = (int64_t)(0xffffffffu - (uint32_t)(cand[jx] & 0xffffffffull));
}

// ---- the selected rows (:2515-2543) ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qs_gather_kernel(const uint16_t *__restrict__ q, const int64_t *__restrict__ topk, uint16_t *__restrict__ target,
                                                        long rows, int k, int S, int C)
{
    const int cpr = C >> 3;
    const long total = rows * cpr, stride = (long)gridDim.x * 256;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const long row = t / cpr;
        const int j = (int)(t - row * cpr);
        const long b = row / k;
        long s = topk[row];
        s = s < 0 ? 0 : s >= S ? S - 1 : s;
        *reinterpret_cast<uint4_t *>(target + row * C + j * 8) = *reinterpret_cast<const uint4_t *>(q + (b * S + s) * C + j * 8);
    }
}

// coords_logits[r, c] = h[r, :] . W[c, :] + bias[c] + log(p / (1 - p)), p = the proposal of the row's index (+inf for a padded row or an
// invalid proposal, the reference's two masked_fill); reference_points = sigmoid of it, so +inf gives 1.0.  fp32; row groups and their
// four fused dot products (row_groups.hpp), as box_refine_kernel (deform_decoder.hip).  valid [rows] (optional): the proposal's validity flag.
template <int G>
__global__ __launch_bounds__(ROWG_THREADS) void qs_tail_kernel(const uint16_t *__restrict__ h, int ldh, const uint16_t *__restrict__ W,
                                                             const uint16_t *__restrict__ bias, const int64_t *__restrict__ topk,
                                                             const uint8_t *__restrict__ pmask, const int64_t *__restrict__ shapes,
                                                             const int64_t *__restrict__ lsi, const int *__restrict__ extents, int L, int S, int k,
                                                             long rows, int C, float *__restrict__ coords, float *__restrict__ refp,
                                                             uint8_t *__restrict__ valid)
{
    const RowLanes<G> ln(rows, C);
    const int j = ln.j;
    const bool fin = j < 4;
    float w[4][8];
    const float bk = load_dot4<G>(W, bias, C, ln, w);
    for (long g = ln.wave0; g < ln.ngroups; g += ln.nwaves) {
        const long row = ln.row(g);
        uint4_t xv = {0u, 0u, 0u, 0u};
        if (ln.act && row < rows) xv = *reinterpret_cast<const uint4_t *>(h + row * ldh + ln.c0);
        float s[4];
        dot4_rows<G>(xv, w, s);
        if (fin && row < rows) {
            const float dot = dot4_pick(s, j);
            const long bi = row / k;
            long idx = topk[row];
            idx = idx < 0 ? 0 : idx >= S ? S - 1 : idx;
            const QsProposal p = qs_proposal(idx, (int)bi, shapes, lsi, L, extents);
            const float pv = j == 0 ? p.v[0] : j == 1 ? p.v[1] : j == 2 ? p.v[2] : p.v[3];
            const bool filled = pmask[bi * S + idx] != 0 || !p.valid;
            const float logit = filled ? INFINITY : logf(__fdiv_rn(pv, 1.f - pv));
            const float z = dot + bk + logit;
            coords[row * 4 + j] = z;
            refp[row * 4 + j] = __fdiv_rn(1.f, 1.f + expf(-z));
            if (valid && j == 0) valid[row] = (uint8_t)p.valid;
        }
    }
}

int extents_launch(const uint8_t *pmask, const int64_t *shapes, const int64_t *lsi, int B, int L, int S, int *extents, hipStream_t st)
{
    VLLM_LAUNCH(qs_extents_kernel, dim3((unsigned)(B * L)), dim3(64), 0, st, pmask, shapes, lsi, L, S, extents);
    VLLM_CHECK_LAUNCH("qs_extents_kernel");
    return VLLM_OK;
}

int norm_launch(uint16_t *x, const uint16_t *lin_b, const uint16_t *w, const uint16_t *b, const uint8_t *pmask, const int64_t *shapes,
                const int64_t *lsi, const int *extents, int L, int S, long rows, int C, float eps, hipStream_t st)
{
    VLLM_LAUNCH_ROW_GROUPS(qs_norm_kernel, rows, C, st, x, lin_b, w, b, pmask, shapes, lsi, extents, L, S, rows, C, eps);
    return VLLM_OK;
}

int topk_launch(const float *scores, int B, int S, int k, int64_t *index, hipStream_t st)
{
    VLLM_LAUNCH(topk_rows_kernel, dim3((unsigned)B), dim3(TK_THREADS), 0, st, scores, S, k, index);
    VLLM_CHECK_LAUNCH("topk_rows_kernel");
    return VLLM_OK;
}

int gather_launch(const uint16_t *q, const int64_t *topk, uint16_t *target, long rows, int k, int S, int C, hipStream_t st)
{
    const long want = (rows * (C / 8) + 255) / 256, cap = (long)device_cus() * 8;
    VLLM_LAUNCH(qs_gather_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, q, topk, target, rows, k, S, C);
    VLLM_CHECK_LAUNCH("qs_gather_kernel");
    return VLLM_OK;
}

int tail_launch(const uint16_t *h, int ldh, const uint16_t *W, const uint16_t *bias, const int64_t *topk, const uint8_t *pmask,
                const int64_t *shapes, const int64_t *lsi, const int *extents, int L, int S, int k, long rows, int C, float *coords, float *refp,
                uint8_t *valid, hipStream_t st)
{
    VLLM_LAUNCH_ROW_GROUPS(qs_tail_kernel, rows, C, st, h, ldh, W, bias, topk, pmask, shapes, lsi, extents, L, S, k, rows, C, coords, refp, valid);
    return VLLM_OK;
}

struct QsWs { long extents, q, scores, t1, t2, total; };
QsWs qs_ws(const VllmQuerySelectDesc *d, long B, long S, long k)
{
    const long C = d->d_model;
    Carver cv;
    QsWs w;
    w.extents = cv.take(B * d->n_levels * 2 * 4);
    w.q = cv.take(B * S * C * 2);
    w.scores = cv.take(B * S * 4);
    w.t1 = cv.take(B * k * C * 2);
    w.t2 = cv.take(B * k * C * 2);
    w.total = cv.off;
    return w;
}

int qs_check_desc(const VllmQuerySelectDesc *d)
{
    VLLM_REQUIRE(d, "query_select: null descriptor");
    VLLM_REQUIRE(d->d_model >= 64 && d->d_model <= 512 && d->d_model % 64 == 0, "query_select: d_model=%d (a multiple of 64 in 64 .. 512)", d->d_model);
    VLLM_REQUIRE(d->max_text_len >= 1 && d->max_text_len <= 256, "query_select: max_text_len=%d (1 .. 256)", d->max_text_len);
    VLLM_REQUIRE(d->n_levels >= 1 && d->n_levels <= QS_MAX_LEVELS, "query_select: n_levels=%d (1 .. %d)", d->n_levels, QS_MAX_LEVELS);
    VLLM_REQUIRE(d->layer_norm_eps >= 0.f, "query_select: negative eps");
    const VllmBoxHead &bh = d->box_head;
    VLLM_REQUIRE(d->enc_output_w && d->enc_output_b && d->enc_output_norm_w && d->enc_output_norm_b && bh.w0 && bh.b0 && bh.w1 && bh.b1 && bh.w2 &&
                     bh.b2,
                 "query_select: missing weights (enc_output / enc_output_norm / box head)");
    return VLLM_OK;
}

int qs_check_sizes(const VllmQuerySelectDesc *d, int B, int S, int Lt, int k)
{
    VLLM_REQUIRE(B >= 0 && S >= 0 && k >= 0, "query_select: B=%d S=%d k=%d (not negative)", B, S, k);
    if ((long)B * k == 0) return VLLM_OK;
    VLLM_REQUIRE(Lt >= 1 && Lt <= d->max_text_len, "query_select: Lt=%d (1 .. max_text_len=%d)", Lt, d->max_text_len);
    VLLM_REQUIRE(k <= S && k <= TK_MAX, "query_select: k=%d (1 .. min(S=%d, %d))", k, S, TK_MAX);
    // (the GEMMs address an operand with 32-bit byte offsets)
    VLLM_REQUIRE((long)B * S * d->d_model * 2 < (1L << 31), "query_select: B S=%ld rows of d_model=%d reach 2^31 bytes", (long)B * S, d->d_model);
    return VLLM_OK;
}

long g_calls = 0;

}  // namespace
}  // namespace vllm

using namespace vllm;

extern "C" unsigned long vllm_query_select_desc_sizeof(void) { return sizeof(VllmQuerySelectDesc); }
extern "C" long vllm_query_select_calls(void) { return g_calls; }

extern "C" long vllm_query_select_workspace_bytes(const VllmQuerySelectDesc *d, int B, int S, int Lt, int k)
{
    if (qs_check_desc(d) != VLLM_OK || qs_check_sizes(d, B, S, Lt, k) != VLLM_OK) return -1;
    if ((long)B * k == 0) return 0;
    return qs_ws(d, B, S, k).total;
}

extern "C" int vllm_rowmax_dot_bf16(const uint16_t *q, const uint16_t *text, const uint8_t *text_token_mask, int B, int S, int Lt, int C,
                                    float *scores, vllm_stream_t stream)
{
    VLLM_REQUIRE(C >= 64 && C <= 512 && C % 64 == 0, "rowmax_dot: C=%d (a multiple of 64 in 64 .. 512)", C);
    VLLM_REQUIRE(B >= 0 && S >= 0, "rowmax_dot: B=%d S=%d (not negative)", B, S);
    if ((long)B * S == 0) return VLLM_OK;
    VLLM_REQUIRE(Lt >= 1 && Lt <= 256, "rowmax_dot: Lt=%d (1 .. 256)", Lt);
    VLLM_REQUIRE(q && text && text_token_mask && scores, "rowmax_dot: null pointer");
    VLLM_REQUIRE(aligned16(q) && aligned16(text) && ((uintptr_t)scores & 3u) == 0, "rowmax_dot: misaligned operand (q, text 16 bytes; scores 4)");
    VLLM_REQUIRE(!ranges_overlap(scores, (long)B * S * 4, q, (long)B * S * C * 2) && !ranges_overlap(scores, (long)B * S * 4, text, (long)B * Lt * C * 2) &&
                     !ranges_overlap(scores, (long)B * S * 4, text_token_mask, (long)B * Lt),
                 "rowmax_dot: scores overlaps an input");
    return rmd_launch<false>(q, text, text_token_mask, B, S, Lt, C, Lt, scores, (hipStream_t)stream);
}

extern "C" int vllm_topk_rows_f32(const float *scores, int B, int S, int k, int64_t *index, vllm_stream_t stream)
{
    VLLM_REQUIRE(B >= 0 && S >= 0 && k >= 0, "topk_rows: B=%d S=%d k=%d (not negative)", B, S, k);
    if ((long)B * k == 0) return VLLM_OK;
    VLLM_REQUIRE(k <= S && k <= TK_MAX, "topk_rows: k=%d (1 .. min(S=%d, %d))", k, S, TK_MAX);
    VLLM_REQUIRE(scores && index, "topk_rows: null pointer");
    VLLM_REQUIRE(((uintptr_t)scores & 3u) == 0 && aligned8(index), "topk_rows: misaligned operand (scores 4 bytes, index 8)");
    VLLM_REQUIRE(!ranges_overlap(index, (long)B * k * 8, scores, (long)B * S * 4), "topk_rows: index overlaps scores");
    return topk_launch(scores, B, S, k, index, (hipStream_t)stream);
}

extern "C" int vllm_query_select_tail_f32(const uint16_t *h, int ldh, const uint16_t *W, const uint16_t *b, const int64_t *topk_index,
                                          const uint8_t *padding_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B,
                                          int S, int L, int k, int C, int32_t *extents, float *coords_logits, float *reference_points,
                                          uint8_t *valid, vllm_stream_t stream)
{
    VLLM_REQUIRE(C >= 64 && C <= 512 && C % 64 == 0, "query_select_tail: C=%d (a multiple of 64 in 64 .. 512)", C);
    VLLM_REQUIRE(B >= 0 && B < (1 << 24) && S >= 0 && k >= 0 && L >= 1 && L <= QS_MAX_LEVELS,
                 "query_select_tail: B=%d S=%d k=%d L=%d (B under 2^24, L in 1 .. %d)", B, S, k, L, QS_MAX_LEVELS);
    if ((long)B * k == 0) return VLLM_OK;
    VLLM_REQUIRE(S >= 1, "query_select_tail: S=%d with rows selected", S);
    VLLM_REQUIRE(h && W && b && topk_index && padding_mask && spatial_shapes && level_start_index && extents && coords_logits && reference_points,
                 "query_select_tail: null pointer");
    VLLM_REQUIRE(aligned16(h) && ldh >= C && ldh % 8 == 0 && aligned16(W) && aligned8(b) && aligned8(topk_index) && aligned8(spatial_shapes) &&
                     aligned8(level_start_index) && ((uintptr_t)extents & 3u) == 0 && aligned16(coords_logits) && aligned16(reference_points),
                 "query_select_tail: misaligned operand (16 bytes; b and the int64 tensors 8; extents 4) or ldh=%d (a multiple of 8, at least C)", ldh);
    const long R = (long)B * k;
    VLLM_REQUIRE(!ranges_overlap(coords_logits, R * 16, reference_points, R * 16) && !ranges_overlap(coords_logits, R * 16, extents, (long)B * L * 8) &&
                     !ranges_overlap(reference_points, R * 16, extents, (long)B * L * 8),
                 "query_select_tail: outputs overlap");
    hipStream_t st = (hipStream_t)stream;
    TRY(extents_launch(padding_mask, spatial_shapes, level_start_index, B, L, S, extents, st));
    return tail_launch(h, ldh, W, b, topk_index, padding_mask, spatial_shapes, level_start_index, extents, L, S, k, R, C, coords_logits,
                       reference_points, valid, st);
}

extern "C" int vllm_query_select_forward(const VllmQuerySelectDesc *d, const uint16_t *memory, const uint8_t *padding_mask, const uint16_t *text,
                                         const uint8_t *text_token_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B,
                                         int S, int Lt, int k, int64_t *topk_index, uint16_t *target, float *coords_logits, float *reference_points,
                                         float *class_logits, float *scores, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    TRY(qs_check_desc(d));
    TRY(qs_check_sizes(d, B, S, Lt, k));
    if ((long)B * k == 0) return VLLM_OK;
    const int C = d->d_model, L = d->n_levels, MTL = d->max_text_len;
    const long R = (long)B * k, RS = (long)B * S;
    const VllmBoxHead &bh = d->box_head;
    VLLM_REQUIRE(memory && padding_mask && text && text_token_mask && spatial_shapes && level_start_index && topk_index && target && coords_logits &&
                     reference_points && class_logits,
                 "query_select: null pointer (memory / padding_mask / text / text_token_mask / spatial_shapes / level_start_index / an output)");
    VLLM_REQUIRE(aligned16(memory) && aligned16(text) && aligned8(spatial_shapes) && aligned8(level_start_index) && aligned8(topk_index) &&
                     aligned16(target) && aligned16(coords_logits) && aligned16(reference_points) && ((uintptr_t)class_logits & 3u) == 0 &&
                     ((uintptr_t)scores & 3u) == 0,
                 "query_select: misaligned memory / text / target / coords_logits / reference_points (16 bytes), spatial_shapes / level_start_index / "
                 "topk_index (8) or class_logits / scores (4)");
    for (const uint16_t *p : {d->enc_output_w, d->enc_output_b, d->enc_output_norm_w, d->enc_output_norm_b, bh.w0, bh.b0, bh.w1, bh.b1, bh.w2})
        VLLM_REQUIRE(aligned16(p), "query_select: misaligned weight or bias (16 bytes; the box head's last bias 8)");
    VLLM_REQUIRE(aligned8(bh.b2), "query_select: misaligned weight or bias (16 bytes; the box head's last bias 8)");
    const struct { const void *p; long bytes; } outs[] = {{topk_index, R * 8}, {target, R * C * 2}, {coords_logits, R * 16}, {reference_points, R * 16},
                                                          {class_logits, R * MTL * 4}, {scores, RS * 4}},
                                                ins[] = {{memory, RS * C * 2}, {padding_mask, RS}, {text, (long)B * Lt * C * 2},
                                                         {text_token_mask, (long)B * Lt}, {spatial_shapes, (long)L * 16}, {level_start_index, (long)L * 8}};
    for (int i = 0; i < 6; ++i) {
        for (const auto &in : ins)
            VLLM_REQUIRE(!ranges_overlap(outs[i].p, outs[i].bytes, in.p, in.bytes), "query_select: an output overlaps an input");
        for (int o = i + 1; o < 6; ++o)
            VLLM_REQUIRE(!ranges_overlap(outs[i].p, outs[i].bytes, outs[o].p, outs[o].bytes), "query_select: two outputs overlap");
    }
    const QsWs w = qs_ws(d, B, S, k);
    VLLM_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.total, "query_select: workspace too small (%ld < %ld bytes) or misaligned",
                 workspace_bytes, w.total);
    for (int i = 0; i < 6; ++i)
        VLLM_REQUIRE(!ranges_overlap(outs[i].p, outs[i].bytes, workspace, w.total), "query_select: an output overlaps the workspace");
    char *ws = (char *)workspace;
    int *extents = (int *)(ws + w.extents);
    uint16_t *q = (uint16_t *)(ws + w.q), *t1 = (uint16_t *)(ws + w.t1), *t2 = (uint16_t *)(ws + w.t2);
    float *sc = scores ? scores : (float *)(ws + w.scores);
    ++g_calls;
    hipStream_t st = (hipStream_t)stream;

    TRY(extents_launch(padding_mask, spatial_shapes, level_start_index, B, L, S, extents, st));
    // :2275 on the raw rows; the zero-filled rows are put right at the norm's load
    TRY(gemm(st, EPI_BIAS, memory, C, d->enc_output_w, C, d->enc_output_b, q, C, (int)RS, C, C));
    TRY(norm_launch(q, d->enc_output_b, d->enc_output_norm_w, d->enc_output_norm_b, padding_mask, spatial_shapes, level_start_index, extents, L, S, RS, C,
                    d->layer_norm_eps, st));
    // :2511-2521
    TRY(rmd_launch<false>(q, text, text_token_mask, B, S, Lt, C, Lt, sc, st));
    TRY(topk_launch(sc, B, S, k, topk_index, st));
    // :2515-2543 on the selected rows
    TRY(gather_launch(q, topk_index, target, R, k, S, C, st));
    TRY(gemm(st, EPI_RELU, target, C, bh.w0, C, bh.b0, t1, C, (int)R, C, C));
    TRY(gemm(st, EPI_RELU, t1, C, bh.w1, C, bh.b1, t2, C, (int)R, C, C));
    TRY(tail_launch(t2, C, bh.w2, bh.b2, topk_index, padding_mask, spatial_shapes, level_start_index, extents, L, S, k, R, C, coords_logits,
                    reference_points, nullptr, st));
    return rmd_launch<true>(target, text, text_token_mask, B, k, Lt, C, MTL, class_logits, st);
}
