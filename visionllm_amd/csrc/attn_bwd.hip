// Flash-style backward of the dense, non-causal, packed-qkv attention of attn.hip: grad_qkv from qkv, the saved (rounded) out, the
// forward's row log-sum-exp and grad_out.  bf16 or IEEE half in / out, fp32 accumulation.
//
// Replaces the backward of flash_attn_varlen_qkvpacked_func (VisionLLMv2/visionllmv2/model/internvit/flash_attention.py:30-75,
// an autograd function in the reference) and of InternAttention._naive_attn's statements (modeling_intern_vit.py:136-140).
//
//   p_ij = exp(scale q_i.k_j - lse_i)      delta_i = sum_d dO_id O_id      dV_j = sum_i p_ij dO_i
//   dS_ij = p_ij (dO_i.v_j - delta_i)      dQ_i = scale sum_j dS_ij k_j    dK_j = scale sum_i dS_ij q_i
//
// Two kernels, seven MFMA products (14 B H S^2 D FLOPs), every output element owned by exactly one wave: no atomics, no
// workgroup waits on another, the caller does no zero-fill, the bits are the same on every run.
//   * attn_bwd_dq_kernel owns 128 query rows per block (32 per wave, Q and dO in registers as B operands) and sweeps 64-key tiles
//     of K and V through the forward's LDS-DMA ring.  Scores are computed transposed as in the forward (S^T = K Q^T, dP^T = V dO^T:
//     the query is on the lane, so lse_i and delta_i are per-lane scalars), dS^T is rounded in place into the B operand of
//     dQ^T += K^T dS^T, and K^T comes from the same LDS image by the hardware transpose read.  It also computes delta for its rows
//     and leaves it in the workspace ([B, H, S] fp32) for the second kernel, which is why it runs first.
//   * attn_bwd_dkv_kernel owns 128 key rows per block (K and V in registers) and sweeps 64-query tiles of Q and dO: S = Q K^T and
//     dP = dO V^T have the KEY on the lane, so their accumulators (dP starts at -delta) are already the B operands of
//     dV^T += dO^T P and dK^T += Q^T dS; Q^T and dO^T are transpose reads of the one LDS image each tile has.
// Rows past S: a ragged tile re-reads row S-1 (finite values) and is then taken out exactly -- keys >= S get dS = 0 in the dQ kernel,
// queries >= S get lse = +1e30 (p = 0, dS = 0) in the dK/dV kernel; padded rows a wave owns are computed and not stored.
// The forward's class-token split is a forward optimisation: S = 64 n + 1 is tiled plainly here.
#include <type_traits>
#include "common.hpp"
#include "kernels.hpp"
#include "attn_common.hpp"

namespace vllm {

struct AttnBwdArgs {
    const uint16_t *qkv, *out, *dout;   // [B, S, 3, H, D], [B, S, H, D], [B, S, H, D]
    const float *lse;                   // [B, H, S]
    float *delta;                       // [B, H, S] (workspace)
    uint16_t *dqkv;                     // [B, S, 3, H, D]
    int B, S, H;
    int nt;                             // 128-row tiles per (b, h)
    float scale, scale_log2e;
};

constexpr float LOG2E = 1.4426950408889634f;
// IEEE half only: P and dS enter their MFMAs times a power of two (exact; taken out again in the one multiply of the epilogue), so
// that a probability of e^-18 -- the class token far below every score -- is a NORMAL half instead of a subnormal with 2^-25 of
// absolute error per term: summed over S queries that error is several spacings of a dV / dK row that is itself that small.
// P <= 1 (+ 2^-11) by construction, so 2^14 cannot overflow; dS gets 2^4 (|dS| up to 4094 before half's infinity).  bf16 has
// fp32's exponent range and needs neither.
constexpr int P_EXP = 14, DS_EXP = 4;

// Both kernels keep every LDS tile (64 rows x D) in the K swizzle of attn_common.hpp (stage_kv<D, false>) and read it two ways.
// By rows (A operand, row on the lane): 16 bytes of row l31, chunk 2 ks + hh -- attn.hip's kofs.
template <int D> __device__ __forceinline__ int row_frag_ofs(int l31, int hh, int ks)
{
    return l31 * (D * 2) + (((2 * ks + hh) ^ swz_k<D>(l31)) << 4);
}
// By columns (A operand of a product that sums over the tile's rows, column on the lane): ds_read_b64_tr_b16 with attn.hip's lane
// pattern (lane = (hh, g1, i16): row 4 hh + i16 / 4 (+ 8 for the high half), columns 32 d + 16 g1 + 4 (i16 & 3) .. + 3), under the K
// swizzle, which looks at row bits 0-3 only: the row blocks 16 u and 32 kb stay immediates, the + 8 of the high half does not.
template <int D> __device__ __forceinline__ int tr_frag_ofs(int lane, int d, int hi)
{
    const int i16 = lane & 15, row = 4 * (lane >> 5) + (i16 >> 2) + 8 * hi;
    const int c = d * 4 + 2 * ((lane >> 4) & 1) + ((i16 & 3) >> 1);
    return row * (D * 2) + ((c ^ swz_k<D>(row)) << 4) + ((i16 & 1) << 3);
}
__device__ __forceinline__ bf16x8_t lds_row_frag(uint32_t addr)
{
    return *(const __attribute__((address_space(3))) bf16x8_t *)(uintptr_t)addr;
}
__device__ __forceinline__ bf16x8_t lds_tr_frag(uint32_t lo, uint32_t hi)
{
    const s16x4_t a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t *)(uintptr_t)lo);
    const s16x4_t b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t *)(uintptr_t)hi);
    return bf16x8_t{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
__device__ __forceinline__ bf16x8_t pack_frag(const uint32_t (&pk)[8], int u)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 w = {pk[4 * u], pk[4 * u + 1], pk[4 * u + 2], pk[4 * u + 3]};
    return __builtin_bit_cast(bf16x8_t, w);
}
// One wave's 32 x D gradient rows, 8 bytes per lane and instruction from the accumulator layout (lane holds columns
// 32 d + 8 rq + 4 hh + 0..3 of row l31), each element rounded once.
template <int D, bool F16>
__device__ __forceinline__ void store_rows(uint16_t *row, const f32x16_t (&acc)[D / 32], float mul, int hh)
{
#pragma unroll
    for (int d = 0; d < D / 32; ++d)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            uint2_t w;
            w.x = pack16x2<F16>(acc[d][4 * rq] * mul, acc[d][4 * rq + 1] * mul);
            w.y = pack16x2<F16>(acc[d][4 * rq + 2] * mul, acc[d][4 * rq + 3] * mul);
            *reinterpret_cast<uint2_t *>(row + d * 32 + 8 * rq + 4 * hh) = w;
        }
}

template <int D, bool F16>
__global__ __launch_bounds__(ATT_THREADS, 2) void attn_bwd_dq_kernel(const AttnBwdArgs a)
{
    constexpr int KS = D / 16, DB = D / 32, TILE = KVBLK * D * 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][K | V]

    if ((uint32_t)(uintptr_t)smem != 0u) __builtin_trap();   // fragment reads address LDS by byte offset: no static LDS here
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int l31 = lane & 31, hh = lane >> 5;

    const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3;   // all query blocks of a (b, head) on one XCD, as in the forward
    const int bh = (sidx / a.nt) * 8 + xcd;
    const int qt = sidx % a.nt;
    if (bh >= a.B * a.H) return;
    const int b = bh / a.H, head = bh % a.H;
    const long C = (long)a.H * D;
    const int ts = (int)(3 * C);
    const uint16_t *qb = a.qkv + (long)b * a.S * 3 * C + (long)head * D;
    const uint16_t *kb_ = qb + C, *vb_ = qb + 2 * C;

    uint32_t kvo[KvStage<D>::NI];   // K and V: same token stride, same swizzle
    kv_lane_offsets<D, false>(ts, wave, lane, kvo);

    // ---- this lane's query: Q and dO fragments (B operands), delta, lse ----
    const int q_row = qt * QBLK + wave * 32 + l31;
    const int q_ld = q_row < a.S ? q_row : a.S - 1;
    const long orow = (((long)b * a.S + q_ld) * a.H + head) * D;
    bf16x8_t qf[KS], dof[KS];
    float dacc = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = *reinterpret_cast<const bf16x8_t *>(qb + (long)q_ld * ts + ks * 16 + hh * 8);
        dof[ks] = *reinterpret_cast<const bf16x8_t *>(a.dout + orow + ks * 16 + hh * 8);
        const uint4_t oo = *reinterpret_cast<const uint4_t *>(a.out + orow + ks * 16 + hh * 8);
        const uint4_t gg = __builtin_bit_cast(uint4_t, dof[ks]);
        dacc = dot2_acc<F16>(gg.x, oo.x, dacc);
        dacc = dot2_acc<F16>(gg.y, oo.y, dacc);
        dacc = dot2_acc<F16>(gg.z, oo.z, dacc);
        dacc = dot2_acc<F16>(gg.w, oo.w, dacc);
    }
    const float delta = halves_sum(dacc);
    const long srow = ((long)b * a.H + head) * a.S;
    if (hh == 0 && q_row < a.S) a.delta[srow + q_row] = delta;
    const float lse2 = a.lse[srow + q_ld] * LOG2E - (F16 ? (float)DS_EXP : 0.f);   // half: p below is 2^DS_EXP p (only dS uses it)
    const float c2 = a.scale_log2e;

    f32x16_t dq[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[d][r] = 0.f;

    int rofs[KS], tofs[DB][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) rofs[ks] = row_frag_ofs<D>(l31, hh, ks);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        tofs[d][0] = tr_frag_ofs<D>(lane, d, 0);
        tofs[d][1] = tr_frag_ofs<D>(lane, d, 1);
    }

    const int nkt = (a.S + KVBLK - 1) / KVBLK;
    const bool live_wave = qt * QBLK + wave * 32 < a.S;   // waves whose 32 query rows are all padding only stage and synchronise
    stage_kv<D, false>(kb_, ts, 0, a.S, smem, wave, lane, kvo);
    stage_kv<D, false>(vb_, ts, 0, a.S, smem + TILE, wave, lane, kvo);
    for (int t = 0; t < nkt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // tile t landed for every wave; everyone is done reading the other stage
        const uint32_t ks_ = (uint32_t)((t & 1) * 2 * TILE), vs_ = ks_ + TILE;
        if (t + 1 < nkt) {
            char *nx = smem + ((t & 1) ^ 1) * 2 * TILE;
            stage_kv<D, false>(kb_, ts, (t + 1) * KVBLK, a.S, nx, wave, lane, kvo);
            stage_kv<D, false>(vb_, ts, (t + 1) * KVBLK, a.S, nx + TILE, wave, lane, kvo);
        }
        if (!live_wave) continue;
        const int nkb = t * KVBLK + 32 < a.S ? 2 : 1;   // a last tile of <= 32 live keys: second key block skipped
        for (int kb = 0; kb < nkb; ++kb) {
            const uint32_t rb = kb * 32 * (D * 2);
            // S^T = K Q^T and dP^T - delta = V dO^T - delta: lane holds keys kb*32 + (r&3) + 8*(r>>2) + 4*hh of query l31
            f32x16_t st, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = -delta; }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) st = mfma16<F16>(lds_row_frag(ks_ + rb + rofs[ks]), qf[ks], st);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) dp = mfma16<F16>(lds_row_frag(vs_ + rb + rofs[ks]), dof[ks], dp);
            uint32_t pk[8];
            const int key0 = t * KVBLK + kb * 32 + 4 * hh;
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int key = key0 + (r & 3) + 8 * (r >> 2);
                const float p0 = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -lse2));
                const float p1 = __builtin_amdgcn_exp2f(fmaf(st[r + 1], c2, -lse2));
                const float s0 = key < a.S ? p0 * dp[r] : 0.f;
                const float s1 = key + 1 < a.S ? p1 * dp[r + 1] : 0.f;
                pk[r >> 1] = pack16x2<F16>(s0, s1);
            }
            // dQ^T += K^T dS^T ; k-slots of step u: regs 8u..8u+7 <-> keys 32kb + 16u + 4hh + {0..3, 8..11}
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bf16x8_t sf = pack_frag(pk, u);
                const uint32_t blk = ks_ + rb + 16 * u * (D * 2);
#pragma unroll
                for (int d = 0; d < DB; ++d) dq[d] = mfma16<F16>(lds_tr_frag(blk + tofs[d][0], blk + tofs[d][1]), sf, dq[d]);
            }
        }
    }
    if (q_row < a.S)
        store_rows<D, F16>(a.dqkv + ((long)b * a.S + q_row) * 3 * C + (long)head * D, dq, a.scale * (F16 ? 1.0f / (1 << DS_EXP) : 1.0f), hh);
}

template <int D, bool F16>
__global__ __launch_bounds__(ATT_THREADS, D == 64 ? 2 : 1) void attn_bwd_dkv_kernel(const AttnBwdArgs a)
{
    constexpr int KS = D / 16, DB = D / 32, TILE = KVBLK * D * 2;
    constexpr int STATS = 4 * TILE;   // behind the ring: [2 stages][lse * log2e : 64 | delta : 64] fp32
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][Q | dO], then the row statistics

    if ((uint32_t)(uintptr_t)smem != 0u) __builtin_trap();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int l31 = lane & 31, hh = lane >> 5;

    const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3;
    const int bh = (sidx / a.nt) * 8 + xcd;
    const int kt = sidx % a.nt;
    if (bh >= a.B * a.H) return;
    const int b = bh / a.H, head = bh % a.H;
    const long C = (long)a.H * D;
    const int ts = (int)(3 * C), ots = (int)C;
    const uint16_t *qb = a.qkv + (long)b * a.S * 3 * C + (long)head * D;
    const uint16_t *ob = a.dout + (long)b * a.S * C + (long)head * D;
    const long srow = ((long)b * a.H + head) * a.S;

    uint32_t qvo[KvStage<D>::NI], ovo[KvStage<D>::NI];
    kv_lane_offsets<D, false>(ts, wave, lane, qvo);
    kv_lane_offsets<D, false>(ots, wave, lane, ovo);

    // ---- this lane's key: K and V fragments (B operands) ----
    const int k_row = kt * QBLK + wave * 32 + l31;
    const int k_ld = k_row < a.S ? k_row : a.S - 1;
    bf16x8_t kf[KS], vf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        kf[ks] = *reinterpret_cast<const bf16x8_t *>(qb + C + (long)k_ld * ts + ks * 16 + hh * 8);
        vf[ks] = *reinterpret_cast<const bf16x8_t *>(qb + 2 * C + (long)k_ld * ts + ks * 16 + hh * 8);
    }
    f32x16_t dk[DB], dv[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[d][r] = 0.f; dv[d][r] = 0.f; }

    int rofs[KS], tofs[DB][2];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) rofs[ks] = row_frag_ofs<D>(l31, hh, ks);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        tofs[d][0] = tr_frag_ofs<D>(lane, d, 0);
        tofs[d][1] = tr_frag_ofs<D>(lane, d, 1);
    }
    const float c2 = a.scale_log2e;

    // Row statistics of a query tile: threads 0..63 fetch lse, 64..127 delta; a query past S gets lse = +1e30 (p = 0 exactly) and
    // delta = 0.  Fetched while tile t is computed, written to the other stage's slot behind the compute.
    const int tid = threadIdx.x;
    auto fetch_stat = [&](int q0) -> float {
        const int q = q0 + (tid & 63);
        if (tid >= 128) return 0.f;
        if (q >= a.S) return tid < 64 ? 1.0e30f : 0.f;
        return tid < 64 ? a.lse[srow + q] * LOG2E - (F16 ? (float)P_EXP : 0.f) : a.delta[srow + q];   // half: p below is 2^P_EXP p
    };
    auto put_stat = [&](int slot, float v) {
        if (tid < 128) *reinterpret_cast<float *>(smem + STATS + slot * 512 + tid * 4) = v;
    };

    const int nqt = (a.S + KVBLK - 1) / KVBLK;
    const bool live_wave = kt * QBLK + wave * 32 < a.S;
    stage_kv<D, false>(qb, ts, 0, a.S, smem, wave, lane, qvo);
    stage_kv<D, false>(ob, ots, 0, a.S, smem + TILE, wave, lane, ovo);
    put_stat(0, fetch_stat(0));
    for (int t = 0; t < nqt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();   // tile t and its statistics are there for every wave; everyone is done reading the other stage
        const int slot = t & 1;
        const uint32_t qs_ = (uint32_t)(slot * 2 * TILE), os_ = qs_ + TILE;
        const bool more = t + 1 < nqt;
        float nstat = 0.f;
        if (more) {
            char *nx = smem + (slot ^ 1) * 2 * TILE;
            stage_kv<D, false>(qb, ts, (t + 1) * KVBLK, a.S, nx, wave, lane, qvo);
            stage_kv<D, false>(ob, ots, (t + 1) * KVBLK, a.S, nx + TILE, wave, lane, ovo);
            nstat = fetch_stat((t + 1) * KVBLK);
        }
        if (live_wave) {
            const int nqb = t * KVBLK + 32 < a.S ? 2 : 1;   // a last tile of <= 32 live queries: second block skipped
            for (int qk = 0; qk < nqb; ++qk) {
                const uint32_t rb = qk * 32 * (D * 2);
                // lane holds queries qk*32 + (r&3) + 8*(r>>2) + 4*hh of key l31: four consecutive queries per 16-byte read
                const uint32_t sbase = (uint32_t)(STATS + slot * 512 + (qk * 32 + 4 * hh) * 4);
                f32x16_t st, dp;
                float ls[16];
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const float4_t l4 = *(const __attribute__((address_space(3))) float4_t *)(uintptr_t)(sbase + rq * 32);
                    const float4_t d4 = *(const __attribute__((address_space(3))) float4_t *)(uintptr_t)(sbase + 256 + rq * 32);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        ls[4 * rq + i] = l4[i];
                        dp[4 * rq + i] = -d4[i];
                        st[4 * rq + i] = 0.f;
                    }
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) st = mfma16<F16>(lds_row_frag(qs_ + rb + rofs[ks]), kf[ks], st);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) dp = mfma16<F16>(lds_row_frag(os_ + rb + rofs[ks]), vf[ks], dp);
                uint32_t pp[8], pd[8];
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const float p0 = __builtin_amdgcn_exp2f(fmaf(st[r], c2, -ls[r]));
                    const float p1 = __builtin_amdgcn_exp2f(fmaf(st[r + 1], c2, -ls[r + 1]));
                    pp[r >> 1] = pack16x2<F16>(p0, p1);
                    constexpr float DSM = F16 ? 1.0f / (1 << (P_EXP - DS_EXP)) : 1.0f;
                    pd[r >> 1] = pack16x2<F16>(p0 * (dp[r] * DSM), p1 * (dp[r + 1] * DSM));
                }
                // dV^T += dO^T P and dK^T += Q^T dS ; k-slots of step u: regs 8u..8u+7 <-> queries 32qk + 16u + 4hh + {0..3, 8..11}
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bf16x8_t pf = pack_frag(pp, u), sf = pack_frag(pd, u);
                    const uint32_t qblk = qs_ + rb + 16 * u * (D * 2), oblk = os_ + rb + 16 * u * (D * 2);
#pragma unroll
                    for (int d = 0; d < DB; ++d) {
                        dv[d] = mfma16<F16>(lds_tr_frag(oblk + tofs[d][0], oblk + tofs[d][1]), pf, dv[d]);
                        dk[d] = mfma16<F16>(lds_tr_frag(qblk + tofs[d][0], qblk + tofs[d][1]), sf, dk[d]);
                    }
                }
            }
        }
        if (more) put_stat(slot ^ 1, nstat);
    }
    if (k_row < a.S) {
        uint16_t *row = a.dqkv + ((long)b * a.S + k_row) * 3 * C + (long)head * D;
        store_rows<D, F16>(row + C, dk, a.scale * (F16 ? 1.0f / (1 << DS_EXP) : 1.0f), hh);
        store_rows<D, F16>(row + 2 * C, dv, F16 ? 1.0f / (1 << P_EXP) : 1.0f, hh);
    }
}

static long attn_bwd_workspace(int B, int S, int H, int D)
{
    if ((D != 64 && D != 128) || B < 0 || S <= 0 || H <= 0) return -1;
    return (((long)B * H * S * 4) + 255) / 256 * 256;   // delta [B, H, S] fp32
}

template <int D, bool F16>
static void attn_bwd_launch_one(const AttnBwdArgs &a, unsigned grid, hipStream_t st)
{
    constexpr size_t lds_dq = 4 * (size_t)KVBLK * D * 2, lds_dkv = lds_dq + 1024;
    if constexpr (lds_dkv > 65536) {
        static unsigned long long attr_mask = 0;
        if (first_use_on_device(&attr_mask))
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&attn_bwd_dkv_kernel<D, F16>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dkv);
    }
    VLLM_LAUNCH((attn_bwd_dq_kernel<D, F16>), dim3(grid), dim3(ATT_THREADS), lds_dq, st, a);
    VLLM_LAUNCH((attn_bwd_dkv_kernel<D, F16>), dim3(grid), dim3(ATT_THREADS), lds_dkv, st, a);
}

int attn_bwd_launch(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *grad_out, int B, int S, int H, int D,
                    float softmax_scale, uint16_t *grad_qkv, void *workspace, long workspace_bytes, bool f16, hipStream_t st)
{
    VLLM_REQUIRE(B >= 0 && S > 0 && H > 0, "attn_bwd: bad dims B=%d S=%d H=%d", B, S, H);
    VLLM_REQUIRE(D == 64 || D == 128, "attn_bwd: head_dim %d not supported (64 or 128)", D);
    if (B == 0) return VLLM_OK;
    const long need = attn_bwd_workspace(B, S, H, D);
    VLLM_REQUIRE((long)H * D < (1l << 22), "attn_bwd: H * D too large for 32-bit tile offsets");
    VLLM_REQUIRE(qkv && out && lse && grad_out && grad_qkv && workspace, "attn_bwd: null pointer (an operand or the workspace)");
    VLLM_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(grad_out) && aligned16(grad_qkv) && aligned16(workspace) &&
                     (reinterpret_cast<uintptr_t>(lse) & 3u) == 0,
                 "attn_bwd: qkv, out, grad_out, grad_qkv and workspace must be 16-byte aligned, lse 4-byte aligned");
    VLLM_REQUIRE(workspace_bytes >= need, "attn_bwd: workspace %ld bytes < %ld (vllm_attn_bwd_workspace_bytes)", workspace_bytes, need);
    AttnBwdArgs a;
    a.qkv = qkv; a.out = out; a.dout = grad_out; a.lse = lse; a.delta = static_cast<float *>(workspace); a.dqkv = grad_qkv;
    a.B = B; a.S = S; a.H = H;
    a.nt = (S + QBLK - 1) / QBLK;
    a.scale = softmax_scale;
    a.scale_log2e = softmax_scale * LOG2E;
    const long groups = ((long)B * H + 7) / 8;
    const unsigned grid = (unsigned)(groups * 8 * a.nt);
    if (D == 64) { if (f16) attn_bwd_launch_one<64, true>(a, grid, st); else attn_bwd_launch_one<64, false>(a, grid, st); }
    else { if (f16) attn_bwd_launch_one<128, true>(a, grid, st); else attn_bwd_launch_one<128, false>(a, grid, st); }
    VLLM_CHECK_LAUNCH("attn_bwd kernels");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" long vllm_attn_bwd_workspace_bytes(int B, int S, int H, int D) { return attn_bwd_workspace(B, S, H, D); }

extern "C" int vllm_attn_bwd_qkvpacked_bf16(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *grad_out,
                                            int B, int S, int H, int D, float softmax_scale, uint16_t *grad_qkv, void *workspace,
                                            long workspace_bytes, vllm_stream_t stream)
{
    return attn_bwd_launch(qkv, out, lse, grad_out, B, S, H, D, softmax_scale, grad_qkv, workspace, workspace_bytes, false,
                           (hipStream_t)stream);
}
extern "C" int vllm_attn_bwd_qkvpacked_f16(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *grad_out,
                                           int B, int S, int H, int D, float softmax_scale, uint16_t *grad_qkv, void *workspace,
                                           long workspace_bytes, vllm_stream_t stream)
{
    return attn_bwd_launch(qkv, out, lse, grad_out, B, S, H, D, softmax_scale, grad_qkv, workspace, workspace_bytes, true,
                           (hipStream_t)stream);
}
