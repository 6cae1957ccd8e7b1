// Masked multi-head attention forward for SHORT sequences: the query self-attention (denoising mask) and the text cross-attention (text
// padding mask) of the deformable DECODER layers, bf16 in / out, fp32 scores, softmax and accumulation.
//
// Replaces nn.MultiheadAttention's scaled_dot_product core inside
//   DeformableTransformerDecoderLayer.forward  unipose/modeling_unipose.py:3279-3294  (self_attn, ca_text)
//   GroundingDinoDecoderLayer.forward          grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1348-1367 (self_attn, encoder_attn_text)
// Not attn.hip: the det heads have d_model 256 / 8 heads = D 32, Lq != Lk, a boolean [Lq, Lk] mask and a per-image key mask, and a few
// hundred to a thousand rows -- the launch-bound end, where a plain kernel with the right instruction is what there is to win.
//
// gfx950 design (wave64, v_mfma_f32_16x16x32_bf16: K = 32 covers D = 32 in ONE instruction):
//   * block = 4 waves = 64 query rows of one (image, head); a wave owns 16 query rows, Q lives in registers; all query blocks of one
//     (image, head) run on one XCD (as attn.hip), so the K / V re-reads hit that L2;
//   * K / V tiles of 64 keys go through LDS: K row-major, V TRANSPOSED ([d][key]), both padded by 16 bytes per row; the next tile's
//     global loads are in flight (registers) while the current one is computed;
//   * scores are computed TRANSPOSED (S^T = K Q^T) with the tile's key rows PERMUTED in the A operand (row m of sub-block s of the
//     32-key block kb is key 32 kb + 8 (m >> 2) + 4 s + (m & 3)), so that lane (query l & 15, group g = l >> 4) ends up with the EIGHT
//     CONSECUTIVE keys 32 kb + 8 g .. + 7 of its query: bf16(P) is then already the B operand of O^T += V^T P^T, no LDS round trip;
//   * online softmax in the exp2 domain; a masked score is -inf, the running maximum STARTS at -inf; a row whose maximum is still
//     -inf after the last tile (every key masked) is written as NaN, explicitly (softmax of an all -inf row: what torch gives);
//   * tails of Lq and Lk are masked here: keys behind Lk are staged as zeros and marked dead, query rows behind Lq are not stored.
// No atomics, a fixed order of operations: the same bits on every run.
#include <math.h>
#include "common.hpp"
#include "kernels.hpp"

namespace vllm {
namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
constexpr int MHA_THREADS = 256, MHA_QBLK = 64, MHA_KV = 64;

struct MhaArgs {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    long q_bs, k_bs, v_bs, o_bs;
    int ldq, ldk, ldv, ldo;
    const uint8_t *am, *kpm;   // [Lq, Lk] / [B, Lk], non-zero = masked; null = none
    int am_words;              // 1: the [Lq, Lk] mask can be read as 4-byte words (4-byte aligned, Lk % 4 == 0)
    int B, Lq, Lk, H, nqt;
    float c2;                  // softmax_scale * log2(e)
};

// 4 workgroups per CU at the workload shape (B 8 x H 8 x 15 blocks over 256 CUs) = 4 waves per SIMD, a budget of 128 VGPRs: the kernel
// takes 77 (D 32) / 112 (D 64) VGPRs and 9.8 / 18.5 KB of static LDS per workgroup, no scratch
template <int D>
__global__ __launch_bounds__(MHA_THREADS, 4) void mha_fwd_kernel(const MhaArgs a)
{
    constexpr int KS = D / 32;            // k-steps of K Q^T
    constexpr int DB = D / 16;            // 16-wide blocks of the output's channels
    constexpr int KLD = D + 8;            // K tile: [key][d], row stride in elements
    constexpr int VLD = MHA_KV + 8;       // V tile: [d][key]
    constexpr int CPR = D / 8;            // 16-byte chunks per K / V row
    constexpr int RPP = MHA_THREADS / CPR;   // rows one staging pass covers
    constexpr int NI = MHA_KV / RPP;      // staging passes per tile
    __shared__ __attribute__((aligned(16))) uint16_t ks[MHA_KV * KLD];
    __shared__ __attribute__((aligned(16))) uint16_t vt[D * VLD];
    __shared__ __attribute__((aligned(16))) uint8_t dead[MHA_KV];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    // ---- block -> (image, head, query block): all query blocks of an (image, head) on one XCD ----
    const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3;
    const int bh = (sidx / a.nqt) * 8 + xcd, qt = sidx % a.nqt;
    if (bh >= a.B * a.H) return;   // (block-uniform, in front of every barrier)
    const int b = bh / a.H, head = bh % a.H;
    const uint16_t *qb = a.q + (long)b * a.q_bs + (long)head * D;
    const uint16_t *kb_ = a.k + (long)b * a.k_bs + (long)head * D;
    const uint16_t *vb_ = a.v + (long)b * a.v_bs + (long)head * D;
    const uint8_t *kpm = a.kpm ? a.kpm + (long)b * a.Lk : nullptr;

    // ---- Q fragments (B operand): lane (query l15, g) holds Q[query][32 ks + 8 g .. + 7]; rows behind Lq read row Lq - 1 ----
    const int q_row = qt * MHA_QBLK + wave * 16 + l15;
    const int q_ld = q_row < a.Lq ? q_row : a.Lq - 1;
    const bool live_wave = qt * MHA_QBLK + wave * 16 < a.Lq;   // wave-uniform
    bf16x8_t qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const bf16x8_t *>(qb + (long)q_ld * a.ldq + 32 * s + 8 * g);
    const uint8_t *am = a.am ? a.am + (long)q_ld * a.Lk : nullptr;

    float4_t o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = (float4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging: thread -> (row = pass * RPP + tid / CPR, chunk = tid % CPR) of the K and of the V tile; keys behind Lk are zeros ----
    const int srow = tid / CPR, sch = tid % CPR;
    uint4_t kreg[NI], vreg[NI];
    uint32_t dreg = 0;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < NI; ++s) {
            const int key = k0 + s * RPP + srow;
            kreg[s] = (uint4_t){0u, 0u, 0u, 0u};
            vreg[s] = (uint4_t){0u, 0u, 0u, 0u};
            if (key < a.Lk) {
                kreg[s] = *reinterpret_cast<const uint4_t *>(kb_ + (long)key * a.ldk + sch * 8);
                vreg[s] = *reinterpret_cast<const uint4_t *>(vb_ + (long)key * a.ldv + sch * 8);
            }
        }
        if (tid < MHA_KV) {
            const int key = k0 + tid;
            dreg = key >= a.Lk ? 1u : kpm ? (uint32_t)kpm[key] : 0u;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int s = 0; s < NI; ++s) {
            const int row = s * RPP + srow;
            *reinterpret_cast<uint4_t *>(&ks[row * KLD + sch * 8]) = kreg[s];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vt[(sch * 8 + 2 * e) * VLD + row] = (uint16_t)(vreg[s][e] & 0xffffu);
                vt[(sch * 8 + 2 * e + 1) * VLD + row] = (uint16_t)(vreg[s][e] >> 16);
            }
        }
        if (tid < MHA_KV) dead[tid] = (uint8_t)(dreg != 0u);
    };

    const int nkt = (a.Lk + MHA_KV - 1) / MHA_KV;
    fetch(0);
    for (int t = 0; t < nkt; ++t) {
        const int k0 = t * MHA_KV;
        __syncthreads();   // every wave has read the tile in front
        commit();
        __syncthreads();
        if (t + 1 < nkt) fetch(k0 + MHA_KV);   // in flight under the arithmetic below
        if (!live_wave) continue;

        // ---- this lane's 16 mask bytes: keys k0 + 32 kb + 8 g + 4 s + r of its query ----
        uint32_t mw[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int kl = kb * 32 + 8 * g + 4 * s, key = k0 + kl;
                uint32_t w = *reinterpret_cast<const uint32_t *>(&dead[kl]);
                if (am) {
                    if (a.am_words) {
                        if (key < a.Lk) w |= *reinterpret_cast<const uint32_t *>(am + key);   // (Lk % 4 == 0: key + 3 < Lk)
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (key + r < a.Lk && am[key + r]) w |= 0xffu << (8 * r);
                    }
                }
                mw[kb][s] = w;
            }

        // ---- S^T = K Q^T, key rows permuted (file comment): st[kb][s][r] = score of key 32 kb + 8 g + 4 s + r ----
        float4_t st[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int row = kb * 32 + 8 * (l15 >> 2) + 4 * s + (l15 & 3);
                float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < KS; ++c) {
                    const bf16x8_t kf = *reinterpret_cast<const bf16x8_t *>(&ks[row * KLD + 32 * c + 8 * g]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[c], acc, 0, 0, 0);
                }
                st[kb][s] = acc;
            }

        // ---- online softmax, exp2 domain ----
        float mx = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = ((mw[kb][s] >> (8 * r)) & 0xffu) ? -INFINITY : st[kb][s][r] * a.c2;
                    st[kb][s][r] = x;
                    mx = fmaxf(mx, x);
                }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        // every key so far masked: m_new is -inf; subtract 0 instead, so that p = exp2(-inf) = 0 and nothing forms (-inf) - (-inf)
        const float m_use = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);   // m_run = -inf: 0, and l_run and o are still 0
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int d = 0; d < DB; ++d) o[d] *= alpha;
        // P rounded to bf16 (what P V multiplies); the row sum is taken from the ROUNDED values, so O / l normalises what was accumulated
        bf16x8_t pf[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            uint4_t pw;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const float p0 = __builtin_amdgcn_exp2f(st[kb][s][r] - m_use), p1 = __builtin_amdgcn_exp2f(st[kb][s][r + 1] - m_use);
                    const uint32_t w = pack_bf16x2(p0, p1);
                    pw[2 * s + (r >> 1)] = w;
                    l_run += bf16lo_to_f32(w) + bf16hi_to_f32(w);
                }
            pf[kb] = __builtin_bit_cast(bf16x8_t, pw);
        }
        // ---- O^T += V^T P^T: A = V^T, lane (channel 16 d + l15, g) reads keys 32 kb + 8 g .. + 7 of its channel ----
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int d = 0; d < DB; ++d) {
                const bf16x8_t vf = *reinterpret_cast<const bf16x8_t *>(&vt[(d * 16 + l15) * VLD + kb * 32 + 8 * g]);
                o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[kb], o[d], 0, 0, 0);
            }
    }

    // ---- finalize: lane (query l15, g) holds channels 16 d + 4 g + r ----
    if (!live_wave) return;
    float l_tot = l_run + __shfl_xor(l_run, 16);
    l_tot += __shfl_xor(l_tot, 32);
    const bool none = m_run == -INFINITY;   // every key of the row masked (the groups of a query agree: m_run is the reduced maximum)
    const float inv = 1.0f / l_tot;
    if (q_row < a.Lq) {
        uint16_t *op = a.out + (long)b * a.o_bs + (long)q_row * a.ldo + head * D + 4 * g;
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            uint2_t w;
            w.x = none ? 0x7fc07fc0u : pack_bf16x2(o[d][0] * inv, o[d][1] * inv);
            w.y = none ? 0x7fc07fc0u : pack_bf16x2(o[d][2] * inv, o[d][3] * inv);
            *reinterpret_cast<uint2_t *>(op + d * 16) = w;
        }
    }
}

bool operand_ok(const void *p, long bs, int ld, int HD) { return aligned16(p) && ld % 8 == 0 && ld >= HD && bs % 8 == 0; }

}  // namespace

// host-only: VLLM_OK where vllm_mha_fwd_bf16 would launch (or has nothing to do), VLLM_EINVAL with the reason otherwise
int mha_fwd_check(const uint16_t *q, long q_bs, int ldq, const uint16_t *k, long k_bs, int ldk, const uint16_t *v, long v_bs, int ldv,
                  const uint16_t *out, long o_bs, int ldo, int B, int Lq, int Lk, int H, int D)
{
    VLLM_REQUIRE(D == 32 || D == 64, "mha_fwd: head dim %d (32 or 64)", D);
    VLLM_REQUIRE(B >= 0 && Lq >= 0 && Lk >= 0 && H >= 1 && (long)B * H < (1L << 28) && (long)H * D < (1L << 24),
                 "mha_fwd: B=%d Lq=%d Lk=%d H=%d (B, Lq, Lk >= 0; H >= 1)", B, Lq, Lk, H);
    if ((long)B * Lq == 0) return VLLM_OK;
    VLLM_REQUIRE(Lk >= 1, "mha_fwd: Lk=%d (at least one key)", Lk);
    VLLM_REQUIRE(q && k && v && out, "mha_fwd: null pointer (q / k / v / out)");
    VLLM_REQUIRE(operand_ok(q, q_bs, ldq, H * D) && operand_ok(k, k_bs, ldk, H * D) && operand_ok(v, v_bs, ldv, H * D) &&
                     operand_ok(out, o_bs, ldo, H * D),
                 "mha_fwd: misaligned operand (16-byte aligned pointers; row and batch strides multiples of 8 elements, row stride at least H D)");
    return VLLM_OK;
}

int mha_fwd_launch(const uint16_t *q, long q_bs, int ldq, const uint16_t *k, long k_bs, int ldk, const uint16_t *v, long v_bs, int ldv,
                   uint16_t *out, long o_bs, int ldo, const uint8_t *attn_mask, const uint8_t *key_padding_mask, int B, int Lq, int Lk,
                   int H, int D, float softmax_scale, hipStream_t st)
{
    const int rc = mha_fwd_check(q, q_bs, ldq, k, k_bs, ldk, v, v_bs, ldv, out, o_bs, ldo, B, Lq, Lk, H, D);
    if (rc != VLLM_OK) return rc;
    if ((long)B * Lq == 0) return VLLM_OK;
    MhaArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.q_bs = q_bs; a.k_bs = k_bs; a.v_bs = v_bs; a.o_bs = o_bs;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.am = attn_mask; a.kpm = key_padding_mask;
    a.am_words = attn_mask && (reinterpret_cast<uintptr_t>(attn_mask) & 3u) == 0 && Lk % 4 == 0;
    a.B = B; a.Lq = Lq; a.Lk = Lk; a.H = H;
    a.nqt = (Lq + MHA_QBLK - 1) / MHA_QBLK;
    a.c2 = softmax_scale * 1.4426950408889634f;
    const long blocks = (long)(((long)B * H + 7) / 8) * 8 * a.nqt;
    VLLM_REQUIRE(blocks < (1L << 31), "mha_fwd: too many workgroups (B H Lq / 64 >= 2^31)");
    const dim3 grid((unsigned)blocks), block(MHA_THREADS);
    if (D == 32) VLLM_LAUNCH((mha_fwd_kernel<32>), grid, block, 0, st, a);
    else VLLM_LAUNCH((mha_fwd_kernel<64>), grid, block, 0, st, a);
    VLLM_CHECK_LAUNCH("mha_fwd_kernel");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_mha_fwd_bf16(const uint16_t *q, long q_batch_stride, int ldq, const uint16_t *k, long k_batch_stride, int ldk,
                                 const uint16_t *v, long v_batch_stride, int ldv, uint16_t *out, long o_batch_stride, int ldo,
                                 const uint8_t *attn_mask, const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D,
                                 float softmax_scale, vllm_stream_t stream)
{
    return mha_fwd_launch(q, q_batch_stride, ldq, k, k_batch_stride, ldk, v, v_batch_stride, ldv, out, o_batch_stride, ldo, attn_mask,
                          key_padding_mask, B, Lq, Lk, H, D, softmax_scale, (hipStream_t)stream);
}
