// The masked-attention tile that mha.hip (D 32 / 64, [Lq, Lk] mask) and xattn.hip (D 128 / 256, key split) share: 4 waves = 64 query rows
// of one (image, head) against K / V tiles of 64 keys in LDS, K row-major with a pitch of D + 8, V transposed ([d][key]) with a pitch of
// 64 + 8.  wave64, v_mfma_f32_16x16x32_bf16; lane (l15 = lane & 15, g = lane >> 4) of a wave owns query row l15 of the wave's sixteen.
// What is here is the same statement for statement in both kernels; the staging of the tiles, the mask words, the split's bookkeeping, the
// LDS declaration and the launch bounds belong to each file.  The design notes are in mha.hip's file comment.
#pragma once
#include <math.h>
#include "common.hpp"

namespace vllm {

// One of q / k / v / out on the host: rows of H * D elements, `ld` elements apart, images `bs` elements apart.
struct AttnOperand {
    const uint16_t *p;
    long bs;
    int ld;
};

constexpr int ATILE_THREADS = 256, ATILE_QBLK = 64, ATILE_KV = 64;
constexpr int ATILE_VLD = ATILE_KV + 8;                           // V tile: [d][key], row stride in elements
template <int D> constexpr int atile_kld() { return D + 8; }      // K tile: [key][d]

// The part of MhaArgs / XattnArgs that both have (the fields carry the same names), from the launch's arguments.
template <typename Args>
void atile_fill_args(Args &a, const AttnOperand &q, const AttnOperand &k, const AttnOperand &v, const AttnOperand &out,
                     const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, float softmax_scale)
{
    a.q = q.p; a.k = k.p; a.v = v.p; a.out = const_cast<uint16_t *>(out.p);
    a.q_bs = q.bs; a.k_bs = k.bs; a.v_bs = v.bs; a.o_bs = out.bs;
    a.ldq = q.ld; a.ldk = k.ld; a.ldv = v.ld; a.ldo = out.ld;
    a.kpm = key_padding_mask;
    a.B = B; a.Lq = Lq; a.Lk = Lk; a.H = H;
    a.nqt = (Lq + ATILE_QBLK - 1) / ATILE_QBLK;
    a.c2 = softmax_scale * 1.4426950408889634f;
}
// workgroups of a launch with `per` blocks for each (image, head): the (image, head) pairs are padded to whole rounds of the 8 XCDs
static inline long atile_blocks(int B, int H, long per) { return (long)(((long)B * H + 7) / 8) * 8 * per; }

#ifdef __HIPCC__
// block -> ((image, head), which of its `per` blocks): every block of an (image, head) on one XCD, so that the K / V re-reads hit that L2.
// False for the blocks behind the last (image, head): block-uniform, the caller returns in front of every barrier.
__device__ __forceinline__ bool atile_block(int per, int BH, int &bh, int &rem)
{
    const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3;
    bh = (sidx / per) * 8 + xcd;
    rem = sidx % per;
    return bh < BH;
}

// Which [Lq, Lk] slab of an attention mask [n_masks, Lq, Lk] the workgroup of (image, head) pair bh = b H + h reads: slab bh % n_masks.
// n_masks = 1 is one shared mask, B H one per (image, head) -- the 3-d mask of nn.MultiheadAttention -- and B what indexing
// `mask.repeat(H, 1, 1)` by b H + h comes to (GroundingDinoTextEnhancerLayer.forward, ...mask_dn.py:837-839), without the copy.
__device__ __forceinline__ long atile_mask_slab(int bh, int n_masks, int Lq, int Lk) { return (long)(bh % n_masks) * Lq * Lk; }

// Q fragments (B operand): lane (query l15, g) holds Q[query][32 ks + 8 g .. + 7]; rows behind Lq read row Lq - 1.  Returns the row read.
template <int KS>
__device__ __forceinline__ int atile_load_q(const uint16_t *qb, int q_row, int Lq, int ldq, int g, bf16x8_t (&qf)[KS])
{
    const int q_ld = q_row < Lq ? q_row : Lq - 1;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const bf16x8_t *>(qb + (long)q_ld * ldq + 32 * s + 8 * g);
    return q_ld;
}

// S^T = K Q^T with the tile's key rows PERMUTED in the A operand (row m of sub-block s of the 32-key block kb is key
// 32 kb + 8 (m >> 2) + 4 s + (m & 3)): st[kb][s][r] = score of key 32 kb + 8 g + 4 s + r of the lane's query
template <int D>
__device__ __forceinline__ void atile_scores(const uint16_t *ks, const bf16x8_t (&qf)[D / 32], int l15, int g, float4_t (&st)[2][2])
{
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = kb * 32 + 8 * (l15 >> 2) + 4 * s + (l15 & 3);
            float4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < D / 32; ++c) {
                const bf16x8_t kf = *reinterpret_cast<const bf16x8_t *>(&ks[row * atile_kld<D>() + 32 * c + 8 * g]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[c], acc, 0, 0, 0);
            }
            st[kb][s] = acc;
        }
}

// One tile's step of the online softmax in the exp2 domain.  mw[kb][s]: the mask bytes of keys 32 kb + 8 g + 4 s + r, non-zero = -inf.
// Rescales m_run, l_run and o; pf[kb] = bf16(P) of keys 32 kb + 8 g .. + 7: already the B operand of O^T += V^T P^T.
template <int DB>
__device__ __forceinline__ void atile_softmax(float4_t (&st)[2][2], const uint32_t (&mw)[2][2], float c2, float &m_run, float &l_run,
                                              float4_t (&o)[DB], bf16x8_t (&pf)[2])
{
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = ((mw[kb][s] >> (8 * r)) & 0xffu) ? -INFINITY : st[kb][s][r] * c2;
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
}

// O^T += V^T P^T: A = V^T, lane (channel 16 d + l15, g) reads keys 32 kb + 8 g .. + 7 of its channel
template <int D>
__device__ __forceinline__ void atile_accumulate(const uint16_t *vt, const bf16x8_t (&pf)[2], int l15, int g, float4_t (&o)[D / 16])
{
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int d = 0; d < D / 16; ++d) {
            const bf16x8_t vf = *reinterpret_cast<const bf16x8_t *>(&vt[(d * 16 + l15) * ATILE_VLD + kb * 32 + 8 * g]);
            o[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[kb], o[d], 0, 0, 0);
        }
}

// the row sum of a query over its four lane groups
__device__ __forceinline__ float atile_row_sum(float l_run)
{
    float l_tot = l_run + __shfl_xor(l_run, 16);
    l_tot += __shfl_xor(l_tot, 32);
    return l_tot;
}

// bf16(O / l) of the lane's channels 16 d + 4 g + r to op (the row's channel 4 g).  A row whose maximum is still -inf (every key masked)
// is written as NaN, explicitly: softmax of an all -inf row, what torch gives.  (The groups of a query agree: m_run is the reduced maximum.)
// Two paths, not a select per word: with selects xattn's one-split kernel at D 256 measured 3 % slower (profiles/det_kernels_refactor.txt).
template <int DB>
__device__ __forceinline__ void atile_store_row(uint16_t *op, const float4_t (&o)[DB], float m_run, float l_tot)
{
    if (m_run == -INFINITY) {
#pragma unroll
        for (int d = 0; d < DB; ++d) *reinterpret_cast<uint2_t *>(op + d * 16) = (uint2_t){0x7fc07fc0u, 0x7fc07fc0u};
    } else {
        const float inv = 1.0f / l_tot;
#pragma unroll
        for (int d = 0; d < DB; ++d)
            *reinterpret_cast<uint2_t *>(op + d * 16) = (uint2_t){pack_bf16x2(o[d][0] * inv, o[d][1] * inv), pack_bf16x2(o[d][2] * inv, o[d][3] * inv)};
    }
}
#endif

}  // namespace vllm
