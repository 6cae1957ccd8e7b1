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
#include "mha_core.hpp"

namespace vllm {
namespace {

constexpr int MHA_THREADS = ATILE_THREADS, MHA_QBLK = ATILE_QBLK, MHA_KV = ATILE_KV;

struct MhaArgs {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    long q_bs, k_bs, v_bs, o_bs;
    int ldq, ldk, ldv, ldo;
    const uint8_t *am, *kpm;   // [n_masks, Lq, Lk] / [B, Lk], non-zero = masked; null = none
    int am_words;              // 1: the mask can be read as 4-byte words (4-byte aligned, Lk % 4 == 0: every row of every slab starts on a word)
    int n_masks;               // slabs of `am`; workgroup (b, head) reads slab (b H + head) % n_masks
    int B, Lq, Lk, H, nqt;
    float c2;                  // softmax_scale * log2(e)
};

// 4 workgroups per CU at the workload shape (B 8 x H 8 x 15 blocks over 256 CUs) = 4 waves per SIMD, a budget of 128 VGPRs: the kernel
// takes 75 (D 32) / 112 (D 64) VGPRs and 9.8 / 18.5 KB of static LDS per workgroup, no scratch
template <int D>
__global__ __launch_bounds__(MHA_THREADS, 4) void mha_fwd_kernel(const MhaArgs a)
{
    constexpr int KS = D / 32;            // k-steps of K Q^T
    constexpr int DB = D / 16;            // 16-wide blocks of the output's channels
    constexpr int KLD = atile_kld<D>(), VLD = ATILE_VLD;   // row strides of the K tile [key][d] and of the V tile [d][key], in elements
    constexpr int CPR = D / 8;            // 16-byte chunks per K / V row
    constexpr int RPP = MHA_THREADS / CPR;   // rows one staging pass covers
    constexpr int NI = MHA_KV / RPP;      // staging passes per tile
    __shared__ __attribute__((aligned(16))) uint16_t ks[MHA_KV * KLD];
    __shared__ __attribute__((aligned(16))) uint16_t vt[D * VLD];
    __shared__ __attribute__((aligned(16))) uint8_t dead[MHA_KV];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    int bh, qt;   // block -> (image, head, query block)
    if (!atile_block(a.nqt, a.B * a.H, bh, qt)) return;
    const int b = bh / a.H, head = bh % a.H;
    const uint16_t *qb = a.q + (long)b * a.q_bs + (long)head * D;
    const uint16_t *kb_ = a.k + (long)b * a.k_bs + (long)head * D;
    const uint16_t *vb_ = a.v + (long)b * a.v_bs + (long)head * D;
    const uint8_t *kpm = a.kpm ? a.kpm + (long)b * a.Lk : nullptr;

    const int q_row = qt * MHA_QBLK + wave * 16 + l15;
    const bool live_wave = qt * MHA_QBLK + wave * 16 < a.Lq;   // wave-uniform
    bf16x8_t qf[KS];
    const int q_ld = atile_load_q<KS>(qb, q_row, a.Lq, a.ldq, g, qf);
    const uint8_t *am = a.am ? a.am + atile_mask_slab(bh, a.n_masks, a.Lq, a.Lk) + (long)q_ld * a.Lk : nullptr;

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

        float4_t st[2][2];
        bf16x8_t pf[2];
        atile_scores<D>(ks, qf, l15, g, st);
        atile_softmax<DB>(st, mw, a.c2, m_run, l_run, o, pf);
        atile_accumulate<D>(vt, pf, l15, g, o);
    }

    // ---- finalize: lane (query l15, g) holds channels 16 d + 4 g + r ----
    if (!live_wave) return;
    const float l_tot = atile_row_sum(l_run);
    if (q_row < a.Lq) atile_store_row<DB>(a.out + (long)b * a.o_bs + (long)q_row * a.ldo + head * D + 4 * g, o, m_run, l_tot);
}

bool operand_ok(const AttnOperand &x, int HD) { return aligned16(x.p) && x.ld % 8 == 0 && x.ld >= HD && x.bs % 8 == 0; }

}  // namespace

// host-only: VLLM_OK where vllm_mha_fwd_bf16 would launch (or has nothing to do), VLLM_EINVAL with the reason otherwise
int mha_fwd_check(const AttnOperand &q, const AttnOperand &k, const AttnOperand &v, const AttnOperand &out, int B, int Lq, int Lk, int H, int D)
{
    VLLM_REQUIRE(D == 32 || D == 64, "mha_fwd: head dim %d (32 or 64)", D);
    VLLM_REQUIRE(B >= 0 && Lq >= 0 && Lk >= 0 && H >= 1 && (long)B * H < (1L << 28) && (long)H * D < (1L << 24),
                 "mha_fwd: B=%d Lq=%d Lk=%d H=%d (B, Lq, Lk >= 0; H >= 1)", B, Lq, Lk, H);
    if ((long)B * Lq == 0) return VLLM_OK;
    VLLM_REQUIRE(Lk >= 1, "mha_fwd: Lk=%d (at least one key)", Lk);
    VLLM_REQUIRE(q.p && k.p && v.p && out.p, "mha_fwd: null pointer (q / k / v / out)");
    VLLM_REQUIRE(operand_ok(q, H * D) && operand_ok(k, H * D) && operand_ok(v, H * D) && operand_ok(out, H * D),
                 "mha_fwd: misaligned operand (16-byte aligned pointers; row and batch strides multiples of 8 elements, row stride at least H D)");
    return VLLM_OK;
}

int mha_fwd_launch(const AttnOperand &q, const AttnOperand &k, const AttnOperand &v, const AttnOperand &out, const uint8_t *attn_mask,
                   const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D, float softmax_scale, hipStream_t st, int n_masks)
{
    const int rc = mha_fwd_check(q, k, v, out, B, Lq, Lk, H, D);
    if (rc != VLLM_OK) return rc;
    VLLM_REQUIRE(n_masks >= 1 && (long)n_masks * Lq * Lk < (1L << 40), "mha_fwd: n_masks=%d (at least 1)", n_masks);
    if ((long)B * Lq == 0) return VLLM_OK;
    MhaArgs a;
    atile_fill_args(a, q, k, v, out, key_padding_mask, B, Lq, Lk, H, softmax_scale);
    a.am = attn_mask;
    a.n_masks = n_masks;
    // (Lk % 4 == 0 makes Lq Lk a multiple of 4 too: a slab's offset keeps the words aligned for every n_masks)
    a.am_words = attn_mask && (reinterpret_cast<uintptr_t>(attn_mask) & 3u) == 0 && Lk % 4 == 0;
    const long blocks = atile_blocks(B, H, a.nqt);
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
    return mha_fwd_launch({q, q_batch_stride, ldq}, {k, k_batch_stride, ldk}, {v, v_batch_stride, ldv}, {out, o_batch_stride, ldo}, attn_mask,
                          key_padding_mask, B, Lq, Lk, H, D, softmax_scale, (hipStream_t)stream);
}

extern "C" int vllm_mha_fwd_masks_bf16(const uint16_t *q, long q_batch_stride, int ldq, const uint16_t *k, long k_batch_stride, int ldk,
                                       const uint16_t *v, long v_batch_stride, int ldv, uint16_t *out, long o_batch_stride, int ldo,
                                       const uint8_t *attn_mask, int n_masks, const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H,
                                       int D, float softmax_scale, vllm_stream_t stream)
{
    return mha_fwd_launch({q, q_batch_stride, ldq}, {k, k_batch_stride, ldk}, {v, v_batch_stride, ldv}, {out, o_batch_stride, ldo}, attn_mask,
                          key_padding_mask, B, Lq, Lk, H, D, softmax_scale, (hipStream_t)stream, n_masks);
}
