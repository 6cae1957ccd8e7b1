// Masked multi-head CROSS attention for LARGE head dims (128 / 256), bf16 in / out, fp32 scores, softmax and accumulation, with an
// optional split over the keys: the two directions of Grounding-DINO's bi-directional image <-> text attention
//   GroundingDinoBiMultiHeadAttention.forward   grounding_dino/modeling_ov_grounding_dino_mask_dn.py:893-1006
// whose one score product is needed at two aspect ratios: tens of thousands of image queries on <= 256 text keys, and <= 256 text
// queries on tens of thousands of image keys.  Not mha.hip (D 32 / 64, a few hundred rows, [Lq, Lk] mask) and not attn.hip (self
// attention over packed qkv, no mask): head dim 256 is 64 accumulator registers per lane for sixteen query rows, and the second
// direction has only B H ceil(Lq / 64) query blocks, so its keys are split over workgroups and a second kernel combines the splits.
//
// gfx950 design (wave64, v_mfma_f32_16x16x32_bf16), the scheme of mha.hip at D 128 / 256:
//   * block = 4 waves = 64 query rows of one (image, head, key split); a wave owns 16 query rows, Q lives in registers (32 VGPRs at
//     D 256), O^T in 64; with the staging registers the kernel stays inside the 256 registers of two waves per SIMD, and two workgroups
//     of 36 / 71 KB of LDS share a CU.  Sixteen rows per wave, not thirty-two: a second row block doubles Q and O to 192 registers, which
//     with the 64 staging registers leaves one wave per SIMD and nothing to run under a wave's softmax;
//   * K / V tiles of 64 keys go through LDS: K row-major, V TRANSPOSED ([d][key]), both padded by 16 bytes per row; the next tile's
//     global loads are in flight (registers) while the current one is computed.  The V transpose is written as 32-bit words of TWO
//     neighbouring keys of a channel (a thread loads the same 16-byte chunk of keys 2p and 2p + 1): each half-wave stores 32
//     consecutive words, no bank conflict.  The fragment READS of both tiles are two-way conflicts in these layouts; K rows in fragment
//     order with row strides of 2 / 10 sixteen-byte slots mod 16 make them conflict-free and measured no change;
//   * scores are computed TRANSPOSED (S^T = K Q^T) with the tile's key rows PERMUTED in the A operand exactly as in mha.hip, so that
//     bf16(P) is already the B operand of O^T += V^T P^T: no LDS round trip of P;
//   * online softmax in the exp2 domain; a masked score is -inf, the running maximum STARTS at -inf; a row whose maximum is still -inf
//     (every key masked) is written as NaN (one split) or as the partial (m = -inf, l = 0, O = 0) (several);
//   * splits > 1: split s of a query block walks keys [s kps, min(Lk, (s + 1) kps)), kps a multiple of the key tile, and writes the fp32
//     (m, l, O) of its rows; xattn_combine_kernel then forms, per row, M = max_s m_s, w_s = exp2(m_s - M) (a split with m_s = -inf gets
//     w_s = 0 and M is finite unless every split is dead, which is the NaN row: (-inf) - (-inf) is never formed), O = sum_s w_s O_s,
//     l = sum_s w_s l_s in ascending s, and stores bf16(O / l).
// The plan (how many splits) is a pure function of (B, Lq, Lk, H, D): never of the device.  No atomics, a fixed order of operations:
// the same bits on every run and on every box.
#include <math.h>
#include "common.hpp"
#include "kernels.hpp"
#include "mha_core.hpp"

namespace vllm {
namespace {

constexpr int XA_THREADS = ATILE_THREADS, XA_QBLK = ATILE_QBLK, XA_KV = ATILE_KV;
// The plan: no split at up to XA_NOSPLIT_TILES key tiles (512 keys: the text side and small maps) or where the query blocks alone fill the
// target of two workgroups on each of 256 CUs; otherwise as many splits as reach the target, of at least XA_MIN_TILES key tiles each (a
// split of fewer than 256 keys does not pay for its partials and their combine).
constexpr long XA_TARGET_WGS = 512, XA_NOSPLIT_TILES = 8, XA_MIN_TILES = 4;

struct XattnArgs {
    const uint16_t *q, *k, *v;
    uint16_t *out;
    float *po;                 // splits > 1: [B H Lq][splits][D] unnormalised partial outputs
    float2_t *pml;             // splits > 1: [B H Lq][splits] {running maximum (exp2 domain), row sum}
    long q_bs, k_bs, v_bs, o_bs;
    int ldq, ldk, ldv, ldo;
    const uint8_t *kpm;        // [B, Lk], non-zero = masked; null = none
    int B, Lq, Lk, H, nqt, splits, kps;
    float c2;                  // softmax_scale * log2(e)
};

template <int D> constexpr int xattn_lds_bytes() { return (XA_KV * atile_kld<D>() + D * ATILE_VLD) * 2 + XA_KV; }

// two workgroups per CU = 2 waves per SIMD, a budget of 256 VGPRs
template <int D, bool SPLIT>
__global__ __launch_bounds__(XA_THREADS, 2) void xattn_fwd_kernel(const XattnArgs a)
{
    constexpr int KS = D / 32;            // k-steps of K Q^T
    constexpr int DB = D / 16;            // 16-wide blocks of the output's channels
    constexpr int KLD = atile_kld<D>(), VLD = ATILE_VLD;   // row strides of the K tile [key][d] and of the V tile [d][key], in elements
    constexpr int CPR = D / 8;           // 16-byte chunks per K / V row
    constexpr int RPP = XA_THREADS / CPR; // K rows one staging pass covers
    constexpr int NI = XA_KV / RPP;       // K staging passes per tile
    constexpr int NV = CPR / 8;           // V staging passes per tile: 32 key pairs x 8 chunks per pass
    extern __shared__ __attribute__((aligned(16))) uint16_t xa_lds[];
    uint16_t *ks = xa_lds, *vt = xa_lds + XA_KV * KLD;
    uint8_t *dead = reinterpret_cast<uint8_t *>(vt + D * VLD);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    int bh, rem;   // block -> (image, head, query block, split)
    if (!atile_block(a.nqt * a.splits, a.B * a.H, bh, rem)) return;
    const int qt = rem / a.splits, split = rem - qt * a.splits;
    const int b = bh / a.H, head = bh % a.H;
    const int kbeg = split * a.kps, kend = a.Lk - kbeg < a.kps ? a.Lk : kbeg + a.kps;   // this split's keys
    const uint16_t *qb = a.q + (long)b * a.q_bs + (long)head * D;
    const uint16_t *kb_ = a.k + (long)b * a.k_bs + (long)head * D;
    const uint16_t *vb_ = a.v + (long)b * a.v_bs + (long)head * D;
    const uint8_t *kpm = a.kpm ? a.kpm + (long)b * a.Lk : nullptr;

    const int q_row = qt * XA_QBLK + wave * 16 + l15;
    const bool live_wave = qt * XA_QBLK + wave * 16 < a.Lq;   // wave-uniform
    bf16x8_t qf[KS];
    atile_load_q<KS>(qb, q_row, a.Lq, a.ldq, g, qf);

    float4_t o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = (float4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    // ---- staging.  K: thread -> (row = pass * RPP + tid / CPR, chunk = tid % CPR).  V: thread -> (keys 2 vp and 2 vp + 1,
    //      chunk = pass * 8 + tid / 32).  Keys behind the split's last one are zeros and marked dead. ----
    const int srow = tid / CPR, sch = tid % CPR, vp = tid & 31, vcg = tid >> 5;
    uint4_t kreg[NI], vreg[NV][2];
    uint32_t dreg = 0;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < NI; ++s) {
            const int key = k0 + s * RPP + srow;
            kreg[s] = (uint4_t){0u, 0u, 0u, 0u};
            if (key < kend) kreg[s] = *reinterpret_cast<const uint4_t *>(kb_ + (long)key * a.ldk + sch * 8);
        }
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int key = k0 + 2 * vp + j;
                vreg[s][j] = (uint4_t){0u, 0u, 0u, 0u};
                if (key < kend) vreg[s][j] = *reinterpret_cast<const uint4_t *>(vb_ + (long)key * a.ldv + (s * 8 + vcg) * 8);
            }
        if (tid < XA_KV) {
            const int key = k0 + tid;
            dreg = key >= kend ? 1u : kpm ? (uint32_t)kpm[key] : 0u;
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int s = 0; s < NI; ++s) *reinterpret_cast<uint4_t *>(&ks[(s * RPP + srow) * KLD + sch * 8]) = kreg[s];
#pragma unroll
        for (int s = 0; s < NV; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = (s * 8 + vcg) * 8 + 2 * e;
                const uint32_t x = vreg[s][0][e], y = vreg[s][1][e];
                *reinterpret_cast<uint32_t *>(&vt[c * VLD + 2 * vp]) = (x & 0xffffu) | (y << 16);
                *reinterpret_cast<uint32_t *>(&vt[(c + 1) * VLD + 2 * vp]) = (x >> 16) | (y & 0xffff0000u);
            }
        if (tid < XA_KV) dead[tid] = (uint8_t)(dreg != 0u);
    };

    const int nkt = (kend - kbeg + XA_KV - 1) / XA_KV;
    fetch(kbeg);
    for (int t = 0; t < nkt; ++t) {
        const int k0 = kbeg + t * XA_KV;
        __syncthreads();   // every wave has read the tile in front
        commit();
        __syncthreads();
        if (t + 1 < nkt) fetch(k0 + XA_KV);   // in flight under the arithmetic below
        if (!live_wave) continue;

        // ---- this lane's 16 mask bytes: keys k0 + 32 kb + 8 g + 4 s + r of its query ----
        uint32_t mw[2][2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) mw[kb][s] = *reinterpret_cast<const uint32_t *>(&dead[kb * 32 + 8 * g + 4 * s]);

        float4_t st[2][2];
        bf16x8_t pf[2];
        atile_scores<D>(ks, qf, l15, g, st);
        atile_softmax<DB>(st, mw, a.c2, m_run, l_run, o, pf);
        atile_accumulate<D>(vt, pf, l15, g, o);
    }

    // ---- finalize: lane (query l15, g) holds channels 16 d + 4 g + r ----
    if (!live_wave || q_row >= a.Lq) return;
    const float l_tot = atile_row_sum(l_run);
    if constexpr (SPLIT) {
        const long slot = ((long)bh * a.Lq + q_row) * a.splits + split;
        float *po = a.po + slot * D + 4 * g;
#pragma unroll
        for (int d = 0; d < DB; ++d) *reinterpret_cast<float4_t *>(po + d * 16) = o[d];
        if (g == 0) a.pml[slot] = (float2_t){m_run, l_tot};
    } else {
        atile_store_row<DB>(a.out + (long)b * a.o_bs + (long)q_row * a.ldo + head * D + 4 * g, o, m_run, l_tot);
    }
}

// One thread per (row, eight channels): the splits of a row in ascending order (file comment).
__global__ __launch_bounds__(256) void xattn_combine_kernel(const XattnArgs a, int D, long items)
{
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int cpr = D >> 3;
    const long row = it / cpr;
    const int ch = (int)(it - row * cpr) * 8;
    const float2_t *ml = a.pml + row * a.splits;
    float M = -INFINITY;
    for (int s = 0; s < a.splits; ++s) M = fmaxf(M, ml[s][0]);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, l = 0.f;
    if (M != -INFINITY) {
        for (int s = 0; s < a.splits; ++s) {
            const float2_t e = ml[s];
            const float w = __builtin_amdgcn_exp2f(e[0] - M);   // a dead split: exp2(-inf) = 0
            const float *po = a.po + (row * a.splits + s) * D + ch;
            const float4_t x = *reinterpret_cast<const float4_t *>(po), y = *reinterpret_cast<const float4_t *>(po + 4);
            l += w * e[1];
#pragma unroll
            for (int c = 0; c < 4; ++c) { acc[c] += w * x[c]; acc[4 + c] += w * y[c]; }
        }
    }
    const long bh = row / a.Lq;
    const int i = (int)(row - bh * a.Lq), b = (int)(bh / a.H), head = (int)(bh % a.H);
    uint4_t w = {0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u, 0x7fc07fc0u};   // every split dead: softmax of an all -inf row
    if (M != -INFINITY) {
        const float inv = 1.0f / l;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] *= inv;
        w = pack8(acc);
    }
    *reinterpret_cast<uint4_t *>(a.out + (long)b * a.o_bs + (long)i * a.ldo + head * D + ch) = w;
}

bool operand_aligned(const AttnOperand &x) { return aligned16(x.p) && x.ld % 8 == 0 && x.bs % 8 == 0; }

bool sizes_ok(int B, int Lq, int Lk, int H, int D)
{
    return (D == 128 || D == 256) && B >= 0 && Lq >= 0 && Lk >= 0 && Lk <= (1 << 30) && H >= 1 && (long)B * H < (1L << 28) &&
           (long)H * D < (1L << 24);
}

void plan(long B, long Lq, long Lk, long H, int *splits, int *kps)
{
    const long nkt = (Lk + XA_KV - 1) / XA_KV, blocks = B * H * ((Lq + XA_QBLK - 1) / XA_QBLK);
    long tps = nkt > 0 ? nkt : 1;
    if (nkt > XA_NOSPLIT_TILES && blocks > 0 && blocks < XA_TARGET_WGS) {
        const long want = (XA_TARGET_WGS + blocks - 1) / blocks;
        tps = (nkt + want - 1) / want;
        if (tps < XA_MIN_TILES) tps = XA_MIN_TILES;
    }
    *splits = nkt > 0 ? (int)((nkt + tps - 1) / tps) : 1;
    *kps = (int)(tps * XA_KV);
}

template <int D, bool SPLIT> int launch(const XattnArgs &a, dim3 grid, hipStream_t st)
{
    static unsigned long long attr_mask = 0;
    constexpr int lds = xattn_lds_bytes<D>();
    if (lds > 48 * 1024 && first_use_on_device(&attr_mask))
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&xattn_fwd_kernel<D, SPLIT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    VLLM_LAUNCH((xattn_fwd_kernel<D, SPLIT>), grid, dim3(XA_THREADS), (size_t)lds, st, a);
    VLLM_CHECK_LAUNCH("xattn_fwd_kernel");
    return VLLM_OK;
}

}  // namespace

long xattn_ws_bytes(int B, int Lq, int Lk, int H, int D)
{
    int splits, kps;
    plan(B, Lq, Lk, H, &splits, &kps);
    return splits > 1 ? (long)B * H * Lq * splits * (D + 2) * 4 : 0;
}

// host-only: VLLM_OK where vllm_xattn_fwd_bf16 would launch (or has nothing to do), VLLM_EINVAL with the reason otherwise
int xattn_fwd_check(const AttnOperand &q, const AttnOperand &k, const AttnOperand &v, const AttnOperand &out, int B, int Lq, int Lk, int H, int D,
                    const void *ws, long ws_bytes)
{
    VLLM_REQUIRE(D == 128 || D == 256, "xattn_fwd: head dim %d (128 or 256)", D);
    VLLM_REQUIRE(sizes_ok(B, Lq, Lk, H, D), "xattn_fwd: B=%d Lq=%d Lk=%d H=%d (B, Lq, Lk >= 0; H >= 1)", B, Lq, Lk, H);
    if ((long)B * Lq == 0) return VLLM_OK;
    VLLM_REQUIRE(Lk >= 1, "xattn_fwd: Lk=%d (at least one key)", Lk);
    VLLM_REQUIRE(q.p && k.p && v.p && out.p, "xattn_fwd: null pointer (q / k / v / out)");
    VLLM_REQUIRE(operand_aligned(q) && operand_aligned(k) && operand_aligned(v) && operand_aligned(out),
                 "xattn_fwd: misaligned operand (16-byte aligned pointers; row and batch strides multiples of 8 elements)");
    VLLM_REQUIRE(q.ld >= H * D && k.ld >= H * D && v.ld >= H * D && out.ld >= H * D, "xattn_fwd: row stride below H D = %d", H * D);
    const long need = xattn_ws_bytes(B, Lq, Lk, H, D);
    if (need > 0) {
        VLLM_REQUIRE(ws, "xattn_fwd: null workspace (the plan splits the keys: %ld bytes)", need);
        VLLM_REQUIRE(aligned16(ws), "xattn_fwd: misaligned workspace (16 bytes)");
        VLLM_REQUIRE(ws_bytes >= need, "xattn_fwd: workspace too small (%ld < %ld bytes)", ws_bytes, need);
    }
    return VLLM_OK;
}

int xattn_fwd_launch(const AttnOperand &q, const AttnOperand &k, const AttnOperand &v, const AttnOperand &out, const uint8_t *key_padding_mask,
                     int B, int Lq, int Lk, int H, int D, float softmax_scale, void *ws, long ws_bytes, hipStream_t st)
{
    const int rc = xattn_fwd_check(q, k, v, out, B, Lq, Lk, H, D, ws, ws_bytes);
    if (rc != VLLM_OK) return rc;
    if ((long)B * Lq == 0) return VLLM_OK;
    XattnArgs a;
    atile_fill_args(a, q, k, v, out, key_padding_mask, B, Lq, Lk, H, softmax_scale);
    plan(B, Lq, Lk, H, &a.splits, &a.kps);
    const long rows = (long)B * H * Lq;
    a.po = a.splits > 1 ? static_cast<float *>(ws) : nullptr;
    a.pml = a.splits > 1 ? reinterpret_cast<float2_t *>(static_cast<float *>(ws) + rows * a.splits * D) : nullptr;
    const long blocks = atile_blocks(B, H, (long)a.nqt * a.splits), items = rows * (D / 8);
    VLLM_REQUIRE(blocks < (1L << 31) && (items + 255) / 256 < (1L << 31), "xattn_fwd: too many workgroups (B H Lq / 64 >= 2^31)");
    const dim3 grid((unsigned)blocks);
    if (a.splits == 1) return D == 128 ? launch<128, false>(a, grid, st) : launch<256, false>(a, grid, st);
    const int r2 = D == 128 ? launch<128, true>(a, grid, st) : launch<256, true>(a, grid, st);
    if (r2 != VLLM_OK) return r2;
    VLLM_LAUNCH(xattn_combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, a, D, items);
    VLLM_CHECK_LAUNCH("xattn_combine_kernel");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_xattn_plan(int B, int Lq, int Lk, int H, int D, int *splits, int *keys_per_split)
{
    VLLM_REQUIRE(D == 128 || D == 256, "xattn_plan: head dim %d (128 or 256)", D);
    VLLM_REQUIRE(sizes_ok(B, Lq, Lk, H, D), "xattn_plan: B=%d Lq=%d Lk=%d H=%d (B, Lq, Lk >= 0; H >= 1)", B, Lq, Lk, H);
    VLLM_REQUIRE(splits && keys_per_split, "xattn_plan: null pointer");
    plan(B, Lq, Lk, H, splits, keys_per_split);
    return VLLM_OK;
}

extern "C" long vllm_xattn_workspace_bytes(int B, int Lq, int Lk, int H, int D)
{
    if (!sizes_ok(B, Lq, Lk, H, D)) {
        set_error("xattn_workspace_bytes: B=%d Lq=%d Lk=%d H=%d D=%d (B, Lq, Lk >= 0; H >= 1; D 128 or 256)", B, Lq, Lk, H, D);
        return -1;
    }
    return xattn_ws_bytes(B, Lq, Lk, H, D);
}

extern "C" int vllm_xattn_fwd_bf16(const uint16_t *q, long q_batch_stride, int ldq, const uint16_t *k, long k_batch_stride, int ldk,
                                   const uint16_t *v, long v_batch_stride, int ldv, uint16_t *out, long o_batch_stride, int ldo,
                                   const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D, float softmax_scale,
                                   void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    return xattn_fwd_launch({q, q_batch_stride, ldq}, {k, k_batch_stride, ldk}, {v, v_batch_stride, ldv}, {out, o_batch_stride, ldo},
                            key_padding_mask, B, Lq, Lk, H, D, softmax_scale, workspace, workspace_bytes, (hipStream_t)stream);
}
