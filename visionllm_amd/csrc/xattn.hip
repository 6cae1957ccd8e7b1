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

namespace vllm {
namespace {

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
constexpr int XA_THREADS = 256, XA_QBLK = 64, XA_KV = 64;
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

template <int D> constexpr int xattn_lds_bytes() { return (XA_KV * (D + 8) + D * (XA_KV + 8)) * 2 + XA_KV; }

// two workgroups per CU = 2 waves per SIMD, a budget of 256 VGPRs
template <int D, bool SPLIT>
__global__ __launch_bounds__(XA_THREADS, 2) void xattn_fwd_kernel(const XattnArgs a)
{
    constexpr int KS = D / 32;            // k-steps of K Q^T
    constexpr int DB = D / 16;            // 16-wide blocks of the output's channels
    constexpr int KLD = D + 8;            // K tile: [key][d], row stride in elements
    constexpr int VLD = XA_KV + 8;        // V tile: [d][key]
    constexpr int CPR = D / 8;            // 16-byte chunks per K / V row
    constexpr int RPP = XA_THREADS / CPR; // K rows one staging pass covers
    constexpr int NI = XA_KV / RPP;       // K staging passes per tile
    constexpr int NV = CPR / 8;           // V staging passes per tile: 32 key pairs x 8 chunks per pass
    extern __shared__ __attribute__((aligned(16))) uint16_t xa_lds[];
    uint16_t *ks = xa_lds, *vt = xa_lds + XA_KV * KLD;
    uint8_t *dead = reinterpret_cast<uint8_t *>(vt + D * VLD);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    // ---- block -> (image, head, query block, split): every block of an (image, head) on one XCD ----
    const int xcd = blockIdx.x & 7, sidx = blockIdx.x >> 3, per = a.nqt * a.splits;
    const int bh = (sidx / per) * 8 + xcd, rem = sidx % per;
    if (bh >= a.B * a.H) return;   // (block-uniform, in front of every barrier)
    const int qt = rem / a.splits, split = rem - qt * a.splits;
    const int b = bh / a.H, head = bh % a.H;
    const int kbeg = split * a.kps, kend = a.Lk - kbeg < a.kps ? a.Lk : kbeg + a.kps;   // this split's keys
    const uint16_t *qb = a.q + (long)b * a.q_bs + (long)head * D;
    const uint16_t *kb_ = a.k + (long)b * a.k_bs + (long)head * D;
    const uint16_t *vb_ = a.v + (long)b * a.v_bs + (long)head * D;
    const uint8_t *kpm = a.kpm ? a.kpm + (long)b * a.Lk : nullptr;

    // ---- Q fragments (B operand): lane (query l15, g) holds Q[query][32 ks + 8 g .. + 7]; rows behind Lq read row Lq - 1 ----
    const int q_row = qt * XA_QBLK + wave * 16 + l15;
    const int q_ld = q_row < a.Lq ? q_row : a.Lq - 1;
    const bool live_wave = qt * XA_QBLK + wave * 16 < a.Lq;   // wave-uniform
    bf16x8_t qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const bf16x8_t *>(qb + (long)q_ld * a.ldq + 32 * s + 8 * g);

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

        // ---- S^T = K Q^T, key rows permuted (mha.hip): st[kb][s][r] = score of key 32 kb + 8 g + 4 s + r ----
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
    if (!live_wave || q_row >= a.Lq) return;
    float l_tot = l_run + __shfl_xor(l_run, 16);
    l_tot += __shfl_xor(l_tot, 32);
    if constexpr (SPLIT) {
        const long slot = ((long)bh * a.Lq + q_row) * a.splits + split;
        float *po = a.po + slot * D + 4 * g;
#pragma unroll
        for (int d = 0; d < DB; ++d) *reinterpret_cast<float4_t *>(po + d * 16) = o[d];
        if (g == 0) a.pml[slot] = (float2_t){m_run, l_tot};
    } else {
        const bool none = m_run == -INFINITY;   // every key of the row masked (the groups of a query agree: m_run is the reduced maximum)
        const float inv = 1.0f / l_tot;
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
int xattn_fwd_check(const uint16_t *q, long q_bs, int ldq, const uint16_t *k, long k_bs, int ldk, const uint16_t *v, long v_bs, int ldv,
                    const uint16_t *out, long o_bs, int ldo, int B, int Lq, int Lk, int H, int D, const void *ws, long ws_bytes)
{
    VLLM_REQUIRE(D == 128 || D == 256, "xattn_fwd: head dim %d (128 or 256)", D);
    VLLM_REQUIRE(sizes_ok(B, Lq, Lk, H, D), "xattn_fwd: B=%d Lq=%d Lk=%d H=%d (B, Lq, Lk >= 0; H >= 1)", B, Lq, Lk, H);
    if ((long)B * Lq == 0) return VLLM_OK;
    VLLM_REQUIRE(Lk >= 1, "xattn_fwd: Lk=%d (at least one key)", Lk);
    VLLM_REQUIRE(q && k && v && out, "xattn_fwd: null pointer (q / k / v / out)");
    VLLM_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 &&
                     q_bs % 8 == 0 && k_bs % 8 == 0 && v_bs % 8 == 0 && o_bs % 8 == 0,
                 "xattn_fwd: misaligned operand (16-byte aligned pointers; row and batch strides multiples of 8 elements)");
    VLLM_REQUIRE(ldq >= H * D && ldk >= H * D && ldv >= H * D && ldo >= H * D, "xattn_fwd: row stride below H D = %d", H * D);
    const long need = xattn_ws_bytes(B, Lq, Lk, H, D);
    if (need > 0) {
        VLLM_REQUIRE(ws, "xattn_fwd: null workspace (the plan splits the keys: %ld bytes)", need);
        VLLM_REQUIRE(aligned16(ws), "xattn_fwd: misaligned workspace (16 bytes)");
        VLLM_REQUIRE(ws_bytes >= need, "xattn_fwd: workspace too small (%ld < %ld bytes)", ws_bytes, need);
    }
    return VLLM_OK;
}

int xattn_fwd_launch(const uint16_t *q, long q_bs, int ldq, const uint16_t *k, long k_bs, int ldk, const uint16_t *v, long v_bs, int ldv,
                     uint16_t *out, long o_bs, int ldo, const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D,
                     float softmax_scale, void *ws, long ws_bytes, hipStream_t st)
{
    const int rc = xattn_fwd_check(q, q_bs, ldq, k, k_bs, ldk, v, v_bs, ldv, out, o_bs, ldo, B, Lq, Lk, H, D, ws, ws_bytes);
    if (rc != VLLM_OK) return rc;
    if ((long)B * Lq == 0) return VLLM_OK;
    XattnArgs a;
    a.q = q; a.k = k; a.v = v; a.out = out;
    a.q_bs = q_bs; a.k_bs = k_bs; a.v_bs = v_bs; a.o_bs = o_bs;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.kpm = key_padding_mask;
    a.B = B; a.Lq = Lq; a.Lk = Lk; a.H = H;
    a.nqt = (Lq + XA_QBLK - 1) / XA_QBLK;
    plan(B, Lq, Lk, H, &a.splits, &a.kps);
    a.c2 = softmax_scale * 1.4426950408889634f;
    const long rows = (long)B * H * Lq;
    a.po = a.splits > 1 ? static_cast<float *>(ws) : nullptr;
    a.pml = a.splits > 1 ? reinterpret_cast<float2_t *>(static_cast<float *>(ws) + rows * a.splits * D) : nullptr;
    const long blocks = (long)(((long)B * H + 7) / 8) * 8 * a.nqt * a.splits, items = rows * (D / 8);
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
    return xattn_fwd_launch(q, q_batch_stride, ldq, k, k_batch_stride, ldk, v, v_batch_stride, ldv, out, o_batch_stride, ldo,
                            key_padding_mask, B, Lq, Lk, H, D, softmax_scale, workspace, workspace_bytes, (hipStream_t)stream);
}
