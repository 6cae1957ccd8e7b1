// Data-movement kernels around the ViT GEMMs (HBM-bound gathers, coalesced on the write side).
//
//   im2col_patches : pixels [N,3,IMG,IMG] -> A [N*P, Kpad] with k = c*ps*ps + ky*ps + kx (== Conv2d weight
//                    flattening), zero padded to Kpad (multiple of 64) so the patch embedding runs as a GEMM.
//                    Replaces the strided gather inside nn.Conv2d(3, C, k=s=14)
//                    (VisionLLMv2/visionllmv2/model/internvit/modeling_intern_vit.py:73-75, 85-86).
//   cls_rows       : hidden[n, 0, :] = class_embedding + position_embedding[0]   (:87-89)
//   pixel_shuffle  : [N, 1+h*w, C] (CLS dropped) -> [N, (h/2)*(w/2), 4C] with the InternVL (w,h) permute order
//                    (visionllmv2/model/modeling_visionllmv2.py:381-392, 569-578)
//   drop_cls       : [N, 1+T, C] -> [N, T, C]   (:571)  (only used by the stand-alone bridge entry point; the
//                    fused path lets the projector GEMM skip the CLS rows while staging)
#include "common.hpp"
#include "kernels.hpp"

namespace vllm {

// One thread per (patch, channel, ky) row segment of `ps` pixels.
template <typename PIX>
__global__ __launch_bounds__(256) void im2col_kernel(const PIX *__restrict__ px, uint16_t *__restrict__ A, int N,
                                                     int img, int ps, int g /*patches per side*/, int Kpad)
{
    const int P = g * g;
    const long nseg = (long)N * P * 3 * ps;
    const int K = 3 * ps * ps;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nseg; i += (long)gridDim.x * blockDim.x) {
        const int ky = (int)(i % ps);
        long t = i / ps;
        const int c = (int)(t % 3);
        t /= 3;
        const int p = (int)(t % P);
        const int n = (int)(t / P);
        const int pyy = p / g, pxx = p % g;
        const PIX *src = px + (((long)n * 3 + c) * img + (pyy * ps + ky)) * img + pxx * ps;
        uint16_t *dst = A + ((long)n * P + p) * Kpad + c * ps * ps + ky * ps;
        for (int kx = 0; kx < ps; ++kx) {
            if constexpr (sizeof(PIX) == 2) dst[kx] = (uint16_t)src[kx];
            else dst[kx] = f32_to_bf16((float)src[kx]);
        }
        if (c == 2 && ky == ps - 1)
            for (int k = K; k < Kpad; ++k) A[((long)n * P + p) * Kpad + k] = 0;
    }
}

__global__ __launch_bounds__(256) void cls_rows_kernel(const uint16_t *__restrict__ cls, const uint16_t *__restrict__ pos,
                                                       uint16_t *__restrict__ hidden, int N, int S, int C)
{
    const long n_el = (long)N * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_el; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long n = i / C;
        // reference adds in the parameter dtype (bf16): one rounding of the sum
        hidden[n * (long)S * C + c] = f32_to_bf16(bf16_to_f32(cls[c]) + bf16_to_f32(pos[c]));
    }
}

// 16-byte chunk copy: out[n][i2*(h/2)+j2][a*2C + bs*C + ch] = in[n][1 + (2*i2+a)*h + (2*j2+bs)][ch]
__global__ __launch_bounds__(256) void pixel_shuffle_kernel(const uint16_t *__restrict__ in, long in_tile_stride,
                                                            int ldin, int tok0, uint16_t *__restrict__ out, int N, int hw,
                                                            int C)
{
    const int h2 = hw / 2, cch = C / 8;
    const long nchunks = (long)N * h2 * h2 * 4 * cch;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nchunks; i += (long)gridDim.x * blockDim.x) {
        const int ck = (int)(i % cch);
        long t = i / cch;
        const int quad = (int)(t % 4);
        t /= 4;
        const int j2 = (int)(t % h2);
        t /= h2;
        const int i2 = (int)(t % h2);
        const long n = t / h2;
        const int a = quad >> 1, bs = quad & 1;
        const long tok = tok0 + (long)(2 * i2 + a) * hw + (2 * j2 + bs);
        const uint4_t v = *reinterpret_cast<const uint4_t *>(in + n * in_tile_stride + tok * ldin + ck * 8);
        *reinterpret_cast<uint4_t *>(out + (((n * h2 + i2) * h2 + j2) * 4L + quad) * C + ck * 8) = v;
    }
}

__global__ __launch_bounds__(256) void drop_cls_kernel(const uint16_t *__restrict__ in, long in_tile_stride, int ldin,
                                                       uint16_t *__restrict__ out, int N, int T, int C)
{
    const int cch = C / 8;
    const long nchunks = (long)N * T * cch;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nchunks; i += (long)gridDim.x * blockDim.x) {
        const int ck = (int)(i % cch);
        long t = i / cch;
        const int tok = (int)(t % T);
        const long n = t / T;
        *reinterpret_cast<uint4_t *>(out + (n * T + tok) * (long)C + ck * 8) =
            *reinterpret_cast<const uint4_t *>(in + n * in_tile_stride + (long)(1 + tok) * ldin + ck * 8);
    }
}

// Row movers.  Round 5: a WAVE owns a row (its index is one scalar-cached load, no per-chunk 64-bit division -- the round 1-4 form
// spent ~80 instructions of integer division per 16-byte chunk and ran at 0.18 of the HBM roofline) and its lanes walk the row's
// 16-byte chunks, four loads in flight per lane.
__device__ __forceinline__ void move_row(const uint16_t *__restrict__ s, uint16_t *__restrict__ d, int cch, int lane)
{
    int ck = lane;
    for (; ck + 192 < cch; ck += 256) {
        const uint4_t a = *reinterpret_cast<const uint4_t *>(s + ck * 8), b = *reinterpret_cast<const uint4_t *>(s + (ck + 64) * 8);
        const uint4_t c = *reinterpret_cast<const uint4_t *>(s + (ck + 128) * 8), e = *reinterpret_cast<const uint4_t *>(s + (ck + 192) * 8);
        *reinterpret_cast<uint4_t *>(d + ck * 8) = a; *reinterpret_cast<uint4_t *>(d + (ck + 64) * 8) = b;
        *reinterpret_cast<uint4_t *>(d + (ck + 128) * 8) = c; *reinterpret_cast<uint4_t *>(d + (ck + 192) * 8) = e;
    }
    for (; ck < cch; ck += 64) *reinterpret_cast<uint4_t *>(d + ck * 8) = *reinterpret_cast<const uint4_t *>(s + ck * 8);
}

// dst[idx[i], :] = src[i, :]   (16-byte chunks; idx int64 on the device)
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint16_t *__restrict__ src, const int64_t *__restrict__ idx,
                                                           uint16_t *__restrict__ dst, long n, int C, long dst_rows)
{
    const int cch = C / 8, lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    for (long r = wave; r < n; r += nwaves) {
        const long d = idx[r];
        if (d >= 0 && d < dst_rows) move_row(src + r * C, dst + d * C, cch, lane);
    }
}

// dst[di[i], :] = src[si[i], :]; a null index means the identity.  Rows of C bf16.
__global__ __launch_bounds__(256) void copy_rows_kernel(const uint16_t *__restrict__ src, const int64_t *__restrict__ si,
                                                        uint16_t *__restrict__ dst, const int64_t *__restrict__ di, long n, int C,
                                                        long src_rows, long dst_rows)
{
    const int cch = C / 8, lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    for (long r = wave; r < n; r += nwaves) {
        const long s = si ? si[r] : r, d = di ? di[r] : r;
        if (s >= 0 && s < src_rows && d >= 0 && d < dst_rows) move_row(src + s * C, dst + d * C, cch, lane);
    }
}

// ---- visual-token splice with the index bookkeeping on the device (round 5; modeling_visionllmv2.py:582-605) ----------------------
// The reference selects with boolean masks (`image_features[has_image]`, `inputs_embeds[selected] = ...`): two host synchronisations
// and two full copies.  Here one block lists the <im_patch> slots in order (chunked count + block scan), marks the samples that have
// an image, lists THEIR tiles, and decides the token-count rule of :597-603 (equal, or slots a whole multiple of the tokens: repeated;
// anything else: nothing is written and the error flag is raised); a second kernel moves a row per wave.
// Workspace (int32): [0] rows to move, [1] visual tokens offered, [2] error, [3] slots found, [4 ...) slot positions [B L],
// then the kept tiles [n_tiles], then (B > 512 only) the tiles per sample [B].
constexpr int SPL_THREADS = 1024, SPL_HDR = 4, SPL_MAXB = 4096, SPL_BYVAL = 512;
struct SplTiles { int n[SPL_BYVAL]; };   // tiles per sample by value (a kernel argument: no host-to-device copy) for B <= 512

__global__ __launch_bounds__(SPL_THREADS) void splice_index_kernel(const int64_t *__restrict__ ids, long imp_id, const SplTiles tv,
                                                                   const int32_t *__restrict__ tiles_dev, int tiles_mode, int B, int L,
                                                                   int n_tiles, int T, int32_t *__restrict__ ws,
                                                                   int32_t *__restrict__ status)
{
    __shared__ int s_cnt[SPL_THREADS / 64], s_has[SPL_MAXB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = SPL_THREADS / 64;
    const long n = (long)B * L;
    // a wave owns a contiguous segment, read 64 positions (512 contiguous bytes) at a time
    const long per = ((n + NW - 1) / NW + 63) & ~63L, lo = wave * per, hi = lo + per < n ? lo + per : n;
    for (int b = tid; b < B; b += SPL_THREADS) s_has[b] = 0;
    __syncthreads();
    int c = 0;
    for (long i0 = lo; i0 < hi; i0 += 64) {
        const long i = i0 + lane;
        const bool sel = i < hi && ids[i] == imp_id;
        if (sel) s_has[i / L] = 1;   // (benign race: every writer stores 1)
        c += __popcll(__ballot(sel));
    }
    if (lane == 0) s_cnt[wave] = c;
    __syncthreads();
    int r = 0, n_sel = 0;
    for (int w = 0; w < NW; ++w) { const int v = s_cnt[w]; r += w < wave ? v : 0; n_sel += v; }
    int32_t *slots = ws + SPL_HDR, *kept = ws + SPL_HDR + n;
    for (long i0 = lo; i0 < hi; i0 += 64) {   // second pass over the (cached) ids: ranks from the ballot
        const long i = i0 + lane;
        const bool sel = i < hi && ids[i] == imp_id;
        const unsigned long long m = __ballot(sel);
        if (sel) slots[r + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
        r += __popcll(m);
    }
    if (tid == 0) {
        int k = 0, t0 = 0, bad = 0;
        for (int b = 0; b < B; ++b) {   // the tiles of the samples that have an image, in order (:585-592)
            const int nt = tiles_mode == 0 ? 1 : tiles_mode == 1 ? tv.n[b] : tiles_dev[b];
            if (nt < 0 || t0 + nt > n_tiles) { bad = 1; break; }
            if (s_has[b])
                for (int j = 0; j < nt; ++j) kept[k++] = t0 + j;
            t0 += nt;
        }
        if (t0 != n_tiles) bad = 1;
        const long n_vit = (long)k * T;
        if (!bad && n_sel != n_vit && !(n_vit > 0 && n_sel > n_vit && n_sel % n_vit == 0)) bad = 1;
        ws[0] = bad ? 0 : n_sel; ws[1] = (int32_t)n_vit; ws[2] = bad; ws[3] = n_sel;
        if (status) { status[0] = n_sel; status[1] = (int32_t)n_vit; status[2] = bad; status[3] = k; }
    }
}

// row i of the slot list <- visual token i (mod the tokens offered) of the kept tiles; a wave per row
__global__ __launch_bounds__(256) void splice_move_kernel(const uint16_t *__restrict__ feats, const int32_t *__restrict__ ws, long n,
                                                          int T, int C, uint16_t *__restrict__ embeds)
{
    const int cch = C / 8, lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    const int n_move = ws[0], n_vit = ws[1];
    const int32_t *slots = ws + SPL_HDR, *kept = ws + SPL_HDR + n;
    for (long r = wave; r < n_move; r += nwaves) {
        const int j = (int)(r % n_vit), kt = j / T, tok = j - kt * T;
        move_row(feats + ((long)kept[kt] * T + tok) * C, embeds + (long)slots[r] * C, cch, lane);
    }
}

// ---- backward of the splice: pure row movement again, driven by the workspace the forward left (slot list, kept tiles, header) ----
// How many entries of the ascending list a[0, n) are below v.  Wave-uniform: 64 probes per step, so 2^18 entries take three steps.
__device__ __forceinline__ int wave_lower_bound(const int32_t *__restrict__ a, int n, int v, int lane)
{
    int lo = 0, len = n;   // the answer lies in [lo, lo + len]
    while (len > 0) {
        const int step = (len + 63) / 64;
        const long off = (long)(lane + 1) * step - 1;
        const bool below = off < len && a[lo + off] < v;   // (ascending: true on a prefix of the lanes)
        const int c = __popcll(__ballot(below));
        const int rest = len - c * step;
        lo += c * step;
        len = rest < step - 1 ? rest : step - 1;
    }
    return lo;
}

__device__ __forceinline__ void zero_row(uint16_t *__restrict__ d, int cch, int lane)
{
    const uint4_t z = {0u, 0u, 0u, 0u};
    for (int ck = lane; ck < cch; ck += 64) *reinterpret_cast<uint4_t *>(d + ck * 8) = z;
}

// d = bf16(s[rows[0]] + s[rows[stride]] + ...), k terms added in fp32 in that order and rounded once
__device__ __forceinline__ void sum_rows(const uint16_t *__restrict__ s, const int32_t *__restrict__ rows, long stride, int k,
                                         long s_rows, int C, uint16_t *__restrict__ d, int cch, int lane)
{
    for (int ck = lane; ck < cch; ck += 64) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < k; ++t) {
            const long r = rows[t * stride];
            if (r < 0 || r >= s_rows) continue;
            const uint4_t v = *reinterpret_cast<const uint4_t *>(s + r * C + ck * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[2 * e] += bf16lo_to_f32(v[e]); acc[2 * e + 1] += bf16hi_to_f32(v[e]); }
        }
        uint4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[2 * e], acc[2 * e + 1]);
        *reinterpret_cast<uint4_t *>(d + ck * 8) = o;
    }
}

// A wave per item.  Items [0, n_chunks): SPLB_ROWS consecutive rows of grad_embeds -- a slot row is zeroed, any other row is
// grad_out's (one search of the slot list per chunk, then a walk).  Items behind them: one row of grad_feats each -- visual token j
// of a kept tile sums grad_out over the slots r = j, j + n_vit, ... < rows moved; a dropped tile, or a forward that wrote nothing,
// gives zeros.  Every grad_out row is read by exactly one of the two halves, every output row is written exactly once.  A half whose
// output was not asked for has no items (n_chunks / n_frows == 0); n_tok = n_tiles * T either way.
constexpr int SPLB_ROWS = 4;
__global__ __launch_bounds__(256) void splice_backward_kernel(const int32_t *__restrict__ ws, const uint16_t *__restrict__ gout, long n,
                                                              long n_chunks, long n_frows, long n_tok, int T, int C,
                                                              uint16_t *__restrict__ gemb, uint16_t *__restrict__ gfeat)
{
    const int cch = C / 8, lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    // (the header is the forward's; the clamps and the row checks below only keep a workspace that is NOT the forward's inside the tensors)
    const int n_vit = ws[1] > 0 && ws[1] <= n_tok ? ws[1] : 0;
    const int n_move = n_vit > 0 && ws[0] > 0 && ws[0] <= n ? ws[0] : 0;
    const int32_t *slots = ws + SPL_HDR, *kept = ws + SPL_HDR + n;
    for (long it = wave; it < n_chunks + n_frows; it += nwaves) {
        if (it < n_chunks) {
            const long r0 = it * SPLB_ROWS, r1 = r0 + SPLB_ROWS < n ? r0 + SPLB_ROWS : n;
            int p = wave_lower_bound(slots, n_move, (int)r0, lane);
            for (long r = r0; r < r1; ++r) {
                if (p < n_move && slots[p] == r) { zero_row(gemb + r * C, cch, lane); ++p; }
                else move_row(gout + r * C, gemb + r * C, cch, lane);
            }
        } else {
            const long q = it - n_chunks;
            const int tile = (int)(q / T), tok = (int)(q - (long)tile * T), n_kept = n_vit / T;
            const int kt = n_move > 0 ? wave_lower_bound(kept, n_kept, tile, lane) : n_kept;
            uint16_t *d = gfeat + q * C;
            if (kt >= n_kept || kept[kt] != tile) { zero_row(d, cch, lane); continue; }
            const int j = kt * T + tok, k = n_move / n_vit;
            if (k == 1) {
                const long s = slots[j];
                if (s >= 0 && s < n) move_row(gout + s * C, d, cch, lane);
                else zero_row(d, cch, lane);
            } else sum_rows(gout, slots + j, n_vit, k, n, C, d, cch, lane);
        }
    }
}

// ---- backward of the other four token loops: two row kernels driven by index arrays the forward built in torch ----------------------
// Segment sum.  A wave owns (dst row d, slab of 64 x 8 channels): each lane keeps 8 fp32 sums of one 16-byte chunk, so a gradient of
// 4 or 64 table rows x 4096 channels still spreads over C / 512 waves per row.  The segment bounds and the term indices are wave-uniform
// loads; the load of term k + 1 is issued before term k is widened and added (segments are 0 to 8 terms long in practice).  The sums
// start from -0.0, the identity of the fp32 add for EVERY value (+0.0 would turn a lone -0.0 term into +0.0), and a segment without a
// valid term stores +0.0, so one term is a bit-exact copy and no term is a zero row.  A term whose row lies outside [0, src_rows) is
// skipped, a segment is clamped to [0, n_idx] first: no content of seg_ptr / src_idx reaches outside the four buffers.
__global__ __launch_bounds__(256) void rows_segment_sum_kernel(const uint16_t *__restrict__ src, long src_rows,
                                                               const int64_t *__restrict__ seg_ptr, const int64_t *__restrict__ src_idx,
                                                               long n_idx, uint16_t *__restrict__ dst, long dst_rows, int C)
{
    const int cch = C / 8, n_slabs = (cch + 63) / 64, lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    const uint4_t z = {0u, 0u, 0u, 0u};
    for (long it = wave; it < dst_rows * n_slabs; it += nwaves) {
        const long d = it / n_slabs;
        const int ck = (int)(it - d * n_slabs) * 64 + lane;
        const bool act = ck < cch;
        long lo = seg_ptr[d], hi = seg_ptr[d + 1];
        lo = lo < 0 ? 0 : lo > n_idx ? n_idx : lo;
        hi = hi < 0 ? 0 : hi > n_idx ? n_idx : hi;   // (hi < lo: the loop below does not run -- an empty segment)
        float acc[8] = {-0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f, -0.f};
        bool any = false, cur_ok = false;
        uint4_t cur = z;
        if (lo < hi) {
            const long r = src_idx[lo];
            cur_ok = r >= 0 && r < src_rows;
            if (cur_ok && act) cur = *reinterpret_cast<const uint4_t *>(src + r * C + ck * 8);
        }
        for (long k = lo; k < hi; ++k) {
            uint4_t nxt = z;
            bool nxt_ok = false;
            if (k + 1 < hi) {
                const long r = src_idx[k + 1];
                nxt_ok = r >= 0 && r < src_rows;
                if (nxt_ok && act) nxt = *reinterpret_cast<const uint4_t *>(src + r * C + ck * 8);
            }
            if (cur_ok) {
                any = true;
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[2 * e] += bf16lo_to_f32(cur[e]); acc[2 * e + 1] += bf16hi_to_f32(cur[e]); }
            }
            cur = nxt;
            cur_ok = nxt_ok;
        }
        if (!act) continue;
        uint4_t o = z;
        if (any) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(acc[2 * e], acc[2 * e + 1]);
        }
        *reinterpret_cast<uint4_t *>(dst + d * C + ck * 8) = o;
    }
}

// dst[r, :] = flag[r] ? 0 : src[r, :]; a wave per row.  A flagged row's source is not read.
__global__ __launch_bounds__(256) void copy_rows_masked_kernel(const uint16_t *__restrict__ src, const uint8_t *__restrict__ flag,
                                                               uint16_t *__restrict__ dst, long rows, int C)
{
    const int cch = C / 8, lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    for (long r = wave; r < rows; r += nwaves) {
        if (flag[r]) zero_row(dst + r * C, cch, lane);
        else move_row(src + r * C, dst + r * C, cch, lane);
    }
}

static inline unsigned grid_for(long n)
{
    long b = (n + 255) / 256;
    if (b > 256L * 16) b = 256L * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

int im2col_launch(const void *pixels, int pixel_is_f32, uint16_t *A, int N, int img, int ps, int Kpad, hipStream_t st)
{
    VLLM_REQUIRE(pixels && A, "im2col: null pointer");
    VLLM_REQUIRE(ps > 0 && img % ps == 0 && Kpad >= 3 * ps * ps, "im2col: bad geometry img=%d patch=%d Kpad=%d", img, ps, Kpad);
    if (N == 0) return VLLM_OK;
    const int g = img / ps;
    const long nseg = (long)N * g * g * 3 * ps;
    if (pixel_is_f32)
        VLLM_LAUNCH((im2col_kernel<float>), dim3(grid_for(nseg)), dim3(256), 0, st, (const float *)pixels, A, N, img, ps, g, Kpad);
    else
        VLLM_LAUNCH((im2col_kernel<uint16_t>), dim3(grid_for(nseg)), dim3(256), 0, st, (const uint16_t *)pixels, A, N, img, ps, g, Kpad);
    VLLM_CHECK_LAUNCH("im2col_kernel");
    return VLLM_OK;
}

int cls_rows_launch(const uint16_t *cls, const uint16_t *pos, uint16_t *hidden, int N, int S, int C, hipStream_t st)
{
    if (N == 0) return VLLM_OK;
    VLLM_LAUNCH(cls_rows_kernel, dim3(grid_for((long)N * C)), dim3(256), 0, st, cls, pos, hidden, N, S, C);
    VLLM_CHECK_LAUNCH("cls_rows_kernel");
    return VLLM_OK;
}

int pixel_shuffle_launch(const uint16_t *in, long in_tile_stride, int ldin, int tok0, uint16_t *out, int N, int hw,
                         int C, hipStream_t st)
{
    VLLM_REQUIRE(in && out, "pixel_shuffle: null pointer");
    VLLM_REQUIRE(hw % 2 == 0 && C % 8 == 0 && ldin % 8 == 0 && in_tile_stride % 8 == 0 && aligned16(in) && aligned16(out),
                 "pixel_shuffle: needs even grid, C %% 8 == 0 and 16-byte aligned hidden / out");
    if (N == 0) return VLLM_OK;
    VLLM_LAUNCH(pixel_shuffle_kernel, dim3(grid_for((long)N * hw * hw * C / 8)), dim3(256), 0, st, in,
                       in_tile_stride, ldin, tok0, out, N, hw, C);
    VLLM_CHECK_LAUNCH("pixel_shuffle_kernel");
    return VLLM_OK;
}

int drop_cls_launch(const uint16_t *in, long in_tile_stride, int ldin, uint16_t *out, int N, int T, int C, hipStream_t st)
{
    VLLM_REQUIRE(in && out && C % 8 == 0 && ldin % 8 == 0 && in_tile_stride % 8 == 0 && aligned16(in) && aligned16(out),
                 "drop_cls: bad arguments");
    if (N == 0) return VLLM_OK;
    VLLM_LAUNCH(drop_cls_kernel, dim3(grid_for((long)N * T * C / 8)), dim3(256), 0, st, in, in_tile_stride, ldin,
                       out, N, T, C);
    VLLM_CHECK_LAUNCH("drop_cls_kernel");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_scatter_rows_bf16(const uint16_t *src, const int64_t *idx, uint16_t *dst, long n, int C, long dst_rows,
                                      vllm_stream_t stream)
{
    VLLM_REQUIRE(n >= 0 && C > 0 && C % 8 == 0, "scatter_rows: C must be a positive multiple of 8");
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(src && idx && dst && aligned16(src) && aligned16(dst), "scatter_rows: null pointer, or src / dst not 16-byte aligned");
    VLLM_LAUNCH(scatter_rows_kernel, dim3(grid_for(n * 64)), dim3(256), 0, (hipStream_t)stream, src, idx, dst, n, C,
                dst_rows);
    VLLM_CHECK_LAUNCH("scatter_rows_kernel");
    return VLLM_OK;
}

extern "C" long vllm_splice_workspace_ints(int B, int L, int n_tiles) { return (long)SPL_HDR + (long)B * L + n_tiles + (B > SPL_BYVAL ? B : 0); }

extern "C" int vllm_splice_visual_tokens_bf16(const int64_t *input_ids, long imp_token_id, const uint16_t *image_features,
                                              const int32_t *tiles_per_sample, int B, int L, int n_tiles, int T, int C,
                                              uint16_t *inputs_embeds, int32_t *workspace, int32_t *status, vllm_stream_t stream)
{
    VLLM_REQUIRE(B >= 0 && L >= 0 && n_tiles >= 0 && T >= 0 && C > 0 && C % 8 == 0, "splice_visual_tokens: bad sizes (C must be a positive multiple of 8)");
    VLLM_REQUIRE(B <= SPL_MAXB && (long)B * L < (1L << 31) && (long)n_tiles * T < (1L << 31), "splice_visual_tokens: too many samples / positions / tokens for one call");
    VLLM_REQUIRE(workspace, "splice_visual_tokens: null workspace");
    VLLM_REQUIRE((long)B * L == 0 || (input_ids && inputs_embeds && aligned16(inputs_embeds)), "splice_visual_tokens: null pointer, or inputs_embeds not 16-byte aligned");
    VLLM_REQUIRE((long)n_tiles * T == 0 || (image_features && aligned16(image_features)), "splice_visual_tokens: null image_features, or not 16-byte aligned");
    SplTiles tv;
    int mode = 0;
    const int32_t *tdev = nullptr;
    if (tiles_per_sample && B <= SPL_BYVAL) {
        mode = 1;
        for (int b = 0; b < B; ++b) tv.n[b] = tiles_per_sample[b];
    } else if (tiles_per_sample) {   // (more than 512 samples: through the workspace)
        mode = 2;
        int32_t *d = workspace + SPL_HDR + (long)B * L + n_tiles;
        VLLM_REQUIRE(hipMemcpyAsync(d, tiles_per_sample, sizeof(int32_t) * B, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess,
                     "splice_visual_tokens: copy of the tiles per sample failed");
        tdev = d;
    }
    VLLM_LAUNCH(splice_index_kernel, dim3(1), dim3(SPL_THREADS), 0, (hipStream_t)stream, input_ids, imp_token_id, tv, tdev, mode, B, L,
                n_tiles, T, workspace, status);
    VLLM_CHECK_LAUNCH("splice_index_kernel");
    if ((long)B * L == 0 || (long)n_tiles * T == 0) return VLLM_OK;
    VLLM_LAUNCH(splice_move_kernel, dim3(grid_for((long)B * L * 64)), dim3(256), 0, (hipStream_t)stream, image_features, workspace,
                (long)B * L, T, C, inputs_embeds);
    VLLM_CHECK_LAUNCH("splice_move_kernel");
    return VLLM_OK;
}

extern "C" int vllm_splice_visual_tokens_backward_bf16(const int32_t *workspace, const uint16_t *grad_out, int B, int L, int n_tiles, int T,
                                                       int C, uint16_t *grad_inputs_embeds, uint16_t *grad_image_features,
                                                       vllm_stream_t stream)
{
    VLLM_REQUIRE(B >= 0 && L >= 0 && n_tiles >= 0 && T >= 0 && C > 0 && C % 8 == 0, "splice_visual_tokens_backward: bad sizes (C must be a positive multiple of 8)");
    VLLM_REQUIRE(B <= SPL_MAXB && (long)B * L < (1L << 31) && (long)n_tiles * T < (1L << 31), "splice_visual_tokens_backward: too many samples / positions / tokens for one call");
    VLLM_REQUIRE(aligned16(grad_out) && aligned16(grad_inputs_embeds) && aligned16(grad_image_features),
                 "splice_visual_tokens_backward: grad_out, grad_inputs_embeds and grad_image_features must be 16-byte aligned");
    const long n = (long)B * L, n_tok = (long)n_tiles * T;
    const long n_chunks = grad_inputs_embeds ? (n + SPLB_ROWS - 1) / SPLB_ROWS : 0, n_frows = grad_image_features ? n_tok : 0;
    if (n_chunks + n_frows == 0) return VLLM_OK;
    VLLM_REQUIRE(workspace, "splice_visual_tokens_backward: null workspace");
    VLLM_REQUIRE(n == 0 || grad_out, "splice_visual_tokens_backward: null grad_out");
    VLLM_LAUNCH(splice_backward_kernel, dim3(grid_for((n_chunks + n_frows) * 64)), dim3(256), 0, (hipStream_t)stream, workspace, grad_out, n,
                n_chunks, n_frows, n_tok, T, C, grad_inputs_embeds, grad_image_features);
    VLLM_CHECK_LAUNCH("splice_backward_kernel");
    return VLLM_OK;
}

extern "C" int vllm_copy_rows_bf16(const uint16_t *src, const int64_t *src_idx, uint16_t *dst, const int64_t *dst_idx, long n,
                                   int C, long src_rows, long dst_rows, vllm_stream_t stream)
{
    VLLM_REQUIRE(n >= 0 && C > 0 && C % 8 == 0, "copy_rows: C must be a positive multiple of 8");
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(src && dst && aligned16(src) && aligned16(dst), "copy_rows: null pointer, or src / dst not 16-byte aligned");
    VLLM_LAUNCH(copy_rows_kernel, dim3(grid_for(n * 64)), dim3(256), 0, (hipStream_t)stream, src, src_idx, dst, dst_idx, n, C,
                src_rows, dst_rows);
    VLLM_CHECK_LAUNCH("copy_rows_kernel");
    return VLLM_OK;
}

extern "C" int vllm_rows_segment_sum_bf16(const uint16_t *src, long src_rows, const int64_t *seg_ptr, const int64_t *src_idx, long n_idx,
                                          uint16_t *dst, long dst_rows, int C, vllm_stream_t stream)
{
    VLLM_REQUIRE(C > 0 && C % 8 == 0, "rows_segment_sum: C must be a positive multiple of 8");
    VLLM_REQUIRE(src_rows >= 0 && n_idx >= 0 && dst_rows >= 0, "rows_segment_sum: src_rows, n_idx and dst_rows must not be negative");
    VLLM_REQUIRE(aligned16(src) && aligned16(dst), "rows_segment_sum: src and dst must be 16-byte aligned");
    if (dst_rows == 0) return VLLM_OK;
    VLLM_REQUIRE(seg_ptr && dst, "rows_segment_sum: null seg_ptr or dst");
    VLLM_REQUIRE(n_idx == 0 || (src && src_idx), "rows_segment_sum: null src or src_idx with n_idx > 0");
    const long items = dst_rows * ((C / 8 + 63) / 64);
    VLLM_LAUNCH(rows_segment_sum_kernel, dim3(grid_for(items * 64)), dim3(256), 0, (hipStream_t)stream, src, src_rows, seg_ptr, src_idx,
                n_idx, dst, dst_rows, C);
    VLLM_CHECK_LAUNCH("rows_segment_sum_kernel");
    return VLLM_OK;
}

extern "C" int vllm_copy_rows_masked_bf16(const uint16_t *src, const uint8_t *zero_row, uint16_t *dst, long rows, int C,
                                          vllm_stream_t stream)
{
    VLLM_REQUIRE(C > 0 && C % 8 == 0, "copy_rows_masked: C must be a positive multiple of 8");
    VLLM_REQUIRE(rows >= 0, "copy_rows_masked: rows must not be negative");
    VLLM_REQUIRE(aligned16(src) && aligned16(dst), "copy_rows_masked: src and dst must be 16-byte aligned");
    if (rows == 0) return VLLM_OK;
    VLLM_REQUIRE(src && zero_row && dst, "copy_rows_masked: null src, zero_row or dst");
    VLLM_LAUNCH(copy_rows_masked_kernel, dim3(grid_for(rows * 64)), dim3(256), 0, (hipStream_t)stream, src, zero_row, dst, rows, C);
    VLLM_CHECK_LAUNCH("copy_rows_masked_kernel");
    return VLLM_OK;
}

extern "C" int vllm_im2col_patches(const void *pixels, int pixel_is_f32, uint16_t *A, int N, int img, int patch,
                                   int Kpad, vllm_stream_t stream)
{
    return im2col_launch(pixels, pixel_is_f32, A, N, img, patch, Kpad, (hipStream_t)stream);
}

extern "C" int vllm_pixel_shuffle_bf16(const uint16_t *hidden, long tile_stride, int ld, int tok0, uint16_t *out, int N,
                                       int hw, int C, vllm_stream_t stream)
{
    return pixel_shuffle_launch(hidden, tile_stride, ld, tok0, out, N, hw, C, (hipStream_t)stream);
}
