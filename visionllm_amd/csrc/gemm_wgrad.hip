// Weight gradient of a Linear:  dW[n, k] = sum_m dY[m, n] A[m, k]   (optionally db[n] = sum_m dY[m, n])
//
// Backward of the projector's linears (visionllmv2/model/modeling_visionllmv2.py:162-182, trained with freeze_vl_bridge=False,
// visionllmv2/train/train.py:162-170).  Both operands are row-major with the reduction running along their ROWS, so neither is
// K-contiguous for the MFMA: [64-row x 128-column] tiles of dY and A are staged as they lie in memory (16-byte loads; zero rows past
// the end of the reduction range, zero columns past N / K) into an XOR-swizzled LDS image, and the MFMA fragments -- 8 consecutive
// rows of ONE column per lane -- come out of it through the hardware transpose read ds_read_b64_tr_b16 (the V operand of attn.hip
// is the in-repo precedent).
//
// gfx950 design: 128 x 128 output tile per 256-thread block, 4 waves (2 x 2), each wave 64 x 64 = 4 x 4 v_mfma_f32_16x16x32_bf16
// tiles; 64 reduction rows per step, LDS double-buffered (2 x 32 KiB), the next step's rows loaded into registers under the current
// step's MFMAs; two blocks per CU.  The product is formed transposed (C[k][n] = A^T dY): a lane then owns 4 consecutive k of one n,
// i.e. 8-byte stores along a dW row.  db rides along as one more MFMA per fragment against a ones operand in the two waves of the
// blocks of output column block 0 (fp32 accumulation of the exact bf16 values: the column sum of dY).
// Split reduction: when the output tiles do not give every CU two blocks, the rows are cut into S ranges (multiples of 64 rows),
// each block leaves an fp32 partial tile in the caller's workspace and one reduce launch sums the S partials in a FIXED order
// (s = 0 .. S-1) and rounds once: run-to-run identical.  fp32 accumulation throughout, one rounding to bf16.
#include <algorithm>
#include "common.hpp"
#include "kernels.hpp"

namespace vllm {

namespace {

constexpr int WG_TN = 128, WG_TK = 128, WG_BM = 64;   // output tile (n x k), reduction rows per step
constexpr int WG_THREADS = 256;
constexpr int WG_ROW = 256;                          // bytes per staged row (128 bf16)
constexpr int WG_OP = WG_BM * WG_ROW;                // 16 KiB per operand per stage
constexpr int WG_LDS = 2 * 2 * WG_OP;                // 2 stages x (dY | A)

struct WgradArgs {
    const uint16_t *dY, *A;
    uint16_t *dW, *db;
    float *part;             // S > 1: [S][N][K] fp32 partial tiles, then [S][N] partial column sums
    int M, N, K, ldy, lda, ldw;
    int nt, kt, S, mchunk;   // tiles along N and K, reduction splits, rows per split (multiple of WG_BM)
};

// LDS image: 16-byte chunk ch (0..15) of staged row r lives at chunk ch ^ swz(r) (plain 256-byte rows with the XOR of the guide's
// transposed-read layout): the two 16-lane groups of a half wave read rows 8 apart in the same columns without a bank conflict
__device__ __forceinline__ int wg_swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// One step's rows of one operand: 64 rows x 16 chunks, 4 chunks per thread.  Rows outside [m, m1) and columns at or past `cols` are
// zeros (they add nothing to dW or db).
__device__ __forceinline__ void wg_load(const uint16_t *__restrict__ src, int ld, int m, int m1, int col0, int cols, uint4_t (&r)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c = threadIdx.x + s * WG_THREADS;
        const int row = c >> 4, ch = c & 15;
        const int mm = m + row, col = col0 + ch * 8;
        r[s] = (uint4_t){0u, 0u, 0u, 0u};
        if (mm < m1 && col < cols) r[s] = *reinterpret_cast<const uint4_t *>(src + (size_t)mm * ld + col);
    }
}
__device__ __forceinline__ void wg_store(char *tile, const uint4_t (&r)[4])
{
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c = threadIdx.x + s * WG_THREADS;
        const int row = c >> 4, ch = c & 15;
        *reinterpret_cast<uint4_t *>(tile + row * WG_ROW + ((ch ^ wg_swz(row)) << 4)) = r[s];
    }
}

// Operand fragment of the 16 columns c0 .. c0 + 15 (c0 a multiple of 16) over the reduction rows 32 ks .. 32 ks + 31: lane l of
// 16-lane group g receives column c0 + (l & 15), row 32 ks + 8 g + e in element e -- the 16x16x32 operand layout on both sides
// (A: row i = the column, k = 8 g + e; B: k = 8 g + e, column j = the column), so the product sums over those rows.  Two
// transposed reads of 4 rows each: lane 4 q + p of a group supplies the address of row q of the block, columns 4 p .. 4 p + 3 =
// byte 8 (p & 1) of chunk c0 / 8 + (p >> 1) through the swizzle.  Every lane of the wave takes part (no lane-dependent branch
// around the call: EXEC is all ones, as the transposed read requires).
__device__ __forceinline__ bf16x8_t wg_frag(const char *tile, int ks, int c0, int lane)
{
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int r_lo = ks * 32 + 8 * g + q, r_hi = r_lo + 4;
    const int ch = (c0 >> 3) + (p >> 1);
    const char *lo = tile + r_lo * WG_ROW + ((ch ^ wg_swz(r_lo)) << 4) + ((p & 1) << 3);
    const char *hi = tile + r_hi * WG_ROW + ((ch ^ wg_swz(r_hi)) << 4) + ((p & 1) << 3);
    const s16x4_t v_lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t *)(uintptr_t)lo);
    const s16x4_t v_hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t *)(uintptr_t)hi);
    return (bf16x8_t){v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
}

template <bool DB>
__global__ __launch_bounds__(WG_THREADS, 2) void gemm_wgrad_kernel(const WgradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 stages][dY tile | A tile]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wn = wave >> 1, wk = wave & 1;
    const int s = blockIdx.x % a.S, tile = blockIdx.x / a.S;
    const int tn = tile % a.nt, tk = tile / a.nt;
    const int n0 = tn * WG_TN, k0 = tk * WG_TK;
    const int m0 = s * a.mchunk, m1 = min(a.M, m0 + a.mchunk);
    const int nsteps = m1 > m0 ? (m1 - m0 + WG_BM - 1) / WG_BM : 0;
    const bool with_db = DB && tk == 0 && wk == 0;   // wave-uniform

    f32x4_t acc[4][4];   // [k fragment j][n fragment i]: C[k][n]
    f32x4_t accb[4];     // column sums of dY (every row of the product against ones holds the same value)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        accb[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j][i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    const short one = (short)0x3f80;   // bf16 1.0
    const bf16x8_t ones = {one, one, one, one, one, one, one, one};

    uint4_t ry[4], ra[4];
    if (nsteps > 0) {
        wg_load(a.dY, a.ldy, m0, m1, n0, a.N, ry);
        wg_load(a.A, a.lda, m0, m1, k0, a.K, ra);
        wg_store(smem, ry);
        wg_store(smem + WG_OP, ra);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const char *cy = smem + (st & 1) * 2 * WG_OP, *ca = cy + WG_OP;
        const bool more = st + 1 < nsteps;
        if (more) {   // the next step's rows, in flight under this step's MFMAs
            wg_load(a.dY, a.ldy, m0 + (st + 1) * WG_BM, m1, n0, a.N, ry);
            wg_load(a.A, a.lda, m0 + (st + 1) * WG_BM, m1, k0, a.K, ra);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t fy[4], fa[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fy[t] = wg_frag(cy, ks, wn * 64 + t * 16, lane);
                fa[t] = wg_frag(ca, ks, wk * 64 + t * 16, lane);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[j], fy[i], acc[j][i], 0, 0, 0);
            if (with_db) {
#pragma unroll
                for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, fy[i], accb[i], 0, 0, 0);
            }
        }
        if (more) {   // (the other stage was last read in step st - 1, before the barrier that ended it)
            char *ny = smem + ((st + 1) & 1) * 2 * WG_OP;
            wg_store(ny, ry);
            wg_store(ny + WG_OP, ra);
        }
        __syncthreads();
    }

    // ---- epilogue: a lane holds C[k .. k+3][n] (rows 4 (l >> 4) + r of the 16 x 16 fragment, column l & 15) ----
    const int nl = lane & 15, kl = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + nl;
        if (n >= a.N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + wk * 64 + j * 16 + kl;
            if (k >= a.K) continue;
            if (a.S > 1) {
                *reinterpret_cast<f32x4_t *>(a.part + ((size_t)s * a.N + n) * a.K + k) = acc[j][i];
            } else {
                uint2_t o;
                o.x = pack_bf16x2(acc[j][i][0], acc[j][i][1]);
                o.y = pack_bf16x2(acc[j][i][2], acc[j][i][3]);
                *reinterpret_cast<uint2_t *>(a.dW + (size_t)n * a.ldw + k) = o;
            }
        }
        if (with_db && (lane >> 4) == 0) {
            if (a.S > 1) a.part[(size_t)a.S * a.N * a.K + (size_t)s * a.N + n] = accb[i][0];
            else a.db[n] = f32_to_bf16(accb[i][0]);
        }
    }
}

// Fixed-order sum of the S partial tiles (and column sums), one rounding to bf16; four k per thread.
__global__ __launch_bounds__(256) void gemm_wgrad_reduce_kernel(const WgradArgs a)
{
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const long k4 = a.K / 4, nk4 = (long)a.N * k4;
    const size_t slice = (size_t)a.N * a.K;
    if (q < nk4) {
        const int n = (int)(q / k4), k = (int)(q - (long)n * k4) * 4;
        f32x4_t t = *reinterpret_cast<const f32x4_t *>(a.part + (size_t)n * a.K + k);
        for (int s = 1; s < a.S; ++s) t += *reinterpret_cast<const f32x4_t *>(a.part + s * slice + (size_t)n * a.K + k);
        uint2_t o;
        o.x = pack_bf16x2(t[0], t[1]);
        o.y = pack_bf16x2(t[2], t[3]);
        *reinterpret_cast<uint2_t *>(a.dW + (size_t)n * a.ldw + k) = o;
    } else if (a.db && q < nk4 + a.N) {
        const int n = (int)(q - nk4);
        const float *pb = a.part + (size_t)a.S * slice;
        float t = pb[n];
        for (int s = 1; s < a.S; ++s) t += pb[(size_t)s * a.N + n];
        a.db[n] = f32_to_bf16(t);
    }
}

// Reduction splits: none when the output tiles give every CU two blocks (4096 x 4096: 1024 tiles); otherwise as many as fill two
// blocks per CU (4096 x 1024: 256 tiles -> 2), each at least 4 steps (256 rows) long, at most 32.
void wgrad_plan(int M, int N, int K, int cus, int *S, int *mchunk)
{
    const long tiles = (long)ceil_div(N, WG_TN) * ceil_div(K, WG_TK);
    int s = 1;
    if (tiles < 2L * cus) {
        s = (int)std::min<long>(32, (2L * cus + tiles - 1) / tiles);
        s = std::min(s, std::max(1, M / (4 * WG_BM)));
    }
    int mc = ceil_div(std::max(M, 1), s);
    mc = ceil_div(mc, WG_BM) * WG_BM;
    *mchunk = mc;
    *S = std::max(1, ceil_div(std::max(M, 1), mc));
}

long g_wgrad_split = 0;   // launches that took the split route (vllm_gemm_wgrad_split_launches: tests assert the route they cover ran)

}  // namespace

long gemm_wgrad_workspace_bytes(int M, int N, int K)
{
    if (M < 0 || N <= 0 || K <= 0) return -1;
    int S, mc;
    wgrad_plan(M, N, K, device_cus(), &S, &mc);
    return S <= 1 ? 0 : (long)S * N * K * 4 + (long)S * N * 4;
}

int gemm_wgrad_launch(const uint16_t *dY, int ldy, const uint16_t *A, int lda, int M, int N, int K, uint16_t *dW, int ldw,
                      uint16_t *db, void *ws, long ws_bytes, hipStream_t st)
{
    VLLM_REQUIRE(dY && A && dW, "gemm_wgrad: null pointer");
    VLLM_REQUIRE(M >= 0 && N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, "gemm_wgrad: N=%d and K=%d must be positive multiples of 64 (M=%d)", N, K, M);
    VLLM_REQUIRE(ldy >= N && lda >= K && ldw >= K && ldy % 8 == 0 && lda % 8 == 0 && ldw % 4 == 0,
                 "gemm_wgrad: row strides ldy=%d, lda=%d (multiples of 8, >= N / K), ldw=%d (multiple of 4, >= K)", ldy, lda, ldw);
    VLLM_REQUIRE(aligned16(dY) && aligned16(A) && (reinterpret_cast<uintptr_t>(dW) & 7u) == 0 && (reinterpret_cast<uintptr_t>(db) & 1u) == 0,
                 "gemm_wgrad: dY and A must be 16-byte aligned, dW 8-byte aligned");
    WgradArgs a;
    a.dY = dY; a.A = A; a.dW = dW; a.db = db; a.part = nullptr;
    a.M = M; a.N = N; a.K = K; a.ldy = ldy; a.lda = lda; a.ldw = ldw;
    a.nt = ceil_div(N, WG_TN); a.kt = ceil_div(K, WG_TK);
    wgrad_plan(M, N, K, device_cus(), &a.S, &a.mchunk);
    if (a.S > 1) {
        const long need = (long)a.S * N * K * 4 + (long)a.S * N * 4;
        VLLM_REQUIRE(ws && ws_bytes >= need && aligned16(ws), "gemm_wgrad: workspace too small or misaligned (%ld < %ld bytes, 16-byte aligned)",
                     ws_bytes, need);
        a.part = reinterpret_cast<float *>(ws);
    }
    static unsigned long long attr_mask = 0;
    if (first_use_on_device(&attr_mask)) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_wgrad_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_wgrad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, WG_LDS);
    }
    if (a.S > 1) __atomic_fetch_add(&g_wgrad_split, 1L, __ATOMIC_RELAXED);
    const dim3 grid((unsigned)((long)a.nt * a.kt * a.S)), block(WG_THREADS);
    if (db) VLLM_LAUNCH((gemm_wgrad_kernel<true>), grid, block, WG_LDS, st, a);
    else VLLM_LAUNCH((gemm_wgrad_kernel<false>), grid, block, WG_LDS, st, a);
    VLLM_CHECK_LAUNCH("gemm_wgrad_kernel");
    if (a.S > 1) {
        const long items = (long)N * (K / 4) + (db ? N : 0);
        VLLM_LAUNCH(gemm_wgrad_reduce_kernel, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, st, a);
        VLLM_CHECK_LAUNCH("gemm_wgrad_reduce_kernel");
    }
    return VLLM_OK;
}

long gemm_wgrad_split_launches() { return __atomic_load_n(&g_wgrad_split, __ATOMIC_RELAXED); }

}  // namespace vllm

using namespace vllm;

extern "C" long vllm_gemm_wgrad_workspace_bytes(int M, int N, int K) { return gemm_wgrad_workspace_bytes(M, N, K); }
extern "C" long vllm_gemm_wgrad_split_launches(void) { return gemm_wgrad_split_launches(); }

extern "C" int vllm_gemm_wgrad_bf16(const uint16_t *dY, int ldy, const uint16_t *A, int lda, int M, int N, int K, uint16_t *dW, int ldw,
                                    uint16_t *db, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    return gemm_wgrad_launch(dY, ldy, A, lda, M, N, K, dW, ldw, db, workspace, workspace_bytes, (hipStream_t)stream);
}
