// Row-wise and layout kernels of the projector backward (bridge_train.cpp):
//   transpose_bf16_kernel   W [R, C] -> W^T: the input-gradient GEMM dX = dY W runs on the existing bf16 GEMM (X W^T form) with
//                           W^T as its weight.  The weights are small next to the activations (<= 105 MB at InternViT-6B's
//                           12 800 -> 4096 Linear, against 10 240 x 4096 rows of dY), so one LDS-tiled transpose per backward is
//                           cheaper than a second, transposed B loader in every GEMM schedule.
//   ln_bwd_kernel           nn.LayerNorm backward (the InternVL projector's LayerNorm, modeling_visionllmv2.py:166-167): per row the
//                           statistics are recomputed from x in fp32, grad_x = r (g - mean(g) - xhat mean(g xhat)), g = grad_y gamma;
//                           the column sums sum_m grad_y xhat / sum_m grad_y go through per-block fp32 partials (each thread owns
//                           its columns in LDS) and ln_bwd_reduce_kernel adds the blocks in a fixed order: run-to-run identical.
#include <algorithm>
#include "common.hpp"
#include "kernels.hpp"

namespace vllm {

namespace {

constexpr int TR_T = 64;   // transpose tile

__global__ __launch_bounds__(256) void transpose_bf16_kernel(const uint16_t *__restrict__ w, int ldw, uint16_t *__restrict__ wt, int ldt)
{
    __shared__ __attribute__((aligned(16))) uint16_t t[TR_T][TR_T + 8];   // (144-byte rows: 16-byte aligned chunks, banks spread)
    const int r0 = blockIdx.y * TR_T, c0 = blockIdx.x * TR_T;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = threadIdx.x + 256 * s, row = i >> 3, ch = i & 7;
        *reinterpret_cast<uint4_t *>(&t[row][ch * 8]) = *reinterpret_cast<const uint4_t *>(w + (size_t)(r0 + row) * ldw + c0 + ch * 8);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int i = threadIdx.x + 256 * s, col = i >> 3, ch = i & 7;   // output row c0 + col, elements r0 + 8 ch .. + 7
        uint32_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = (uint32_t)t[ch * 8 + 2 * k][col] | ((uint32_t)t[ch * 8 + 2 * k + 1][col] << 16);
        *reinterpret_cast<uint4_t *>(wt + (size_t)(c0 + col) * ldt + r0 + ch * 8) = (uint4_t){p[0], p[1], p[2], p[3]};
    }
}

constexpr int LNB_THREADS = 256;
constexpr int LNB_MAX_C = 16384;

// sum over the block, the same value in every thread (xor butterfly inside the wave, then the 4 waves in a fixed order)
__device__ __forceinline__ float2_t lnb_block_sum2(float a, float b, float *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * w] = a; red[2 * w + 1] = b; }
    __syncthreads();
    const float2_t r = {(red[0] + red[2]) + (red[4] + red[6]), (red[1] + red[3]) + (red[5] + red[7])};
    __syncthreads();
    return r;
}

__device__ __forceinline__ void lnb_load4(const uint16_t *p, float (&v)[4])
{
    const uint2_t u = *reinterpret_cast<const uint2_t *>(p);
    v[0] = bf16lo_to_f32(u.x); v[1] = bf16hi_to_f32(u.x); v[2] = bf16lo_to_f32(u.y); v[3] = bf16hi_to_f32(u.y);
}

// One block per range of `rpb` rows; a thread owns the 4-column chunks t, t + 256, ... of every row.
template <bool DX>
__global__ __launch_bounds__(LNB_THREADS) void ln_bwd_kernel(const uint16_t *__restrict__ x, int ldx, const float *__restrict__ dz, int ldz,
                                                             const uint16_t *__restrict__ gamma, uint16_t *__restrict__ dx, int lddx,
                                                             float *__restrict__ part, long rows, int C, int rpb, float eps)
{
    extern __shared__ __attribute__((aligned(16))) float lsm[];   // [C] sum dz xhat, [C] sum dz of this block's rows, [8] reduction
    float *pg = lsm, *pb = lsm + C, *red = lsm + 2 * C;
    const int nch = C >> 2, t = threadIdx.x;
    for (int c = t; c < nch; c += LNB_THREADS) {
        *reinterpret_cast<float4_t *>(pg + 4 * c) = (float4_t){0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<float4_t *>(pb + 4 * c) = (float4_t){0.f, 0.f, 0.f, 0.f};
    }
    const float invC = 1.f / (float)C;
    const long r0 = (long)blockIdx.x * rpb, r1 = std::min(rows, r0 + rpb);
    for (long r = r0; r < r1; ++r) {
        const uint16_t *xr = x + r * ldx;
        const float *zr = dz + r * ldz;
        float s = 0.f;
        for (int c = t; c < nch; c += LNB_THREADS) {
            float v[4];
            lnb_load4(xr + 4 * c, v);
            s += (v[0] + v[1]) + (v[2] + v[3]);
        }
        const float mean = lnb_block_sum2(s, 0.f, red).x * invC;
        float q = 0.f;
        for (int c = t; c < nch; c += LNB_THREADS) {
            float v[4];
            lnb_load4(xr + 4 * c, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) q = fmaf(v[e] - mean, v[e] - mean, q);
        }
        const float rstd = rsqrtf(lnb_block_sum2(q, 0.f, red).x * invC + eps);
        float sg = 0.f, sgx = 0.f;
        for (int c = t; c < nch; c += LNB_THREADS) {
            float v[4], gm[4];
            lnb_load4(xr + 4 * c, v);
            lnb_load4(gamma + 4 * c, gm);
            const float4_t z = *reinterpret_cast<const float4_t *>(zr + 4 * c);
            float4_t ag = *reinterpret_cast<const float4_t *>(pg + 4 * c), ab = *reinterpret_cast<const float4_t *>(pb + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (v[e] - mean) * rstd, g = z[e] * gm[e];
                sg += g;
                sgx = fmaf(g, xh, sgx);
                ag[e] = fmaf(z[e], xh, ag[e]);
                ab[e] += z[e];
            }
            *reinterpret_cast<float4_t *>(pg + 4 * c) = ag;
            *reinterpret_cast<float4_t *>(pb + 4 * c) = ab;
        }
        if (DX) {
            const float2_t tot = lnb_block_sum2(sg, sgx, red);
            const float mg = tot.x * invC, mgx = tot.y * invC;
            for (int c = t; c < nch; c += LNB_THREADS) {
                float v[4], gm[4], o[4];
                lnb_load4(xr + 4 * c, v);
                lnb_load4(gamma + 4 * c, gm);
                const float4_t z = *reinterpret_cast<const float4_t *>(zr + 4 * c);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float xh = (v[e] - mean) * rstd;
                    o[e] = rstd * (z[e] * gm[e] - mg - xh * mgx);
                }
                *reinterpret_cast<uint2_t *>(dx + r * lddx + 4 * c) = (uint2_t){pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
            }
        }
    }
    __syncthreads();
    float *pp = part + (size_t)blockIdx.x * 2 * C;
    for (int i = t; i < 2 * nch; i += LNB_THREADS) *reinterpret_cast<float4_t *>(pp + 4 * i) = *reinterpret_cast<const float4_t *>(lsm + 4 * i);
}

// grad_w[c] = sum_b part[b][0][c], grad_b[c] = sum_b part[b][1][c], b = 0 .. nb-1 in order
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float *__restrict__ part, int nb, int C, uint16_t *gw, uint16_t *gb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * C) return;
    float s = part[i];
    for (int b = 1; b < nb; ++b) s += part[(size_t)b * 2 * C + i];
    if (i < C) {
        if (gw) gw[i] = f32_to_bf16(s);
    } else if (gb) {
        gb[i - C] = f32_to_bf16(s);
    }
}

void ln_bwd_plan(long rows, int *nb, int *rpb)
{
    const long b = std::max(1L, std::min<long>(rows, device_cus()));
    *rpb = (int)((rows + b - 1) / b);
    *nb = *rpb > 0 ? (int)((rows + *rpb - 1) / *rpb) : 1;
}

}  // namespace

int transpose_bf16_launch(const uint16_t *w, int ldw, uint16_t *wt, int ldt, int R, int C, hipStream_t st)
{
    VLLM_REQUIRE(w && wt && R > 0 && C > 0 && R % TR_T == 0 && C % TR_T == 0 && ldw >= C && ldt >= R && ldw % 8 == 0 && ldt % 8 == 0 &&
                     aligned16(w) && aligned16(wt), "transpose_bf16: R=%d, C=%d must be multiples of 64, 16-byte aligned rows", R, C);
    VLLM_LAUNCH(transpose_bf16_kernel, dim3((unsigned)(C / TR_T), (unsigned)(R / TR_T)), dim3(256), 0, st, w, ldw, wt, ldt);
    VLLM_CHECK_LAUNCH("transpose_bf16_kernel");
    return VLLM_OK;
}

long ln_bwd_workspace_bytes(long rows, int C)
{
    if (rows < 0 || C <= 0) return -1;
    int nb, rpb;
    ln_bwd_plan(rows, &nb, &rpb);
    return (long)nb * 2 * C * 4;
}

int ln_bwd_launch(const uint16_t *x, int ldx, const float *dz, int ldz, const uint16_t *gamma, float eps, long rows, int C,
                  uint16_t *dx, int lddx, uint16_t *grad_w, uint16_t *grad_b, void *ws, long ws_bytes, hipStream_t st)
{
    VLLM_REQUIRE(x && dz && gamma, "layernorm_backward: null pointer");
    VLLM_REQUIRE(rows >= 0 && C > 0 && C % 64 == 0 && C <= LNB_MAX_C, "layernorm_backward: C=%d must be a multiple of 64 and <= %d", C, LNB_MAX_C);
    VLLM_REQUIRE(ldx >= C && ldz >= C && ldx % 4 == 0 && ldz % 4 == 0 && (!dx || (lddx >= C && lddx % 4 == 0)),
                 "layernorm_backward: row strides must be >= C and multiples of 4");
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(x) & 7u) == 0 && (reinterpret_cast<uintptr_t>(gamma) & 7u) == 0 && aligned16(dz) &&
                     (reinterpret_cast<uintptr_t>(dx) & 7u) == 0 && (reinterpret_cast<uintptr_t>(grad_w) & 1u) == 0 &&
                     (reinterpret_cast<uintptr_t>(grad_b) & 1u) == 0,
                 "layernorm_backward: x, weight, grad_x 8-byte aligned, grad_y 16-byte aligned");
    if (rows == 0) {   // no rows: the parameter gradients are zero sums
        if (grad_w) VLLM_REQUIRE(hipMemsetAsync(grad_w, 0, (size_t)C * 2, st) == hipSuccess, "layernorm_backward: memset failed");
        if (grad_b) VLLM_REQUIRE(hipMemsetAsync(grad_b, 0, (size_t)C * 2, st) == hipSuccess, "layernorm_backward: memset failed");
        return VLLM_OK;
    }
    int nb, rpb;
    ln_bwd_plan(rows, &nb, &rpb);
    const long need = (long)nb * 2 * C * 4;
    VLLM_REQUIRE(ws && ws_bytes >= need && aligned16(ws), "layernorm_backward: workspace too small or misaligned (%ld < %ld bytes)", ws_bytes, need);
    const size_t lds = ((size_t)2 * C + 8) * sizeof(float);
    static unsigned long long attr_mask = 0;
    if (first_use_on_device(&attr_mask)) {
        const int mx = (int)(((size_t)2 * LNB_MAX_C + 8) * sizeof(float));
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ln_bwd_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, mx);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&ln_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, mx);
    }
    float *part = reinterpret_cast<float *>(ws);
    if (dx) VLLM_LAUNCH((ln_bwd_kernel<true>), dim3((unsigned)nb), dim3(LNB_THREADS), lds, st, x, ldx, dz, ldz, gamma, dx, lddx, part, rows, C, rpb, eps);
    else VLLM_LAUNCH((ln_bwd_kernel<false>), dim3((unsigned)nb), dim3(LNB_THREADS), lds, st, x, ldx, dz, ldz, gamma, dx, lddx, part, rows, C, rpb, eps);
    VLLM_CHECK_LAUNCH("ln_bwd_kernel");
    if (grad_w || grad_b) {
        VLLM_LAUNCH(ln_bwd_reduce_kernel, dim3((unsigned)ceil_div(2L * C, 256)), dim3(256), 0, st, part, nb, C, grad_w, grad_b);
        VLLM_CHECK_LAUNCH("ln_bwd_reduce_kernel");
    }
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" long vllm_layernorm_backward_workspace_bytes(long rows, int C) { return ln_bwd_workspace_bytes(rows, C); }

extern "C" int vllm_layernorm_backward_bf16(const uint16_t *x, int ldx, const float *grad_y, int ldg, const uint16_t *weight, float eps,
                                            long rows, int C, uint16_t *grad_x, int ldgx, uint16_t *grad_w, uint16_t *grad_b,
                                            void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    return ln_bwd_launch(x, ldx, grad_y, ldg, weight, eps, rows, C, grad_x, ldgx, grad_w, grad_b, workspace, workspace_bytes,
                         (hipStream_t)stream);
}
