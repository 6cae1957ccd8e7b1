// The row group: G lanes of a wave share a row of C <= 8 G bf16 elements (G 32: two rows per wave, G 64: one) and lane j of the group owns
// the 16-byte chunk j, so a row is one load per lane whatever C is; lanes behind the row's last chunk carry zeros through the reductions.
// A wave walks its row groups with a grid stride.  The body of add_layernorm_kernel (deform_encoder_layer.hip), box_refine_kernel
// (deform_decoder.hip), qs_norm_kernel and qs_tail_kernel (query_select.hip): the lane geometry, the fixed xor tree, the LayerNorm of a
// chunk, the four fused dot products, and the launch geometry.  The loops -- what a row reads, whether the next group is asked for before
// the current one is reduced -- stay in the kernels.
#pragma once
#include "common.hpp"

namespace vllm {

constexpr int ROWG_THREADS = 256;

// {G, workgroups} for rows of C: G 32 up to C 256, else 64; four waves a workgroup, a row group per wave, at most 8 workgroups per CU
struct RowGroupPlan { int G; unsigned grid; };
static inline RowGroupPlan row_group_plan(long rows, int C)
{
    const int G = C <= 256 ? 32 : 64;
    const long ngroups = (rows + 64 / G - 1) / (64 / G), want = (ngroups + 3) / 4, cap = (long)device_cus() * 8;
    return {G, (unsigned)(want < cap ? want : cap)};
}
// launches kernel<32> or kernel<64> by the plan of (rows, C) and returns VLLM_ELAUNCH from the enclosing function where that fails
#define VLLM_LAUNCH_ROW_GROUPS(kernel, rows, C, st, ...)                                                            \
    do {                                                                                                            \
        const ::vllm::RowGroupPlan p__ = ::vllm::row_group_plan(rows, C);                                           \
        if (p__.G == 32) VLLM_LAUNCH((kernel<32>), dim3(p__.grid), dim3(::vllm::ROWG_THREADS), 0, st, __VA_ARGS__); \
        else VLLM_LAUNCH((kernel<64>), dim3(p__.grid), dim3(::vllm::ROWG_THREADS), 0, st, __VA_ARGS__);             \
        VLLM_CHECK_LAUNCH(#kernel);                                                                                 \
    } while (0)

#ifdef __HIPCC__
// a thread's place: lane j of sub-row `sub` of its wave's group; the wave's first group and the stride of its walk
template <int G> struct RowLanes {
    static constexpr int R = 64 / G;   // rows of a group
    int j, sub, c0;                    // c0: the first element of the lane's chunk
    bool act;                          // the chunk lies inside the row
    long wave0, nwaves, ngroups;
    __device__ __forceinline__ RowLanes(long rows, int C)
    {
        const int lane = threadIdx.x & 63;
        j = lane % G;
        sub = lane / G;
        nwaves = (long)gridDim.x * (ROWG_THREADS / 64);
        wave0 = (long)blockIdx.x * (ROWG_THREADS / 64) + (threadIdx.x >> 6);
        ngroups = (rows + R - 1) / R;
        act = j < (C >> 3);
        c0 = j * 8;
    }
    __device__ __forceinline__ long row(long g) const { return g * R + sub; }
};

// sums over the G lanes of a row, in every lane: one fixed xor tree for the N values, step by step
template <int G, int N> __device__ __forceinline__ void group_sum(float (&s)[N])
{
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] += __shfl_xor(s[k], o);
    }
}
template <int G> __device__ __forceinline__ float group_sum(float s)
{
    float t[1] = {s};
    group_sum<G, 1>(t);
    return t[0];
}

// once per wave: the lane's chunks of gamma and beta as floats; zeros behind the row's last chunk
template <int G>
__device__ __forceinline__ void load_affine(const uint16_t *__restrict__ w, const uint16_t *__restrict__ b, const RowLanes<G> &ln,
                                            float (&gw)[8], float (&gb)[8])
{
    uint4_t wv = {0u, 0u, 0u, 0u}, bv = {0u, 0u, 0u, 0u};
    if (ln.act) { wv = *reinterpret_cast<const uint4_t *>(w + ln.c0); bv = *reinterpret_cast<const uint4_t *>(b + ln.c0); }
    unpack8(wv, gw);
    unpack8(bv, gb);
}
// once per wave: the lane's 4 x 8 slice of W [4, C] and, in lanes j < 4, bias[j]
template <int G>
__device__ __forceinline__ float load_dot4(const uint16_t *__restrict__ W, const uint16_t *__restrict__ bias, int C, const RowLanes<G> &ln,
                                           float (&w)[4][8])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint4_t wv = {0u, 0u, 0u, 0u};
        if (ln.act) wv = *reinterpret_cast<const uint4_t *>(W + (long)k * C + ln.c0);
        unpack8(wv, w[k]);
    }
    return ln.j < 4 ? bf16_to_f32(bias[ln.j]) : 0.f;
}

// LayerNorm of a row from the lanes' eight fp32 values, fp32 from the sum to the one rounding, the second moment taken about the mean
// (norm_bf16_kernel), in two steps.  layernorm_center: every lane of the group must be here; centres v and returns 1 / std.
// layernorm_chunk: the lane's eight outputs packed, for the lanes that store (under the caller's own condition: the compiler fuses the
// multiply-adds of a block, so where this stands decides the rounding).
template <int G> __device__ __forceinline__ float layernorm_center(float (&v)[8], bool act, float invC, float eps)
{
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[e];
    const float mean = group_sum<G>(s) * invC;
    float m2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = act ? v[e] - mean : 0.f; m2 += v[e] * v[e]; }
    return 1.0f / sqrtf(group_sum<G>(m2) * invC + eps);
}
__device__ __forceinline__ uint4_t layernorm_chunk(const float (&v)[8], float rstd, const float (&gw)[8], const float (&gb)[8])
{
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = v[e] * rstd * gw[e] + gb[e];
    return pack8(o8);
}

// s[k] = h . W[k, :] for k = 0 .. 3 over the row from the lanes' chunks, in every lane of the group (which must all be here);
// dot4_pick: component j for lane j < 4, the one it finishes
template <int G> __device__ __forceinline__ void dot4_rows(const uint4_t &x, const float (&w)[4][8], float (&s)[4])
{
    float v[8];
    unpack8(x, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s[k] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s[k] = fmaf(v[e], w[k][e], s[k]);
    }
    group_sum<G, 4>(s);
}
__device__ __forceinline__ float dot4_pick(const float (&s)[4], int j) { return j == 0 ? s[0] : j == 1 ? s[1] : j == 2 ? s[2] : s[3]; }
#endif

}  // namespace vllm
