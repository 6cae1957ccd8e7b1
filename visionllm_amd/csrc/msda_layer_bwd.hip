// The elementwise kernels of the deformable-attention layer's backward (orchestrated by msda_layer_train.cpp).  All three are HBM-bound:
// one read of every input, one write of every output, 16-byte accesses per lane where the shape allows, no LDS, no atomics.
//   msda_prep_bwd_kernel     the backward of msda_prep_kernel (msda_layer.hip): from the operator's grad_loc / grad_attw and the saved
//                            softmax weights to the gradient of the sampling_offsets / attention_weights linears' OUTPUT, as one bf16
//                            row [offsets | logits | zero pad] -- the dY operand of the two GEMMs over the concatenated linears
//   f32_to_bf16_masked_kernel  grad_value fp32 -> bf16 with the padded keys' rows as zeros (the backward of the key-padding zero fill)
//   bf16_to_f32_kernel       a bf16-saved value widened for the fp32 operator backward (lossless)
#include "common.hpp"
#include "msda_layer.hpp"

namespace vllm {
namespace {

// (sx, sy) of location = ref + offset * (sx, sy): the same three forms, the same arithmetic as msda_prep_kernel
__device__ __forceinline__ void offset_scale(const float *r, float W, float H, int P, int ref_dim, int four_d, float &sx, float &sy)
{
    if (ref_dim == 2) { sx = 1.f / W; sy = 1.f / H; }
    else if (four_d) { sx = r[2] * 0.5f / W; sy = r[3] * 0.5f / H; }
    else { sx = r[2] * 0.5f / (float)P; sy = r[3] * 0.5f / (float)P; }
}

// The forward's mapping: one thread per (row, head, level); its P points are contiguous in every operand (P * 2 location gradients,
// P weight gradients, P weights), the L threads of a (row, head) sit in consecutive lanes and add up the softmax dot product with
// shuffles.  L is a power of two <= 8, P is 4 or 8: the thread reads 16-byte vectors and stores P * 2 bf16 offsets as 16-byte vectors
// (the logits as 8 bytes with P = 4).  The (M * L) threads of a row share out the row's pad columns, 4 at a time (3 M L P is a
// multiple of 4 here and npad one of 64).
template <int P, int L>
__global__ __launch_bounds__(256) void msda_prep_bwd_kernel(const float *__restrict__ gl, const float *__restrict__ gw,
                                                            const float *__restrict__ w, const float *__restrict__ ref,
                                                            const int64_t *__restrict__ shapes, long RM, int M, int ref_dim, int four_d,
                                                            uint16_t *__restrict__ dq, int npad)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;   // ((row * M + m) * L + l)
    const bool live = t < RM * L;
    const long tt = live ? t : RM * L - 1;
    const int l = (int)(tt % L);
    const long rm = tt / L, row = rm / M;
    const int m = (int)(rm - row * M);
    float sx, sy;
    offset_scale(ref + (row * L + l) * ref_dim, (float)shapes[2 * l + 1], (float)shapes[2 * l], P, ref_dim, four_d, sx, sy);
    float o[P * 2], g[P], a[P];
#pragma unroll
    for (int i = 0; i < P * 2; i += 4) {
        const float4_t v = *reinterpret_cast<const float4_t *>(gl + tt * (P * 2) + i);
        o[i] = v[0]; o[i + 1] = v[1]; o[i + 2] = v[2]; o[i + 3] = v[3];
    }
#pragma unroll
    for (int i = 0; i < P; i += 4) {
        const float4_t v = *reinterpret_cast<const float4_t *>(gw + tt * P + i);
        const float4_t u = *reinterpret_cast<const float4_t *>(w + tt * P + i);
        g[i] = v[0]; g[i + 1] = v[1]; g[i + 2] = v[2]; g[i + 3] = v[3];
        a[i] = u[0]; a[i + 1] = u[1]; a[i + 2] = u[2]; a[i + 3] = u[3];
    }
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < P; ++i) dot += g[i] * a[i];
#pragma unroll
    for (int d = 1; d < L; d <<= 1) dot += __shfl_xor(dot, d);
    if (!live) return;
    const int MLP = M * L * P, ml = m * L + l;
    uint16_t *qrow = dq + row * npad;
    uint32_t po[P], pg[P / 2];
#pragma unroll
    for (int i = 0; i < P; ++i) po[i] = pack_bf16x2(o[2 * i] * sx, o[2 * i + 1] * sy);
#pragma unroll
    for (int i = 0; i < P; i += 2) pg[i / 2] = pack_bf16x2(a[i] * (g[i] - dot), a[i + 1] * (g[i + 1] - dot));
#pragma unroll
    for (int i = 0; i < P; i += 4) {
        const uint4_t v = {po[i], po[i + 1], po[i + 2], po[i + 3]};
        *reinterpret_cast<uint4_t *>(qrow + ml * (P * 2) + 2 * i) = v;
    }
    if (P == 4) {
        const uint2_t v = {pg[0], pg[1]};
        *reinterpret_cast<uint2_t *>(qrow + 2 * MLP + ml * P) = v;
    } else {
#pragma unroll
        for (int i = 0; i < P / 2; i += 4) {
            const uint4_t v = {pg[i], pg[i + 1], pg[i + 2], pg[i + 3]};
            *reinterpret_cast<uint4_t *>(qrow + 2 * MLP + ml * P + 2 * i) = v;
        }
    }
    const uint2_t zero = {0u, 0u};
    for (int c = 3 * MLP + 4 * ml; c < npad; c += 4 * M * L) *reinterpret_cast<uint2_t *>(qrow + c) = zero;
}

// Any L, P: one thread per (row, head); the M threads of a row share out the pad columns.
__global__ __launch_bounds__(256) void msda_prep_bwd_generic_kernel(const float *__restrict__ gl, const float *__restrict__ gw,
                                                                    const float *__restrict__ w, const float *__restrict__ ref,
                                                                    const int64_t *__restrict__ shapes, long RM, int M, int L, int P,
                                                                    int ref_dim, int four_d, uint16_t *__restrict__ dq, int npad)
{
    const long rm = (long)blockIdx.x * 256 + threadIdx.x;
    if (rm >= RM) return;
    const long row = rm / M;
    const int m = (int)(rm - row * M), MLP = M * L * P;
    const float *g = gw + rm * L * P, *a = w + rm * L * P, *o = gl + rm * L * P * 2;
    uint16_t *qrow = dq + row * npad;
    uint16_t *qo = qrow + (long)m * L * P * 2, *qg = qrow + 2 * MLP + (long)m * L * P;
    float dot = 0.f;
    for (int i = 0; i < L * P; ++i) dot += g[i] * a[i];
    for (int l = 0; l < L; ++l) {
        float sx, sy;
        offset_scale(ref + (row * L + l) * ref_dim, (float)shapes[2 * l + 1], (float)shapes[2 * l], P, ref_dim, four_d, sx, sy);
        for (int p = 0; p < P; ++p) {
            const int i = l * P + p;
            qo[2 * i] = f32_to_bf16(o[2 * i] * sx);
            qo[2 * i + 1] = f32_to_bf16(o[2 * i + 1] * sy);
            qg[i] = f32_to_bf16(a[i] * (g[i] - dot));
        }
    }
    for (int c = 3 * MLP + m; c < npad; c += M) qrow[c] = 0;
}

// Grid-stride over 16-byte input vectors; the row of a vector is one 32-bit division (the launcher keeps the vector count below 2^31).
__global__ __launch_bounds__(256) void f32_to_bf16_masked_kernel(const float *__restrict__ src, uint16_t *__restrict__ dst, unsigned n4,
                                                                 unsigned c4, const uint8_t *__restrict__ mask)
{
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const float4_t v = reinterpret_cast<const float4_t *>(src)[i];
        uint2_t o;
        o.x = pack_bf16x2(v[0], v[1]);
        o.y = pack_bf16x2(v[2], v[3]);
        if (mask && mask[i / c4]) { o.x = 0u; o.y = 0u; }   // (a select: a NaN in a padded key's row does not get through)
        reinterpret_cast<uint2_t *>(dst)[i] = o;
    }
}

// Any row length and element alignment: one element per thread step.
__global__ __launch_bounds__(256) void f32_to_bf16_masked_scalar_kernel(const float *__restrict__ src, uint16_t *__restrict__ dst, long n,
                                                                        long cols, const uint8_t *__restrict__ mask)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        dst[i] = (mask && mask[i / cols]) ? (uint16_t)0 : f32_to_bf16(src[i]);
}

// 8 elements per thread step: one 16-byte read, two 16-byte writes.
__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const uint16_t *__restrict__ src, float *__restrict__ dst, long n8, long n)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const uint4_t v = reinterpret_cast<const uint4_t *>(src)[i];
        const float4_t lo = {bf16lo_to_f32(v[0]), bf16hi_to_f32(v[0]), bf16lo_to_f32(v[1]), bf16hi_to_f32(v[1])};
        const float4_t hi = {bf16lo_to_f32(v[2]), bf16hi_to_f32(v[2]), bf16lo_to_f32(v[3]), bf16hi_to_f32(v[3])};
        reinterpret_cast<float4_t *>(dst)[2 * i] = lo;
        reinterpret_cast<float4_t *>(dst)[2 * i + 1] = hi;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long k = n8 * 8; k < n; ++k) dst[k] = bf16_to_f32(src[k]);
}

inline unsigned stream_grid(long items) { const long b = (items + 255) / 256; return (unsigned)(b < 1 ? 1 : b < 8192 ? b : 8192); }

}  // namespace

int msda_prep_bwd_launch(const float *gl, const float *gw, const float *w, const float *ref, const int64_t *shapes, long R, int M, int L,
                         int P, int ref_dim, int four_d, uint16_t *dq, int npad, hipStream_t st)
{
    VLLM_REQUIRE(R >= 0 && M > 0 && L > 0 && P > 0 && (ref_dim == 2 || ref_dim == 4), "msda_prep_backward: bad sizes");
    const long RM = R * M, MLP = (long)M * L * P;
    VLLM_REQUIRE(npad >= 3 * MLP && 3 * MLP < (1L << 30), "msda_prep_backward: row stride %d < 3 * M * L * P = %ld", npad, 3 * MLP);
    if (RM == 0) return VLLM_OK;
    VLLM_REQUIRE(gl && gw && w && ref && shapes && dq, "msda_prep_backward: null pointer");
    VLLM_REQUIRE(RM * L < (1L << 38), "msda_prep_backward: too many rows");
    // the vector form: 16-byte aligned operands and a row stride that keeps every row's start so
    const bool vec = aligned16(gl) && aligned16(gw) && aligned16(w) && aligned16(dq) && npad % 8 == 0;
#define GO(PP, LL)                                                                                                                    \
    VLLM_LAUNCH((msda_prep_bwd_kernel<PP, LL>), dim3((unsigned)ceil_div(RM * LL, 256)), dim3(256), 0, st, gl, gw, w, ref, shapes, RM, M, \
                ref_dim, four_d, dq, npad)
    if (vec && P == 4 && L == 4) GO(4, 4);
    else if (vec && P == 4 && L == 1) GO(4, 1);
    else if (vec && P == 4 && L == 2) GO(4, 2);
    else if (vec && P == 4 && L == 8) GO(4, 8);
    else if (vec && P == 8 && L == 4) GO(8, 4);
    else
        VLLM_LAUNCH(msda_prep_bwd_generic_kernel, dim3((unsigned)ceil_div(RM, 256)), dim3(256), 0, st, gl, gw, w, ref, shapes, RM, M, L, P,
                    ref_dim, four_d, dq, npad);
#undef GO
    VLLM_CHECK_LAUNCH("msda_prep_bwd_kernel");
    return VLLM_OK;
}

int f32_to_bf16_masked_launch(const float *src, uint16_t *dst, long rows, int cols, const uint8_t *mask, hipStream_t st)
{
    VLLM_REQUIRE(rows >= 0 && cols > 0, "f32_to_bf16_masked: bad sizes");
    const long n = rows * cols;
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(src && dst, "f32_to_bf16_masked: null pointer");
    if (cols % 4 == 0 && aligned16(src) && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0 && n / 4 < (1L << 31)) {
        VLLM_LAUNCH(f32_to_bf16_masked_kernel, dim3(stream_grid(n / 4)), dim3(256), 0, st, src, dst, (unsigned)(n / 4), (unsigned)(cols / 4), mask);
    } else {
        VLLM_LAUNCH(f32_to_bf16_masked_scalar_kernel, dim3(stream_grid(n)), dim3(256), 0, st, src, dst, n, (long)cols, mask);
    }
    VLLM_CHECK_LAUNCH("f32_to_bf16_masked_kernel");
    return VLLM_OK;
}

int bf16_to_f32_launch(const uint16_t *src, float *dst, long n, hipStream_t st)
{
    VLLM_REQUIRE(n >= 0, "bf16_to_f32: bad size");
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(src && dst && aligned16(src) && aligned16(dst), "bf16_to_f32: src and dst must be 16-byte aligned device pointers");
    VLLM_LAUNCH(bf16_to_f32_kernel, dim3(stream_grid(n / 8)), dim3(256), 0, st, src, dst, n / 8, n);
    VLLM_CHECK_LAUNCH("bf16_to_f32_kernel");
    return VLLM_OK;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_msda_prep_backward_f32(const float *grad_loc, const float *grad_attw, const float *attw, const float *ref,
                                           const int64_t *shapes, long R, int M, int L, int P, int ref_dim, int four_d, uint16_t *dq,
                                           int npad, vllm_stream_t stream)
{
    return msda_prep_bwd_launch(grad_loc, grad_attw, attw, ref, shapes, R, M, L, P, ref_dim, four_d, dq, npad, (hipStream_t)stream);
}

extern "C" int vllm_f32_to_bf16_masked(const float *src, uint16_t *dst, long rows, int cols, const uint8_t *row_mask, vllm_stream_t stream)
{
    return f32_to_bf16_masked_launch(src, dst, rows, cols, row_mask, (hipStream_t)stream);
}

extern "C" int vllm_bf16_to_f32(const uint16_t *src, float *dst, long n, vllm_stream_t stream)
{
    return bf16_to_f32_launch(src, dst, n, (hipStream_t)stream);
}
