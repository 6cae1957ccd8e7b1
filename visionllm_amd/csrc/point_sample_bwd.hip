// Region-encoder point sampling, BACKWARD with respect to the feature map.
// Replaces the autograd of visionllmv2/model/region_encoder.py:135-140 (F.grid_sample's backward: one float atomic add per
// (point, corner, channel), then the division's and the sum's backward).
//
// Masked mean (the trained path).  The forward is linear in the map (point_sample.hip, round 6):
//     out[n, c] = (1 / cnt_n) sum_pix A[n, pix] in[n, c, pix],     A[n, pix] = sum over the valid points of the corner weight on pix
// so the gradient is an OUTER PRODUCT
//     grad_in[n, c, pix] = (A[n, pix] / cnt_n) * grad_out[n, c]                       (0 for every pix when cnt_n == 0)
// Every element is written exactly once: no atomics on the output, no zero-fill by the caller, the same bits on every run.  It does
// not read the map.  A region without a valid point gets ZEROS -- the derivative of the constant 0 the forward returns there; the
// reference's autograd puts NaN on every pixel one of the region's (invalid) points touches (the division's backward is
// 0 * (1 / 0)).  Deliberate departure.
// A is rebuilt exactly as the forward builds it (ps_geo's weights, 2^40-scaled 64-bit integer atomics: they commute, hence
// deterministic; a corner weight below 2^-40 contributes neither to the forward nor to the gradient).  Three roundings follow: A to
// float, / cnt, * grad_out; the bf16 output is that fp32 product rounded to nearest even once.
//   * maps whose accumulators fit in LDS (the forward's pixel-weight form): ONE launch, grid (channel chunks, N).  A block rebuilds
//     A[n, .] in LDS and streams its chunk grad_in[n, c0 : c0 + cpb, :] -- one contiguous range of memory -- with 16-byte stores.
//     The chunk is sized on the host so that the launch has about PMB_BLOCKS blocks (measured: see there).  fp32, 16 regions x 3072
//     channels x 24 x 24: 22.2 us = 0.81 of the 6.29 TB/s store roof; bf16 14.3 us.
//   * larger maps (80 x 80, ...): A in the caller's workspace with 64-bit integer vector atomics on global memory (memset, scatter,
//     then the same store stream reading A from global).
//
// Unfused point_sample backward (grad_out [N, C, P] -> grad_in [N, C, H, W]; nothing in the model trains through this entry):
// a block (region, PS_CCH channels) accumulates its planes in LDS with float atomics and stores them once, fully written.  Maps that
// do not fit take float atomics on global memory into an output this entry clears itself.  Both SUM IN ARRIVAL ORDER: the last bits
// may differ between runs.
#include "common.hpp"
#include "point_sample_geo.hpp"

namespace vllm {
namespace {

// Blocks the one-launch masked-mean backward aims for: the host picks channels per block = N C / PMB_BLOCKS (a multiple of 8 in
// [8, PMB_CPB_MAX]).  A block's rebuild of A (P points: coordinate arithmetic + 4 LDS atomics each) is redundant work, its stores are
// not.  Decided by measurement (profiles/region_train.txt, 16 regions x 24 x 24 x 2304 points): 256 blocks -- 192 channels per block
// at C = 3072, 64 at C = 1024 -- is fastest or level for fp32 and bf16 at both (22.2 / 11.8 us fp32); 1024 blocks lose up to 5 us to
// the rebuilds, 128 leave CUs idle at C = 1024, and a one-launch precompute of A into the workspace (the large-map form below, forced
// with -DPMB_LDS_MAX=0) costs ~10 us more: three stream operations instead of one.
#ifndef PMB_BLOCKS
#define PMB_BLOCKS 256
#endif
// LDS budget of the one-launch form (-DPMB_LDS_MAX=0 builds a library that always takes the workspace form, for timing it)
#ifndef PMB_LDS_MAX
#define PMB_LDS_MAX PS_LDS_MAX
#endif
constexpr int PMB_CPB_MAX = 256;

template <typename T> struct PsOut;
template <> struct PsOut<float> {
    static __device__ __forceinline__ void store1(float *p, float v) { *p = v; }
    static __device__ __forceinline__ void store4(float *p, const float *v)
    {
        const float4_t o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<float4_t *>(p) = o;
    }
};
template <> struct PsOut<uint16_t> {
    static __device__ __forceinline__ void store1(uint16_t *p, float v) { *p = f32_to_bf16(v); }
    static __device__ __forceinline__ void store4(uint16_t *p, const float *v)
    {
        const uint2_t o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
        *reinterpret_cast<uint2_t *>(p) = o;
    }
    static __device__ __forceinline__ void store8(uint16_t *p, const float *v)
    {
        const uint4_t o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
        *reinterpret_cast<uint4_t *>(p) = o;
    }
};
// VEC consecutive pixels of one channel: w * g (a zero weight stays zero whatever grad_out holds), rounded once, one store
template <typename T, int VEC>
__device__ __forceinline__ void psb_store(T *p, const float *w, float g)
{
    float v[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = w[k] != 0.f ? w[k] * g : 0.f;
    if constexpr (VEC == 1) PsOut<T>::store1(p, v[0]);
    else if constexpr (VEC == 4) PsOut<T>::store4(p, v);
    else PsOut<T>::store8(p, v);
}
__device__ __forceinline__ float psb_weight(unsigned long long acc, int cnt)
{
    const float a = (float)((double)acc * (1.0 / 1099511627776.0));
    return cnt > 0 ? a / (float)cnt : 0.f;
}

// One launch: grid (ceil(C / cpb), N), PMB_THREADS threads.  LDS: [HW] 64-bit sums, [HW] float weights, [cpb] grad_out values.
// VEC pixels per store: 4 (fp32: 16 bytes; bf16: 8 bytes) or 8 (bf16: 16 bytes) where H W % VEC == 0 and grad_in is aligned, else 1.
// The rebuild of A is a latency chain (valid -> coordinates -> LDS atomics) in front of the store stream: a thread loads PMB_BATCH
// points' operands at once, so the region encoder's 2304 points are ONE round trip to memory per block (one point per loop
// iteration in 256-thread blocks: 26.5 us instead of 22.4 at 16 x 3072 x 24 x 24 with the same chunks, profiles/region_train.txt).
constexpr int PMB_THREADS = 512, PMB_BATCH = 8;
template <typename T, int VEC>
__global__ __launch_bounds__(PMB_THREADS) void point_sample_mean_bwd_kernel(const float *__restrict__ coords, const uint8_t *__restrict__ valid,
                                                                            const float *__restrict__ grad_out, T *__restrict__ grad_in,
                                                                            int C, int H, int W, int P, int cpb)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long pb_acc[];
    __shared__ int s_cnt;
    const int HW = H * W, tid = threadIdx.x, lane = tid & 63;
    float *Wt = reinterpret_cast<float *>(pb_acc + ((HW + 1) & ~1));
    float *gs = Wt + ((HW + 3) & ~3);
    const int c0 = blockIdx.x * cpb;
    const long n = blockIdx.y;
    const int nc = min(cpb, C - c0);
    for (int i = tid; i < HW; i += PMB_THREADS) pb_acc[i] = 0ull;
    for (int c = tid; c < nc; c += PMB_THREADS) gs[c] = grad_out[n * C + c0 + c];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int cnt = 0;
    for (int p0 = tid; p0 < P; p0 += PMB_THREADS * PMB_BATCH) {
        float2_t xy[PMB_BATCH];
        bool ok[PMB_BATCH];
#pragma unroll
        for (int u = 0; u < PMB_BATCH; ++u) {
            const int p = p0 + u * PMB_THREADS;
            const bool in = p < P;
            const long q = n * P + (in ? p : p0);       // (p0 < P: a valid address for the lanes past the end)
            ok[u] = in && valid[q];
            xy[u] = *reinterpret_cast<const float2_t *>(coords + q * 2);
        }
#pragma unroll
        for (int u = 0; u < PMB_BATCH; ++u) {
            if (!ok[u]) continue;
            const PsGeo g = ps_geo(xy[u].x, xy[u].y, H, W);
            ++cnt;
            if (g.w00 != 0.f) atomicAdd(pb_acc + g.o00, (unsigned long long)(g.w00 * PS_FIX_SCALE));
            if (g.w01 != 0.f) atomicAdd(pb_acc + g.o01, (unsigned long long)(g.w01 * PS_FIX_SCALE));
            if (g.w10 != 0.f) atomicAdd(pb_acc + g.o10, (unsigned long long)(g.w10 * PS_FIX_SCALE));
            if (g.w11 != 0.f) atomicAdd(pb_acc + g.o11, (unsigned long long)(g.w11 * PS_FIX_SCALE));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    const int tc = s_cnt;
    for (int i = tid; i < HW; i += PMB_THREADS) Wt[i] = psb_weight(pb_acc[i], tc);
    __syncthreads();
    // the chunk's planes are one contiguous range: vector v of it is pixels (v % HWV) * VEC ... of channel v / HWV
    const int HWV = HW / VEC;
    const long total = (long)nc * HWV;
    T *dst = grad_in + (n * C + c0) * (long)HW;
    int c = tid / HWV, i = tid - c * HWV;
    const int dc = PMB_THREADS / HWV, di = PMB_THREADS - dc * HWV;
    for (long v = tid; v < total; v += PMB_THREADS) {
        float w[VEC];
        if constexpr (VEC == 1) w[0] = Wt[i];
        else {
#pragma unroll
            for (int k = 0; k < VEC; k += 4) {
                const float4_t q = *reinterpret_cast<const float4_t *>(Wt + i * VEC + k);
                w[k] = q[0]; w[k + 1] = q[1]; w[k + 2] = q[2]; w[k + 3] = q[3];
            }
        }
        psb_store<T, VEC>(dst + v * VEC, w, gs[c]);
        c += dc; i += di;
        if (i >= HWV) { i -= HWV; ++c; }
    }
}

// ---- maps too large for the LDS accumulators: A and the counts in the workspace ----
// grid (ceil(P / 256), N): one thread per point
__global__ __launch_bounds__(256) void point_sample_scatter_weights_kernel(const float *__restrict__ coords, const uint8_t *__restrict__ valid,
                                                                           unsigned long long *__restrict__ acc, int *__restrict__ cnts,
                                                                           int H, int W, int P)
{
    const long n = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    if (p < P && valid[n * P + p]) {
        const float2_t xy = *reinterpret_cast<const float2_t *>(coords + (n * P + p) * 2);
        const PsGeo g = ps_geo(xy.x, xy.y, H, W);
        unsigned long long *a = acc + n * (long)H * W;
        cnt = 1;
        if (g.w00 != 0.f) atomicAdd(a + g.o00, (unsigned long long)(g.w00 * PS_FIX_SCALE));
        if (g.w01 != 0.f) atomicAdd(a + g.o01, (unsigned long long)(g.w01 * PS_FIX_SCALE));
        if (g.w10 != 0.f) atomicAdd(a + g.o10, (unsigned long long)(g.w10 * PS_FIX_SCALE));
        if (g.w11 != 0.f) atomicAdd(a + g.o11, (unsigned long long)(g.w11 * PS_FIX_SCALE));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(cnts + n, cnt);
}
// grid (ceil(C / cpb), N): a thread keeps the weights of VEC pixels in registers and walks the chunk's channels
template <typename T, int VEC>
__global__ __launch_bounds__(256) void point_sample_mean_bwd_ws_kernel(const unsigned long long *__restrict__ acc, const int *__restrict__ cnts,
                                                                       const float *__restrict__ grad_out, T *__restrict__ grad_in, int C,
                                                                       int HW, int cpb)
{
    __shared__ float gs[PMB_CPB_MAX];
    const int c0 = blockIdx.x * cpb;
    const long n = blockIdx.y;
    const int nc = min(cpb, C - c0);
    for (int c = threadIdx.x; c < nc; c += 256) gs[c] = grad_out[n * C + c0 + c];
    __syncthreads();
    const int tc = cnts[n];
    const unsigned long long *a = acc + n * (long)HW;
    T *dst = grad_in + (n * C + c0) * (long)HW;
    for (int i = threadIdx.x * VEC; i < HW; i += 256 * VEC) {
        float w[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) w[k] = psb_weight(a[i + k], tc);
        for (int c = 0; c < nc; ++c) psb_store<T, VEC>(dst + (long)c * HW + i, w, gs[c]);
    }
}

// ---- unfused: grad_in[n, c, pix] = sum_p w(p, pix) grad_out[n, c, p] ----
// LDS = true: grid (ceil(C / PS_CCH), N), the block's planes in LDS (float atomics), stored once.  LDS = false: the same walk with
// float atomics on the (cleared) output.
template <bool LDS>
__global__ __launch_bounds__(256) void point_sample_bwd_kernel(const float *__restrict__ coords, const float *__restrict__ grad_out,
                                                               float *__restrict__ grad_in, int C, int H, int W, int P)
{
    extern __shared__ __attribute__((aligned(16))) float pb_planes[];
    const int c0 = blockIdx.x * PS_CCH;
    const long n = blockIdx.y;
    const int HW = H * W, nc = min(PS_CCH, C - c0);
    float *planes_g = grad_in + (n * C + c0) * (long)HW;
    if (LDS) {
        for (int i = threadIdx.x; i < nc * HW; i += 256) pb_planes[i] = 0.f;
        __syncthreads();
    }
    float *planes = LDS ? pb_planes : planes_g;
    for (int p = threadIdx.x; p < P; p += 256) {
        const float2_t xy = *reinterpret_cast<const float2_t *>(coords + (n * P + p) * 2);
        const PsGeo g = ps_geo(xy.x, xy.y, H, W);
        const float *go = grad_out + (n * C + c0) * (long)P + p;
        for (int c = 0; c < nc; ++c) {
            const float v = go[(long)c * P];
            float *pl = planes + (long)c * HW;
            if (g.w00 != 0.f) atomicAdd(pl + g.o00, g.w00 * v);
            if (g.w01 != 0.f) atomicAdd(pl + g.o01, g.w01 * v);
            if (g.w10 != 0.f) atomicAdd(pl + g.o10, g.w10 * v);
            if (g.w11 != 0.f) atomicAdd(pl + g.o11, g.w11 * v);
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nc * HW; i += 256) planes_g[i] = pb_planes[i];
    }
}

inline size_t pmb_lds_bytes(long HW, int cpb) { return (size_t)((HW + 1) & ~1L) * 8 + (size_t)((HW + 3) & ~3L) * 4 + (size_t)cpb * 4; }
inline bool pmb_one_launch(long HW) { return pmb_lds_bytes(HW, PMB_CPB_MAX) <= (size_t)(PMB_LDS_MAX); }
inline long pmb_workspace(long N, long HW) { return ((N * HW * 8 + N * 4) + 15) & ~15L; }
inline int pmb_cpb(long N, int C)
{
    long cpb = (N * C / (PMB_BLOCKS) + 7) & ~7L;
    cpb = cpb < 8 ? 8 : cpb > PMB_CPB_MAX ? PMB_CPB_MAX : cpb;
    return (int)cpb;
}

template <typename T>
int mean_backward(const char *who, const float *coords, const uint8_t *valid, const float *grad_out, int N, int C, int H, int W, int P,
                  T *grad_in, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    VLLM_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && P >= 0, "%s: bad sizes", who);
    if ((long)N * C == 0) return VLLM_OK;
    VLLM_REQUIRE(grad_out && grad_in && (P == 0 || (coords && valid)), "%s: null pointer", who);
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(coords) & 7u) == 0, "%s: coords must be 8-byte aligned", who);
    VLLM_REQUIRE(N <= 65535 && (long)H * W < (1L << 24), "%s: too many regions / too large a map for one launch", who);
    const long HW = (long)H * W;
    hipStream_t st = (hipStream_t)stream;
    const int cpb = pmb_cpb(N, C);
    const dim3 grid((unsigned)ceil_div(C, cpb), (unsigned)N);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(grad_in);
    // elements per store: 16-byte stores where the planes allow (bf16: 8 pixels), 4 pixels where only that fits, else single elements
    const int vec = (sizeof(T) == 2 && HW % 8 == 0 && (addr & 15u) == 0) ? 8 : (HW % 4 == 0 && (addr & (4 * sizeof(T) - 1)) == 0) ? 4 : 1;
    if (pmb_one_launch(HW)) {
        const size_t lds = pmb_lds_bytes(HW, cpb);
#define PMB_GO(V) VLLM_LAUNCH((point_sample_mean_bwd_kernel<T, V>), grid, dim3(PMB_THREADS), lds, st, coords, valid, grad_out, grad_in, C, H, W, P, cpb)
        if constexpr (sizeof(T) == 2) { if (vec == 8) PMB_GO(8); else if (vec == 4) PMB_GO(4); else PMB_GO(1); }
        else { if (vec == 4) PMB_GO(4); else PMB_GO(1); }
#undef PMB_GO
        VLLM_CHECK_LAUNCH("point_sample_mean_bwd_kernel");
        return VLLM_OK;
    }
    const long need = pmb_workspace(N, HW);
    VLLM_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace of %ld bytes needed (vllm_point_sample_backward_workspace_bytes)", who, need);
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, "%s: workspace must be 8-byte aligned", who);
    unsigned long long *acc = static_cast<unsigned long long *>(workspace);
    int *cnts = reinterpret_cast<int *>(acc + (long)N * HW);
    if (hipMemsetAsync(workspace, 0, (size_t)need, st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return VLLM_ELAUNCH;
    }
    if (P > 0) {
        VLLM_LAUNCH(point_sample_scatter_weights_kernel, dim3((unsigned)ceil_div(P, 256), (unsigned)N), dim3(256), 0, st, coords, valid, acc, cnts, H, W, P);
        VLLM_CHECK_LAUNCH("point_sample_scatter_weights_kernel");
    }
#define PMB_GO(V) VLLM_LAUNCH((point_sample_mean_bwd_ws_kernel<T, V>), grid, dim3(256), 0, st, acc, cnts, grad_out, grad_in, C, (int)HW, cpb)
    if constexpr (sizeof(T) == 2) { if (vec == 8) PMB_GO(8); else if (vec == 4) PMB_GO(4); else PMB_GO(1); }
    else { if (vec == 4) PMB_GO(4); else PMB_GO(1); }
#undef PMB_GO
    VLLM_CHECK_LAUNCH("point_sample_mean_bwd_ws_kernel");
    return VLLM_OK;
}

}  // namespace
}  // namespace vllm

using namespace vllm;

extern "C" long vllm_point_sample_backward_workspace_bytes(int N, int C, int H, int W, int P)
{
    (void)P;
    if (N < 0 || C <= 0 || H <= 0 || W <= 0 || P < 0) {
        set_error("point_sample_backward_workspace_bytes: bad sizes");
        return VLLM_EINVAL;
    }
    const long HW = (long)H * W;
    if ((long)N * C == 0 || pmb_one_launch(HW)) return 0;
    return pmb_workspace(N, HW);
}

extern "C" int vllm_point_sample_mean_backward_f32(const float *coords, const uint8_t *valid, const float *grad_out, int N, int C, int H,
                                                   int W, int P, float *grad_in, void *workspace, long workspace_bytes,
                                                   vllm_stream_t stream)
{
    return mean_backward<float>("point_sample_mean_backward", coords, valid, grad_out, N, C, H, W, P, grad_in, workspace, workspace_bytes, stream);
}

extern "C" int vllm_point_sample_mean_backward_bf16(const float *coords, const uint8_t *valid, const float *grad_out, int N, int C, int H,
                                                    int W, int P, uint16_t *grad_in, void *workspace, long workspace_bytes,
                                                    vllm_stream_t stream)
{
    return mean_backward<uint16_t>("point_sample_mean_backward", coords, valid, grad_out, N, C, H, W, P, grad_in, workspace, workspace_bytes, stream);
}

extern "C" int vllm_point_sample_backward_f32(const float *coords, const float *grad_out, int N, int C, int H, int W, int P,
                                              float *grad_in, void *workspace, long workspace_bytes, vllm_stream_t stream)
{
    (void)workspace; (void)workspace_bytes;   // (none needed: the large-map form accumulates into grad_in itself)
    VLLM_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && P >= 0, "point_sample_backward: bad sizes");
    if ((long)N * C == 0) return VLLM_OK;
    VLLM_REQUIRE(grad_in && (P == 0 || (coords && grad_out)), "point_sample_backward: null pointer");
    VLLM_REQUIRE((reinterpret_cast<uintptr_t>(coords) & 7u) == 0, "point_sample_backward: coords must be 8-byte aligned");
    VLLM_REQUIRE(N <= 65535 && (long)H * W < (1L << 24), "point_sample_backward: too many regions / too large a map for one launch");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)PS_CCH * H * W * sizeof(float);
    const dim3 grid((unsigned)ceil_div(C, PS_CCH), (unsigned)N);
    if (lds <= (size_t)PS_LDS_MAX) {
        VLLM_LAUNCH((point_sample_bwd_kernel<true>), grid, dim3(256), lds, st, coords, grad_out, grad_in, C, H, W, P);
    } else {
        if (hipMemsetAsync(grad_in, 0, (size_t)N * C * H * W * sizeof(float), st) != hipSuccess) {
            set_error("point_sample_backward: hipMemsetAsync failed");
            return VLLM_ELAUNCH;
        }
        if (P == 0) return VLLM_OK;
        VLLM_LAUNCH((point_sample_bwd_kernel<false>), grid, dim3(256), 0, st, coords, grad_out, grad_in, C, H, W, P);
    }
    VLLM_CHECK_LAUNCH("point_sample_bwd_kernel");
    return VLLM_OK;
}
