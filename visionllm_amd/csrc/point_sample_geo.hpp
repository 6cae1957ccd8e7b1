// Corner geometry of the region encoder's bilinear point sampling, shared by the forward (point_sample.hip) and the backward
// (point_sample_bwd.hip) so that the backward's weights are the forward's bit for bit.
// ATen's arithmetic (grid_sampler_unnormalize / bilinear with per-corner bounds, GridSampler.h): g = 2*c - 1,
// ix = ((g + 1) * W - 1) / 2, corners floor(ix), floor(ix)+1, a corner outside the map contributes nothing.
#pragma once
#include "common.hpp"

namespace vllm {
namespace {

struct PsCorner {
    int x0, y0;
    float w00, w01, w10, w11;   // weights of (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1), zero where out of the map
    bool any;
};

__device__ __forceinline__ PsCorner ps_corner(float cx, float cy, int H, int W)
{
    PsCorner k;
    const float gx = 2.0f * cx - 1.0f, gy = 2.0f * cy - 1.0f;
    const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
    // NaN / inf / far-away coordinates never reach address arithmetic
    const bool fin = ix > -2.f && iy > -2.f && ix < (float)W + 1.f && iy < (float)H + 1.f;
    const float fx = fin ? floorf(ix) : 0.f, fy = fin ? floorf(iy) : 0.f;
    k.x0 = (int)fx; k.y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy;
    const bool xl = fin && k.x0 >= 0 && k.x0 < W, xh = fin && k.x0 + 1 >= 0 && k.x0 + 1 < W;
    const bool yl = k.y0 >= 0 && k.y0 < H, yh = k.y0 + 1 >= 0 && k.y0 + 1 < H;
    k.w00 = (xl && yl) ? (1.f - tx) * (1.f - ty) : 0.f;
    k.w01 = (xh && yl) ? tx * (1.f - ty) : 0.f;
    k.w10 = (xl && yh) ? (1.f - tx) * ty : 0.f;
    k.w11 = (xh && yh) ? tx * ty : 0.f;
    k.any = (xl || xh) && (yl || yh);
    return k;
}

// Round 5: both kernels evaluate a point's corner geometry ONCE and walk a chunk of channels with it (rounds 1-4: one thread per
// output element -- ~40 VALU of coordinate arithmetic per 4 loads and a store: 0.12 / 0.04 of the HBM roofline at the region
// encoder's shapes, profiles/r05_bench_line.json).  The zero-weight guards (a NaN at a clamped address must not get through a zero
// weight) are selects on the loaded values.
struct PsGeo {
    int o00, o01, o10, o11;     // clamped element offsets inside a plane
    float w00, w01, w10, w11;
};
__device__ __forceinline__ PsGeo ps_geo(float cx, float cy, int H, int W)
{
    const PsCorner k = ps_corner(cx, cy, H, W);
    PsGeo g;
    const int x0 = min(max(k.x0, 0), W - 1), x1 = min(max(k.x0 + 1, 0), W - 1);
    const int y0 = min(max(k.y0, 0), H - 1), y1 = min(max(k.y0 + 1, 0), H - 1);
    g.o00 = y0 * W + x0; g.o01 = y0 * W + x1; g.o10 = y1 * W + x0; g.o11 = y1 * W + x1;
    g.w00 = k.any ? k.w00 : 0.f; g.w01 = k.any ? k.w01 : 0.f; g.w10 = k.any ? k.w10 : 0.f; g.w11 = k.any ? k.w11 : 0.f;
    return g;
}

constexpr int PS_CCH = 16;      // channel planes a block stages / a thread walks
constexpr int PS_LDS_MAX = 48 * 1024;   // the planes of a block in LDS when they fit (24 x 24 x 16 x 4 B = 36 KiB at the region encoder's shape)
constexpr float PS_FIX_SCALE = 1099511627776.0f;   // 2^40: the pixel-weight scatters add corner weights as 64-bit integers of this scale

}  // namespace
}  // namespace vllm
