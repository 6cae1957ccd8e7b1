// Launch interface of region_stem.hip for its orchestrator (region_train.cpp).  Host code only.
#pragma once
#include "common.hpp"

namespace vllm {

constexpr int REGION_MAX_LEVELS = 4, REGION_MAX_MAPS = REGION_MAX_LEVELS + 1;

// pooled[n, c] = sum_m sum_pix w[m][n, pix] x[m][n, pix, c]: map 0 is the stem, maps 1 .. the levels, each with its own strides (elements)
struct RegionPoolArgs {
    const uint16_t *x[REGION_MAX_MAPS] = {};
    const float *w[REGION_MAX_MAPS] = {};
    long row_stride[REGION_MAX_MAPS] = {}, img_stride[REGION_MAX_MAPS] = {};
    uint16_t *out = nullptr;   // [n, C]
    int maps = 0, HW = 0, C = 0;
};

int region_im2col_launch(const void *images, const void *masks, int is_f32, uint16_t *A, int n, int H, int W, int k, int Kpad, hipStream_t st);
bool ln_gelu_takes(int C);
int ln_gelu_launch(const uint16_t *x, int ldx, const uint16_t *w, const uint16_t *b, uint16_t *pre, uint16_t *y, long rows, int C, float eps,
                   hipStream_t st);
// [R, (c, q)] -> [R, (q, c)] with q in 0 .. 3 (K = 4 C1 columns); inverse = 1: back
int region_wperm_launch(const uint16_t *src, uint16_t *dst, int R, int K, int inverse, hipStream_t st);
bool region_pool_weights_fit(long HW);
int region_pool_weights_launch(const float *coords, const uint8_t *valid, float *w, int n, int L, int H, int W, int P, hipStream_t st);
int region_pool_launch(const RegionPoolArgs &a, int n, hipStream_t st);
int region_outer_launch(const float *w, const uint16_t *g, uint16_t *out, int n, int HW, int C, hipStream_t st);

}  // namespace vllm
