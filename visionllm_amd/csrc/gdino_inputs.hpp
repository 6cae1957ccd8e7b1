// The geometry that the kernels and the orchestrator of gdino_inputs.hip share: the levels of the encoder's input as a kernel argument, and
// the sizes that both the size query and the call compute.  Host and device.
#pragma once
#include "common.hpp"

namespace vllm {

constexpr int GI_MAX_LEVELS = 8;    // struct VllmGdinoInputsDesc's arrays
constexpr int GN_GROUPS = 32;       // nn.GroupNorm(32, d_model)
constexpr int GN_SLAB_ROWS = 32;    // rows of one {count, mean, M2} partial

// H_l x W_l cells per level and the row at which the level starts inside an image's S rows; a kernel argument by value
struct LevelGeo {
    int L;
    int h[GI_MAX_LEVELS], w[GI_MAX_LEVELS];
    int start[GI_MAX_LEVELS];
    int S;
};

// a 3 x 3 / stride 2 / padding 1 conv's output extent
static inline int conv3s2_extent(int n) { return (n - 1) / 2 + 1; }

static inline long gn_slabs(long HW) { return (HW + GN_SLAB_ROWS - 1) / GN_SLAB_ROWS; }

}  // namespace vllm
