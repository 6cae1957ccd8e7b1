// MSDA forward: dispatcher of the LDS-tiled kernels for the encoder self-attention case (queries == pyramid pixels, Lq == S).
//
// Which kernel serves which call (one forward kernel per geometry class; the other generations are in tools/experiments/ with
// their measurements in NOTES/):
//   * nested level maps (exact 2x pyramids and ceil- / floor-divided halves), fp32 values:  generation 9, msda_tiled9.hip;
//   * any other geometry, fp32 values:                                                      generation 4, msda_tiled4.hip;
//   * bf16 values (vllm_msda_forward_bf16, exact 2x pyramids):                              generation 6, msda_tiled6.hip;
//   * every other shape (decoder queries, D != 32, P != 4, fp64, tensors beyond 32-bit offsets): the gather kernels, msda.hip.
// The host may know the geometry (VLLM_GEO_*: one launch); if it does not, generation 9 and generation 4 are enqueued back to back
// and each checks the shape tensor on the device -- exactly one of them does the work, no host synchronisation.
#include "common.hpp"
#include "kernels.hpp"
#include "msda_sample.hpp"

namespace vllm {

constexpr int MT_MAXL = 8;

bool msda_tiled_ok(int D, int L, int P, int Lq, int S, int B, int M, const void *value, const void *out, const void *loc)
{
    // (the tiled kernels keep pixel / pair offsets in 32 bits: larger tensors take the gather kernel, whose indices are 64-bit)
    const bool fits32 = (long)S * M * 32 < (1L << 30) && (long)B * Lq * M * L * P * 2 < (1L << 30);
    return msda_tiled_enabled() && fits32 && D == 32 && P == 4 && L <= MT_MAXL && Lq == S && Lq >= 4096 && aligned16(value) && aligned16(out) &&
           (reinterpret_cast<uintptr_t>(loc) & 7u) == 0;
}

// D == 32, P == 4, L <= 4, Lq == S, 32-bit pair / pixel offsets (the pyramid-item kernels: generations 6 and 9); 16-byte aligned
// tensors are checked by the caller
bool msda_pyramid_items_ok(int D, int L, int P, int Lq, int S, int B, int M)
{
    return D == 32 && P == 4 && L >= 1 && L <= 4 && Lq == S && Lq >= 4096 && (long)S * M * 32 < (1L << 29) &&
           (long)B * Lq * M * L * P * 2 < (1L << 30);
}

int msda_tiled4_launch(const float *value, const int64_t *shapes, const int64_t *lsi, const float *loc,
                       const float *attw, int B, int S, int M, int L, int Lq, float *out, bool skip_nested,
                       hipStream_t st);   // msda_tiled4.hip
int msda_tiled9_launch(const float *value, const int64_t *shapes, const int64_t *lsi, const float *loc, const float *attw,
                       int B, int S, int M, int L, int Lq, float *out, int prof, hipStream_t st, uint16_t *out16, int hinted,
                       int which);   // msda_tiled9.hip

// Generation 9 (pyramid items, two teams of six waves half a period apart) does the work when the level maps are nested halves
// -- it checks that on the device, from the shape tensor, and returns at once otherwise -- and the generation-4 launch behind it
// skips such maps, so exactly one of the two runs whatever the geometry, without a host synchronisation.  "msda_tiled" = 21
// runs generation 9's phase-clock build (vllm_debug_counters).
int msda_tiled_launch(const float *value, const int64_t *shapes, const int64_t *lsi, const float *loc,
                      const float *attw, int B, int S, int M, int L, int Lq, int P, float *out, hipStream_t st, uint16_t *out16,
                      int *wrote16, int geometry)
{
    // out16 (optional): where a caller that wants the result in bf16 would like it.  *wrote16 = 1 tells it that a pyramid
    // geometry's result went THERE (and `out` was left alone); any other geometry's result is in `out` as usual.
    if (wrote16) *wrote16 = 0;
    // geometry (VLLM_GEO_*): what the HOST knows about the level maps.  UNKNOWN: both kernels are enqueued and the device
    // picks (no host synchronisation; one ~5 us empty launch); PYRAMID / NESTED / GENERAL: exactly one launch.
    if (msda_pyramid_items_ok(32, L, P, Lq, S, B, M) && aligned16(loc) && aligned16(attw) && geometry != VLLM_GEO_GENERAL) {
        if (out16 && wrote16) *wrote16 = 1; else out16 = nullptr;
        // host hint: PYRAMID = exact halves, NESTED = halves rounded either way (one launch each); UNKNOWN: the device decides
        const int hinted = geometry == VLLM_GEO_PYRAMID || geometry == VLLM_GEO_NESTED;
        const int which = geometry == VLLM_GEO_PYRAMID ? 1 : geometry == VLLM_GEO_NESTED ? 2 : 3;
        if (int e = msda_tiled9_launch(value, shapes, lsi, loc, attw, B, S, M, L, Lq, out, msda_tiled_enabled() == 21, st, out16, hinted,
                                       which))
            return e;
        if (hinted) return VLLM_OK;
        return msda_tiled4_launch(value, shapes, lsi, loc, attw, B, S, M, L, Lq, out, true, st);
    }
    return msda_tiled4_launch(value, shapes, lsi, loc, attw, B, S, M, L, Lq, out, false, st);
}

}  // namespace vllm
