// Host-side scaffolding shared by the orchestrators (vit.cpp, layer_train.cpp, bridge_train.cpp, region_train.cpp, embed_train.hip,
// msda_layer.hip, msda_layer_train.cpp, dcnv3_layer.hip, deform_encoder_layer.hip, deform_decoder_layer.hip, deform_decoder.hip, query_select.hip, fusion_layer.cpp, gdino_encoder.hip, gdino_inputs.hip): the
// pieces every entry point that strings kernels together on the caller's stream used to copy from the one before.  Host code only.
#pragma once
#include <initializer_list>
#include "kernels.hpp"

#define TRY(x) do { const int rc__ = (x); if (rc__ != VLLM_OK) return rc__; } while (0)

namespace vllm {

inline long align256(long x) { return (x + 255) & ~255L; }

// Carves a workspace into 256-byte aligned pieces: take() answers the offset of the next piece; `off` behind the last one is the total.
struct Carver {
    long off = 0;
    long take(long bytes) { const long o = off; off += align256(bytes); return o; }
};

// true where [a, a + abytes) and [b, b + bbytes) share a byte (either pointer null: false)
inline bool ranges_overlap(const void *a, long abytes, const void *b, long bbytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a && b && a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// what the row kernels ask of an operand of rows of C bf16: 16-byte aligned base, row stride a multiple of 8 and >= C
inline bool row_operand_ok(const void *p, int ld, int C) { return aligned16(p) && ld >= C && ld % 8 == 0; }

// The flags of the stream-K scratch are zeroed once per orchestrated call (kernels.hpp, SK_FLAG_BYTES); a call without scratch has none.
inline int sk_scratch_reset(void *sk, hipStream_t st, const char *who)
{
    if (sk) VLLM_REQUIRE(hipMemsetAsync(sk, 0, SK_FLAG_BYTES, st) == hipSuccess, "%s: flag reset failed", who);
    return VLLM_OK;
}

// "No rows: every gradient is an empty sum" -- zero `elements` bf16 values at each non-null pointer, in the order given.
struct Bf16Span { uint16_t *p; long elements; };
inline int zero_bf16(hipStream_t st, const char *who, std::initializer_list<Bf16Span> spans)
{
    for (const Bf16Span &e : spans)
        if (e.p) VLLM_REQUIRE(hipMemsetAsync(e.p, 0, (size_t)e.elements * 2, st) == hipSuccess, "%s: memset failed", who);
    return VLLM_OK;
}

// Input gradient of a Linear with weight W [out, in] (dense rows): dX [M, in] = epilogue(dY [M, out] W), as the bf16 GEMM on W^T, which is
// written into wt [in, out] first.  `pre` is the saved pre-activation [M, in] of EPI_GELU_BWD / EPI_QUICK_GELU_BWD (null otherwise); dX is fp32 for EPI_F32.
inline int linear_dgrad(hipStream_t st, int epi, const uint16_t *dY, const uint16_t *W, int out, int in, long M, uint16_t *wt, void *dX,
                        const uint16_t *pre, void *sk, long sk_bytes)
{
    TRY(transpose_bf16_launch(W, in, wt, out, out, in, st));
    GemmArgs a = gemm_args(dY, out, wt, out, nullptr, static_cast<uint16_t *>(dX), in, M, in, out);
    if (pre) { a.res = pre; a.ldr = in; }
    gemm_set_scratch(a, sk, sk_bytes);
    return gemm_bf16_launch(epi, a, st);
}

// Attention over packed qkv: q and k are the first two column blocks of the [B S, 3C] slab `qk`, v the third of the slab `qkv` (the same
// slab, unless a QK-norm has written q / k elsewhere); out [B, S, H, D]; `lse` [B, H, S] in the training forward only.
inline AttnArgs packed_qkv_attn(const uint16_t *qk, const uint16_t *qkv, uint16_t *out, int B, int S, int H, int D, float scale,
                                float *lse = nullptr)
{
    const int C = H * D;
    AttnArgs a;
    a.q = qk; a.k = qk + C; a.v = qkv + 2 * C; a.out = out;
    a.q_bs = a.k_bs = a.v_bs = (long)S * 3 * C;
    a.q_ts = a.k_ts = a.v_ts = 3 * C;
    a.q_hs = a.k_hs = a.v_hs = D;
    a.B = B; a.S = S; a.H = H; a.nqt = 0;
    a.scale_log2e = scale * 1.4426950408889634f;
    a.lse = lse;
    return a;
}

}  // namespace vllm
