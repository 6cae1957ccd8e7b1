// The deformable ENCODER LAYER around the deformable-attention layer (msda_layer.hip) for bf16 modules at inference:
//   query = src + pos -> self_attn(query, reference_points, src) -> src + attn -> norm1 -> linear1 -> act -> linear2 -> + -> norm2
// Reference: DeformableTransformerEncoderLayer.forward  unipose/modeling_unipose.py:3132-3186;
//            GroundingDinoDeformableLayer.forward       grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1105-1180.
//
// One call, one stream, a caller workspace.  The launches, in order:
//   add_bf16_kernel        query = src + pos            (only the first layer of a chain: the others get it from the layer in front)
//   the attention layer    msda_layer_run, whose output_proj adds `src` in its epilogue (EPI_RESIDUAL)
//   add_layernorm_kernel   norm1, in place
//   per slab of rows:      linear1 + ReLU / GELU (EPI_RELU / EPI_GELU), linear2 + residual (EPI_RESIDUAL)
//   add_layernorm_kernel   norm2 -> out, and out + pos -> query_out for the next layer
// The FFN intermediate [rows, d_ffn] is the largest tensor of the call: with the option "deform_enc_ffn_slab_rows" it exists one slab
// of rows at a time, so the workspace holds a slab of it and linear2 finds the slab linear1 has just written in the cache.
#include "common.hpp"
#include <stdlib.h>
#include "orchestrate.hpp"
#include "msda_layer.hpp"
#include "deform_blocks.hpp"
#include "row_groups.hpp"
#include "gdino_encoder.hpp"

namespace vllm {
namespace {

// y = LayerNorm(x + res) * w + b over rows of C <= 8 G elements; y_pos = bf16(bf16(y) + pos).  G lanes share a row (32: two rows per
// wave, 64: one) and lane j of the group owns the 16-byte chunk j, so a row is one load per lane whatever C is; lanes behind the row's
// last chunk carry zeros through the reductions.  A wave walks its rows with a grid stride and asks for the next row's x / res / pos
// before it reduces the current one (the scheme of rms_bwd_kernel, norm.hip): the reductions of one row run under the loads of the
// next.  fp32 from the sum to the one rounding of y; the second moment is taken about the mean (norm_bf16_kernel).  x and y may be
// the same memory: a lane writes the chunk it has read and no other.
struct AlnRow { uint4_t x, r, p; };

template <int G>
__global__ __launch_bounds__(ROWG_THREADS) void add_layernorm_kernel(const uint16_t *x, int ldx, const uint16_t *res, int ldr,
                                                                    const uint16_t *__restrict__ w, const uint16_t *__restrict__ b, uint16_t *y,
                                                                    int ldy, const uint16_t *pos, int ldp, uint16_t *y_pos, int ldq, long rows,
                                                                    int C, float eps)
{
    const RowLanes<G> ln(rows, C);
    const bool act = ln.act;
    const int c0 = ln.c0;
    const long nwaves = ln.nwaves;
    float gw[8], gb[8];
    load_affine<G>(w, b, ln, gw, gb);
    auto load = [&](long g) {
        AlnRow t = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        const long row = ln.row(g);
        if (act && row < rows) {
            t.x = *reinterpret_cast<const uint4_t *>(x + row * ldx + c0);
            if (res) t.r = *reinterpret_cast<const uint4_t *>(res + row * ldr + c0);
            if (y_pos) t.p = *reinterpret_cast<const uint4_t *>(pos + row * ldp + c0);
        }
        return t;
    };
    const float invC = 1.0f / (float)C;
    long g = ln.wave0;
    AlnRow cur = load(g);   // (g >= ngroups: row >= rows, nothing is read)
    for (; g < ln.ngroups; g += nwaves) {
        const AlnRow nxt = load(g + nwaves);
        const long row = ln.row(g);
        float v[8], rr[8];
        unpack8(cur.x, v);
        unpack8(cur.r, rr);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += rr[e];
        const float rstd = layernorm_center<G>(v, act, invC, eps);
        if (act && row < rows) {
            const uint4_t yo = layernorm_chunk(v, rstd, gw, gb);
            *reinterpret_cast<uint4_t *>(y + row * ldy + c0) = yo;
            if (y_pos) {   // from the STORED y: the bits of adding pos to y afterwards
                float ys[8], pp[8];
                unpack8(yo, ys);
                unpack8(cur.p, pp);
#pragma unroll
                for (int e = 0; e < 8; ++e) ys[e] += pp[e];
                *reinterpret_cast<uint4_t *>(y_pos + row * ldq + c0) = pack8(ys);
            }
        }
        cur = nxt;
    }
}

// out = bf16(a + b): 16-byte vectors over the first n8 * 8 elements, the rest one by one (n8 = 0 for operands that are not 16-byte aligned)
__global__ __launch_bounds__(256) void add_bf16_kernel(const uint16_t *__restrict__ a, const uint16_t *__restrict__ b, uint16_t *__restrict__ out,
                                                       long n8, long n)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    for (long i = t; i < n8; i += stride) {
        float fa[8], fb[8];
        unpack8(reinterpret_cast<const uint4_t *>(a)[i], fa);
        unpack8(reinterpret_cast<const uint4_t *>(b)[i], fb);
#pragma unroll
        for (int e = 0; e < 8; ++e) fa[e] += fb[e];
        reinterpret_cast<uint4_t *>(out)[i] = pack8(fa);
    }
    for (long k = n8 * 8 + t; k < n; k += stride) out[k] = f32_to_bf16(bf16_to_f32(a[k]) + bf16_to_f32(b[k]));
}

}  // namespace

int add_layernorm_launch(const uint16_t *x, int ldx, const uint16_t *res, int ldr, const uint16_t *w, const uint16_t *b, uint16_t *y, int ldy,
                         const uint16_t *pos, int ldp, uint16_t *y_pos, int ldq, long rows, int C, float eps, hipStream_t st)
{
    VLLM_LAUNCH_ROW_GROUPS(add_layernorm_kernel, rows, C, st, x, ldx, res, ldr, w, b, y, ldy, pos, ldp, y_pos, ldq, rows, C, eps);
    return VLLM_OK;
}

int add_launch(const uint16_t *a, const uint16_t *b, uint16_t *out, long n, hipStream_t st)
{
    const long n8 = aligned16(a) && aligned16(b) && aligned16(out) ? n / 8 : 0;
    const long work = n8 > 0 ? n8 : n, want = (work + 255) / 256, cap = (long)device_cus() * 16;
    VLLM_LAUNCH(add_bf16_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, a, b, out, n8, n);
    VLLM_CHECK_LAUNCH("add_bf16_kernel");
    return VLLM_OK;
}

int ffn_check(const char *who, const FfnBlock &k)
{
    VLLM_REQUIRE(k.d_ffn > 0 && k.d_ffn % 64 == 0, "%s: d_ffn=%d must be a positive multiple of 64", who, k.d_ffn);
    VLLM_REQUIRE(k.act == 0 || k.act == VLLM_EPI_GELU, "%s: unknown act %d (0 = ReLU, VLLM_EPI_GELU = erf GELU)", who, k.act);
    VLLM_REQUIRE(k.eps >= 0.f, "%s: negative eps", who);
    VLLM_REQUIRE(k.fc1_w && k.fc1_b && k.fc2_w && k.fc2_b && k.norm_w && k.norm_b, "%s: missing weights", who);
    return VLLM_OK;
}

int ffn_block_run(hipStream_t st, const FfnBlock &k, const uint16_t *x, long R, int C, uint16_t *h, long slab_rows, uint16_t *t, uint16_t *out,
                  const uint16_t *pos, uint16_t *y_pos)
{
    const int F = k.d_ffn;
    for (long r0 = 0; r0 < R; r0 += slab_rows) {
        const long m = R - r0 < slab_rows ? R - r0 : slab_rows;
        TRY(gemm(st, k.act == 0 ? EPI_RELU : EPI_GELU, x + r0 * C, C, k.fc1_w, C, k.fc1_b, h, F, (int)m, F, C));
        TRY(gemm(st, EPI_RESIDUAL, h, F, k.fc2_w, F, k.fc2_b, t + r0 * C, C, (int)m, C, F, nullptr, x + r0 * C, C));
    }
    return add_layernorm_launch(t, C, nullptr, 0, k.norm_w, k.norm_b, out, C, y_pos ? pos : nullptr, C, y_pos, C, R, C, k.eps, st);
}

namespace {

// deform_enc_ffn_slab_rows(): rows of the FFN intermediate per slab; 0 = the whole tensor at once, the default: measured at cfg 4, B = 8
// the whole tensor is the fastest of 0 / 65 536 / 16 384 rows (2191 / 2267 / 2360 us per layer, profiles/deform_encoder_layer.txt); a slab
// height is for callers who want the smaller workspace
struct EncWs {
    long t0, x1, h, attn, total;   // t0: the query, later linear2's output; x1: src + attn, normalised in place; h: a slab of the intermediate
    long slab;                     // rows per slab
};
EncWs enc_ws(const VllmDeformEncLayerDesc *d, long B, long S)
{
    const long R = B * S, C = d->attn.d_model, F = d->d_ffn;
    EncWs w;
    // a slab's bytes stay below 2^31 whatever the option says (the GEMMs' 32-bit byte offsets), in whole 256-row tiles
    const long most = (((1L << 31) - 1) / (F * 2) - 256) & ~255L;
    const long opt = deform_enc_ffn_slab_rows();
    w.slab = opt > 0 && opt < R ? opt : R;
    if (w.slab > most) w.slab = most;
    Carver cv;
    w.t0 = cv.take(R * C * 2);
    w.x1 = cv.take(R * C * 2);
    w.h = cv.take(w.slab * F * 2);
    w.attn = cv.take(msda_layer_ws_bytes(&d->attn, (int)B, (int)S, (int)S));
    w.total = cv.off;
    return w;
}

FfnBlock enc_ffn(const VllmDeformEncLayerDesc *d)
{
    return {d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, d->norm2_w, d->norm2_b, d->act, d->d_ffn, d->norm2_eps};
}

}  // namespace

int enc_layer_check_desc(const VllmDeformEncLayerDesc *d)
{
    VLLM_REQUIRE(d, "deform_enc_layer: null descriptor");
    TRY(msda_layer_check_desc(&d->attn));
    VLLM_REQUIRE(d->attn.ref_dim == 2, "deform_enc_layer: ref_dim=%d, the encoder layer takes 2-d reference points", d->attn.ref_dim);
    VLLM_REQUIRE(d->attn.d_model <= 512, "deform_enc_layer: d_model=%d above 512 (the LayerNorm kernel's rows)", d->attn.d_model);
    TRY(ffn_check("deform_enc_layer", enc_ffn(d)));
    VLLM_REQUIRE(d->norm1_eps >= 0.f, "deform_enc_layer: negative eps");
    VLLM_REQUIRE(d->norm1_w && d->norm1_b && d->attn.value_proj_b && d->attn.sampling_offsets_b && d->attn.attention_weights_b &&
                     d->attn.output_proj_b,
                 "deform_enc_layer: missing weights");
    return VLLM_OK;
}

long enc_layer_ws_bytes(const VllmDeformEncLayerDesc *d, int B, int S) { return enc_ws(d, B, S).total; }

int enc_layer_check_call(const VllmDeformEncLayerDesc *d, const uint16_t *src, const uint16_t *pos, const uint16_t *query_in,
                         const float *reference_points, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int S,
                         const uint16_t *out, const uint16_t *query_out, const void *workspace, long workspace_bytes)
{
    VLLM_REQUIRE(src && reference_points && spatial_shapes && level_start_index && out, "deform_enc_layer: null pointer (src / reference_points / spatial_shapes / level_start_index / out)");
    VLLM_REQUIRE(!query_out || pos, "deform_enc_layer: null pointer (query_out needs pos)");
    const VllmMsdaLayerDesc &at = d->attn;
    VLLM_REQUIRE(aligned16(src) && aligned16(pos) && aligned16(query_in) && aligned16(out) && aligned16(query_out) &&
                     (reinterpret_cast<uintptr_t>(reference_points) & 7u) == 0,
                 "deform_enc_layer: misaligned src / pos / query_in / out / query_out (16 bytes) or reference_points (8 bytes)");
    for (const uint16_t *p : {d->norm1_w, d->norm1_b, d->fc1_w, d->fc1_b, d->fc2_w, d->fc2_b, d->norm2_w, d->norm2_b})
        VLLM_REQUIRE(aligned16(p), "deform_enc_layer: misaligned weight or bias (16 bytes)");
    for (const uint16_t *p : msda_weights(at)) VLLM_REQUIRE(aligned16(p), "deform_enc_layer: misaligned weight or bias (16 bytes)");
    const EncWs w = enc_ws(d, B, S);
    VLLM_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.total,
                 "deform_enc_layer: workspace too small (%ld < %ld bytes) or misaligned", workspace_bytes, w.total);
    return VLLM_OK;
}

int enc_layer_run(const VllmDeformEncLayerDesc *d, const uint16_t *src, const uint16_t *pos, const uint16_t *query_in, const float *reference_points,
                  const uint8_t *padding_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int S, uint16_t *out,
                  uint16_t *query_out, void *workspace, hipStream_t st)
{
    const VllmMsdaLayerDesc &at = d->attn;
    const EncWs w = enc_ws(d, B, S);
    char *ws = (char *)workspace;
    const long R = (long)B * S;
    const int C = at.d_model;
    uint16_t *t0 = (uint16_t *)(ws + w.t0), *x1 = (uint16_t *)(ws + w.x1), *h = (uint16_t *)(ws + w.h);
    // 1. the query (modeling_unipose.py:3174 with_pos_embed; ...mask_dn.py:771-772)
    const uint16_t *query = query_in ? query_in : src;
    if (!query_in && pos) { TRY(add_launch(src, pos, t0, R * C, st)); query = t0; }
    // 2. x1 = src + self_attn(query, reference_points, src) (:3174-3176; :1151-1164): the residual goes into output_proj's epilogue
    TRY(msda_layer_run(&at, query, reference_points, src, padding_mask, spatial_shapes, level_start_index, B, S, S, x1,
                       msda_layer_bufs(&at, ws + w.attn, B, S, S), nullptr, st, src));
    // 3. norm1 (:3177; :1165), in place
    TRY(add_layernorm_launch(x1, C, nullptr, 0, d->norm1_w, d->norm1_b, x1, C, nullptr, 0, nullptr, 0, R, C, d->norm1_eps, st));
    // 4. - 6. t0 = x1 + linear2(act(linear1(x1))) (:3167-3168; :1167-1174), a slab of rows at a time (t0 held the query: the attention has read
    // it); norm2 (:3169; :1175) -> out, and the next layer's query out + pos
    return ffn_block_run(st, enc_ffn(d), x1, R, C, h, w.slab, t0, out, pos, query_out);
}

namespace {
long g_calls = 0;
}

}  // namespace vllm

using namespace vllm;

extern "C" int vllm_add_layernorm_bf16(const uint16_t *x, int ldx, const uint16_t *res, int ldr, const uint16_t *weight, const uint16_t *bias,
                                       uint16_t *y, int ldy, const uint16_t *pos, int ldp, uint16_t *y_pos, int ldq, long rows, int C, float eps,
                                       vllm_stream_t stream)
{
    VLLM_REQUIRE(rows >= 0 && C >= 64 && C <= 512 && C % 64 == 0, "add_layernorm: rows=%ld C=%d (C a multiple of 64 in 64 .. 512)", rows, C);
    if (rows == 0) return VLLM_OK;
    VLLM_REQUIRE(x && weight && bias && y && (!y_pos || pos), "add_layernorm: null pointer");
    VLLM_REQUIRE(row_operand_ok(x, ldx, C) && row_operand_ok(y, ldy, C) && (!res || row_operand_ok(res, ldr, C)) &&
                     (!y_pos || (row_operand_ok(pos, ldp, C) && row_operand_ok(y_pos, ldq, C))) && aligned16(weight) && aligned16(bias),
                 "add_layernorm: misaligned operand (16-byte aligned pointers, row strides multiples of 8 and at least C)");
    return add_layernorm_launch(x, ldx, res, ldr, weight, bias, y, ldy, y_pos ? pos : nullptr, ldp, y_pos, ldq, rows, C, eps, (hipStream_t)stream);
}

extern "C" int vllm_add_bf16(const uint16_t *a, const uint16_t *b, uint16_t *out, long n, vllm_stream_t stream)
{
    VLLM_REQUIRE(n >= 0, "add_bf16: negative size");
    if (n == 0) return VLLM_OK;
    VLLM_REQUIRE(a && b && out, "add_bf16: null pointer");
    return add_launch(a, b, out, n, (hipStream_t)stream);
}

extern "C" unsigned long vllm_deform_enc_layer_desc_sizeof(void) { return sizeof(VllmDeformEncLayerDesc); }
extern "C" long vllm_deform_enc_layer_calls(void) { return g_calls; }

extern "C" long vllm_deform_enc_layer_workspace_bytes(const VllmDeformEncLayerDesc *d, int B, int S)
{
    if (enc_layer_check_desc(d) != VLLM_OK) return -1;
    if (B < 0 || S < 0 || (long)B * S >= (1L << 31)) { set_error("deform_enc_layer: B=%d S=%d (0 <= B S < 2^31)", B, S); return -1; }
    if ((long)B * S == 0) return 0;
    return enc_layer_ws_bytes(d, B, S);
}

extern "C" int vllm_deform_enc_layer_forward(const VllmDeformEncLayerDesc *d, const uint16_t *src, const uint16_t *pos, const uint16_t *query_in,
                                             const float *reference_points, const uint8_t *padding_mask, const int64_t *spatial_shapes,
                                             const int64_t *level_start_index, int B, int S, uint16_t *out, uint16_t *query_out, void *workspace,
                                             long workspace_bytes, vllm_stream_t stream)
{
    TRY(enc_layer_check_desc(d));
    VLLM_REQUIRE(B >= 0 && S >= 0 && (long)B * S < (1L << 31), "deform_enc_layer: B=%d S=%d (0 <= B S < 2^31)", B, S);
    if ((long)B * S == 0) return VLLM_OK;
    TRY(enc_layer_check_call(d, src, pos, query_in, reference_points, spatial_shapes, level_start_index, B, S, out, query_out, workspace,
                             workspace_bytes));
    ++g_calls;
    return enc_layer_run(d, src, pos, query_in, reference_points, padding_mask, spatial_shapes, level_start_index, B, S, out, query_out, workspace,
                         (hipStream_t)stream);
}
