// The Grounding-DINO DECODER for bf16 modules at inference, as one call: the loop of GroundingDinoDecoder.forward
// (grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1792-1981) around the decoder layer of deform_decoder_layer.hip.
//
// One call, one stream, a caller workspace.  Per layer, in order:
//   refpoint_embed_kernel   reference_points_input = ref * valid_ratios (fp32) and the sine embedding of its level 0 (bf16)   (:1865-1873)
//   GEMM + ReLU, GEMM       reference_points_head -> query_pos                                                               (:1874)
//   dec_layer_run           the layer's own launches on the running hidden state                                             (:1907-1921)
//   add_layernorm           layer_norm -> intermediate[l]                                                                    (:1939)
//   GEMM + ReLU twice, box_refine_kernel   bbox_embed[l] and the refinement -> intermediate_reference_points[l]              (:1925-1937)
// The outputs are layer-major, so every LayerNorm and refine launch writes one dense block; the hidden state between two layers is the
// un-normed layer output, in two ping-pong buffers; reference points are fp32 throughout.  One layer's workspace serves every layer.
#include "common.hpp"
#include "orchestrate.hpp"
#include "deform_decoder_layer.hpp"
#include "deform_blocks.hpp"
#include "row_groups.hpp"

namespace vllm {
namespace {

// A lane owns 8 consecutive outputs of one sine row ([y | x | w | h] groups of P, P % 8 == 0: a chunk lies in one group), so a row is
// P / 2 lanes and a store 16 bytes.  The lanes of a row also write its L products ref * valid_ratios, one float4 each.  fp32 as the
// module's statements: (v * 2 pi) / dim_t[i] with a true division, the accurate sinf / cosf (arguments reach 2 pi), one rounding.
__global__ __launch_bounds__(256) void refpoint_embed_kernel(const float *__restrict__ ref, const float *__restrict__ vr,
                                                             const float *__restrict__ dim_t, long rows, int Lq, int L, int P,
                                                             float *__restrict__ rpi, uint16_t *__restrict__ sine, int ld)
{
    const int cpr = P >> 1;   // 16-byte chunks per row
    const long total = rows * cpr, stride = (long)gridDim.x * 256;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
        const long row = t / cpr;
        const int j = (int)(t - row * cpr);
        const long b = row / Lq;
        const float4_t r = *reinterpret_cast<const float4_t *>(ref + row * 4);
        const float2_t *vrb = reinterpret_cast<const float2_t *>(vr) + b * L;
        for (int l = j; l < L; l += cpr) {
            const float2_t s = vrb[l];
            *reinterpret_cast<float4_t *>(rpi + (row * L + l) * 4) = (float4_t){r[0] * s[0], r[1] * s[1], r[2] * s[0], r[3] * s[1]};
        }
        const int grp = (j * 8) / P, i0 = j * 8 - grp * P;
        const float2_t s0 = vrb[0];
        // the reference's order of the groups: y, x, w, h
        const float v = grp == 0 ? r[1] * s0[1] : grp == 1 ? r[0] * s0[0] : grp == 2 ? r[2] * s0[0] : r[3] * s0[1];
        const float pos = v * 6.283185307179586f;
        const float4_t d0 = *reinterpret_cast<const float4_t *>(dim_t + i0), d1 = *reinterpret_cast<const float4_t *>(dim_t + i0 + 4);
        float o[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a0 = __fdiv_rn(pos, d0[e]), a1 = __fdiv_rn(pos, d1[e]);
            o[e] = (e & 1) ? cosf(a0) : sinf(a0);
            o[4 + e] = (e & 1) ? cosf(a1) : sinf(a1);
        }
        *reinterpret_cast<uint4_t *>(sine + row * ld + j * 8) = pack8(o);
    }
}

// new_ref[r, k] = sigmoid(h[r, :] . W[k, :] + b[k] + inverse_sigmoid(ref[r, k])), fp32.  Row groups (row_groups.hpp): a lane keeps its
// 4 x 8 slice of W in registers; a wave asks for the next rows' h and ref before it reduces the current ones.  The four sums go through
// one fixed xor tree; lane k < 4 of the group finishes component k.  A lane reads the element of `ref` it writes and no other, and a row
// is read only by the wave that writes it: new_ref may be ref.
struct BrRow { uint4_t x; float r; };

template <int G>
__global__ __launch_bounds__(ROWG_THREADS) void box_refine_kernel(const uint16_t *__restrict__ h, int ldh, const uint16_t *__restrict__ W,
                                                                const uint16_t *__restrict__ bias, const float *ref, float *new_ref, long rows,
                                                                int C, float eps)
{
    const RowLanes<G> ln(rows, C);
    const int j = ln.j;
    const bool fin = j < 4;
    const long nwaves = ln.nwaves;
    float w[4][8];
    const float bk = load_dot4<G>(W, bias, C, ln, w);
    auto load = [&](long g) {
        BrRow t = {{0u, 0u, 0u, 0u}, 0.5f};
        const long row = ln.row(g);
        if (row < rows) {
            if (ln.act) t.x = *reinterpret_cast<const uint4_t *>(h + row * ldh + ln.c0);
            if (fin) t.r = ref[row * 4 + j];
        }
        return t;
    };
    long g = ln.wave0;
    BrRow cur = load(g);   // (g >= ngroups: row >= rows, nothing is read)
    for (; g < ln.ngroups; g += nwaves) {
        const BrRow nxt = load(g + nwaves);
        const long row = ln.row(g);
        float s[4];
        dot4_rows<G>(cur.x, w, s);
        if (fin && row < rows) {
            const float dot = dot4_pick(s, j);
            float x = cur.r;
            x = x < 0.f ? 0.f : x > 1.f ? 1.f : x;          // comparisons: a NaN stays a NaN, as in torch.clamp
            const float x1 = x < eps ? eps : x, om = 1.f - x, x2 = om < eps ? eps : om;
            const float z = dot + bk + logf(__fdiv_rn(x1, x2));
            new_ref[row * 4 + j] = __fdiv_rn(1.f, 1.f + expf(-z));
        }
        cur = nxt;
    }
}

int refpoint_embed_launch(const float *ref, const float *vr, const float *dim_t, long rows, int Lq, int L, int P, float *rpi, uint16_t *sine,
                          int ld, hipStream_t st)
{
    const long want = (rows * (P / 2) + 255) / 256, cap = (long)device_cus() * 8;
    VLLM_LAUNCH(refpoint_embed_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, ref, vr, dim_t, rows, Lq, L, P, rpi, sine, ld);
    VLLM_CHECK_LAUNCH("refpoint_embed_kernel");
    return VLLM_OK;
}

int box_refine_launch(const uint16_t *h, int ldh, const uint16_t *W, const uint16_t *b, const float *ref, float *new_ref, long rows, int C,
                      float eps, hipStream_t st)
{
    VLLM_LAUNCH_ROW_GROUPS(box_refine_kernel, rows, C, st, h, ldh, W, b, ref, new_ref, rows, C, eps);
    return VLLM_OK;
}

struct DecoderWs {
    long layer, layer_bytes;   // one layer's workspace, the largest of the layers', reused by every layer
    long hid[2];               // the running hidden state [R, C], ping-pong
    long sine, t1, t2, qpos;   // sine [R, 4P]; the MLPs' intermediates [R, C]; query_pos [R, C]
    long rpi;                  // reference_points_input [R, L, 4] fp32
    long total;
};
DecoderWs decoder_ws(const VllmDeformDecoderDesc *d, long B, long Lq, long Lt, long S)
{
    const long R = B * Lq, C = d->layers[0].cross_attn.d_model, L = d->layers[0].cross_attn.n_levels;
    DecoderWs w;
    w.layer_bytes = 0;
    for (int l = 0; l < d->n_layers; ++l) {
        const long b = dec_layer_ws_bytes(&d->layers[l], (int)B, (int)Lq, (int)Lt, (int)S);
        if (b > w.layer_bytes) w.layer_bytes = b;
    }
    Carver cv;
    w.layer = cv.take(w.layer_bytes);
    w.hid[0] = cv.take(R * C * 2);
    w.hid[1] = cv.take(R * C * 2);
    w.sine = cv.take(R * 4 * d->n_pos_feats * 2);
    w.t1 = cv.take(R * C * 2);
    w.t2 = cv.take(d->box_heads ? R * C * 2 : 0);
    w.qpos = cv.take(R * C * 2);
    w.rpi = cv.take(R * L * 4 * 4);
    w.total = cv.off;
    return w;
}

int decoder_check_desc(const VllmDeformDecoderDesc *d)
{
    VLLM_REQUIRE(d, "deform_decoder: null descriptor");
    VLLM_REQUIRE(d->n_layers >= 1 && d->n_layers <= 64 && d->layers, "deform_decoder: n_layers=%d (1 .. 64, with their descriptors)", d->n_layers);
    for (int l = 0; l < d->n_layers; ++l) {
        TRY(dec_layer_check_desc(&d->layers[l]));
        const VllmMsdaLayerDesc &at = d->layers[l].cross_attn, &a0 = d->layers[0].cross_attn;
        VLLM_REQUIRE(at.ref_dim == 4, "deform_decoder: layer %d has ref_dim=%d, the decoder takes 4-d reference points", l, at.ref_dim);
        VLLM_REQUIRE(at.d_model == a0.d_model && at.n_levels == a0.n_levels, "deform_decoder: layer %d has d_model=%d n_levels=%d, layer 0 %d and %d",
                     l, at.d_model, at.n_levels, a0.d_model, a0.n_levels);
    }
    VLLM_REQUIRE(d->n_pos_feats > 0 && d->n_pos_feats % 16 == 0, "deform_decoder: n_pos_feats=%d must be a positive multiple of 16", d->n_pos_feats);
    VLLM_REQUIRE(d->layer_norm_eps >= 0.f && d->inverse_sigmoid_eps >= 0.f, "deform_decoder: negative eps");
    VLLM_REQUIRE(d->ref_head_w0 && d->ref_head_b0 && d->ref_head_w1 && d->ref_head_b1 && d->layer_norm_w && d->layer_norm_b && d->dim_t,
                 "deform_decoder: missing weights (reference_points_head / layer_norm / dim_t)");
    if (d->box_heads)
        for (int l = 0; l < d->n_layers; ++l) {
            const VllmBoxHead &bh = d->box_heads[l];
            VLLM_REQUIRE(bh.w0 && bh.b0 && bh.w1 && bh.b1 && bh.w2 && bh.b2, "deform_decoder: missing weights (box head %d)", l);
        }
    return VLLM_OK;
}

int decoder_check_sizes(const VllmDeformDecoderDesc *d, int B, int Lq, int Lt, int S)
{
    for (int l = 0; l < d->n_layers; ++l) TRY(dec_layer_check_sizes(&d->layers[l], B, Lq, Lt, S));
    // (the GEMMs address an operand with 32-bit byte offsets)
    VLLM_REQUIRE((long)B * Lq * 4 * d->n_pos_feats * 2 < (1L << 31), "deform_decoder: B Lq=%ld rows of the sine embedding reach 2^31 bytes", (long)B * Lq);
    return VLLM_OK;
}

long g_calls = 0;

}  // namespace
}  // namespace vllm

using namespace vllm;

extern "C" unsigned long vllm_deform_decoder_desc_sizeof(void) { return sizeof(VllmDeformDecoderDesc); }
extern "C" long vllm_deform_decoder_calls(void) { return g_calls; }

extern "C" long vllm_deform_decoder_workspace_bytes(const VllmDeformDecoderDesc *d, int B, int Lq, int Lt, int S)
{
    if (decoder_check_desc(d) != VLLM_OK || decoder_check_sizes(d, B, Lq, Lt, S) != VLLM_OK) return -1;
    if ((long)B * Lq == 0) return 0;
    return decoder_ws(d, B, Lq, Lt, S).total;
}

extern "C" int vllm_refpoint_embed_bf16(const float *reference_points, const float *valid_ratios, const float *dim_t, int B, int Lq, int L,
                                        int ref_dim, int P, float *reference_points_input, uint16_t *sine, int ld_sine, vllm_stream_t stream)
{
    VLLM_REQUIRE(ref_dim == 4, "refpoint_embed: ref_dim=%d, 4-d reference points only", ref_dim);
    VLLM_REQUIRE(P > 0 && P % 2 == 0 && P % 8 == 0, "refpoint_embed: P=%d must be even and a multiple of 8", P);
    VLLM_REQUIRE(B >= 0 && Lq >= 0 && L >= 1 && (long)B * Lq < (1L << 31), "refpoint_embed: B=%d Lq=%d L=%d", B, Lq, L);
    if ((long)B * Lq == 0) return VLLM_OK;
    VLLM_REQUIRE(reference_points && valid_ratios && dim_t && reference_points_input && sine, "refpoint_embed: null pointer");
    VLLM_REQUIRE(aligned16(reference_points) && aligned8(valid_ratios) && aligned16(dim_t) && aligned16(reference_points_input) && aligned16(sine) &&
                     ld_sine >= 4 * P && ld_sine % 8 == 0,
                 "refpoint_embed: misaligned operand (16 bytes; valid_ratios 8) or ld_sine=%d (a multiple of 8, at least 4 P)", ld_sine);
    return refpoint_embed_launch(reference_points, valid_ratios, dim_t, (long)B * Lq, Lq, L, P, reference_points_input, sine, ld_sine,
                                 (hipStream_t)stream);
}

extern "C" int vllm_box_refine_f32(const uint16_t *h, int ldh, const uint16_t *W, const uint16_t *b, const float *ref, float *new_ref, long R,
                                   int C, float eps, vllm_stream_t stream)
{
    VLLM_REQUIRE(R >= 0 && C >= 64 && C <= 512 && C % 64 == 0, "box_refine: R=%ld C=%d (C a multiple of 64 in 64 .. 512)", R, C);
    if (R == 0) return VLLM_OK;
    VLLM_REQUIRE(h && W && b && ref && new_ref, "box_refine: null pointer");
    VLLM_REQUIRE(aligned16(h) && ldh >= C && ldh % 8 == 0 && aligned16(W) && aligned8(b) && aligned16(ref) && aligned16(new_ref),
                 "box_refine: misaligned operand (16 bytes; b 8) or ldh=%d (a multiple of 8, at least C)", ldh);
    VLLM_REQUIRE(new_ref == ref || !ranges_overlap(new_ref, R * 16, ref, R * 16), "box_refine: new_ref overlaps ref without being ref");
    return box_refine_launch(h, ldh, W, b, ref, new_ref, R, C, eps, (hipStream_t)stream);
}

extern "C" int vllm_deform_decoder_forward(const VllmDeformDecoderDesc *d, const uint16_t *tgt, const float *reference_points,
                                           const float *valid_ratios, const uint8_t *self_attn_mask, const uint16_t *memory_text,
                                           const uint8_t *text_key_padding_mask, const uint16_t *memory, const uint8_t *memory_padding_mask,
                                           const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int Lq, int Lt, int S,
                                           uint16_t *intermediate, float *intermediate_reference_points, void *workspace, long workspace_bytes,
                                           vllm_stream_t stream)
{
    TRY(decoder_check_desc(d));
    TRY(decoder_check_sizes(d, B, Lq, Lt, S));
    if ((long)B * Lq == 0) return VLLM_OK;
    const int NL = d->n_layers, C = d->layers[0].cross_attn.d_model, L = d->layers[0].cross_attn.n_levels, P = d->n_pos_feats;
    const long R = (long)B * Lq;
    VLLM_REQUIRE(tgt && reference_points && valid_ratios && intermediate && intermediate_reference_points,
                 "deform_decoder: null pointer (tgt / reference_points / valid_ratios / intermediate / intermediate_reference_points)");
    VLLM_REQUIRE(aligned16(tgt) && aligned16(reference_points) && aligned8(valid_ratios) && aligned16(intermediate) &&
                     aligned16(intermediate_reference_points) && aligned16(d->dim_t),
                 "deform_decoder: misaligned tgt / reference_points / dim_t / intermediate / intermediate_reference_points (16 bytes) or valid_ratios (8)");
    for (const uint16_t *p : {d->ref_head_w0, d->ref_head_b0, d->ref_head_w1, d->ref_head_b1, d->layer_norm_w, d->layer_norm_b})
        VLLM_REQUIRE(aligned16(p), "deform_decoder: misaligned weight or bias (16 bytes)");
    if (d->box_heads)
        for (int l = 0; l < NL; ++l) {
            const VllmBoxHead &bh = d->box_heads[l];
            VLLM_REQUIRE(aligned16(bh.w0) && aligned16(bh.b0) && aligned16(bh.w1) && aligned16(bh.b1) && aligned16(bh.w2) && aligned8(bh.b2),
                         "deform_decoder: misaligned weight or bias of box head %d (16 bytes; the last bias 8)", l);
        }
    const long ibytes = NL * R * C * 2, rbytes = NL * R * 16;
    const struct { const void *p; long bytes; } inputs[] = {{tgt, R * C * 2}, {reference_points, R * 16}, {valid_ratios, (long)B * L * 8},
                                                            {memory, (long)B * S * C * 2}, {memory_text, (long)B * Lt * C * 2}};
    for (const auto &in : inputs)
        VLLM_REQUIRE(!ranges_overlap(intermediate, ibytes, in.p, in.bytes) && !ranges_overlap(intermediate_reference_points, rbytes, in.p, in.bytes),
                     "deform_decoder: an output overlaps an input (tgt / reference_points / valid_ratios / memory / memory_text)");
    VLLM_REQUIRE(!ranges_overlap(intermediate, ibytes, intermediate_reference_points, rbytes), "deform_decoder: the two outputs overlap");
    const DecoderWs w = decoder_ws(d, B, Lq, Lt, S);
    VLLM_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= w.total,
                 "deform_decoder: workspace too small (%ld < %ld bytes) or misaligned", workspace_bytes, w.total);
    char *ws = (char *)workspace;
    uint16_t *hid[2] = {(uint16_t *)(ws + w.hid[0]), (uint16_t *)(ws + w.hid[1])};
    uint16_t *sine = (uint16_t *)(ws + w.sine), *t1 = (uint16_t *)(ws + w.t1), *t2 = (uint16_t *)(ws + w.t2), *qpos = (uint16_t *)(ws + w.qpos);
    float *rpi = (float *)(ws + w.rpi);
    // every layer's own refusals, on the operands it will get, before anything is enqueued
    for (int l = 0; l < NL; ++l)
        TRY(dec_layer_check_call(&d->layers[l], l == 0 ? tgt : hid[(l - 1) & 1], qpos, rpi, memory_text, memory, spatial_shapes, level_start_index, B,
                                 Lq, Lt, S, hid[l & 1], ws + w.layer, w.layer_bytes));
    ++g_calls;
    hipStream_t st = (hipStream_t)stream;

    const uint16_t *x = tgt;
    const float *ref = reference_points;
    for (int l = 0; l < NL; ++l) {
        uint16_t *y = hid[l & 1];
        // :1865-1874
        TRY(refpoint_embed_launch(ref, valid_ratios, d->dim_t, R, Lq, L, P, rpi, sine, 4 * P, st));
        TRY(gemm(st, EPI_RELU, sine, 4 * P, d->ref_head_w0, 4 * P, d->ref_head_b0, t1, C, (int)R, C, 4 * P));
        TRY(gemm(st, EPI_BIAS, t1, C, d->ref_head_w1, C, d->ref_head_b1, qpos, C, (int)R, C, C));
        // :1907-1921
        TRY(dec_layer_run(&d->layers[l], x, qpos, rpi, self_attn_mask, memory_text, text_key_padding_mask, memory, memory_padding_mask,
                          spatial_shapes, level_start_index, B, Lq, Lt, S, y, ws + w.layer, st));
        // :1939 (no checks of its own: y is a piece of the workspace, layer_norm_w / _b and intermediate are 16-byte aligned by the
        // checks above, a layer's block of intermediate is R C 2 bytes, C a multiple of 64 in 64 .. 512 by dec_layer_check_desc; R > 0)
        TRY(add_layernorm_launch(y, C, nullptr, 0, d->layer_norm_w, d->layer_norm_b, intermediate + (long)l * R * C, C, nullptr, 0, nullptr, 0, R,
                                 C, d->layer_norm_eps, st));
        // :1924-1937, :1940
        float *nref = intermediate_reference_points + (long)l * R * 4;
        if (d->box_heads) {
            const VllmBoxHead &bh = d->box_heads[l];
            TRY(gemm(st, EPI_RELU, y, C, bh.w0, C, bh.b0, t1, C, (int)R, C, C));
            TRY(gemm(st, EPI_RELU, t1, C, bh.w1, C, bh.b1, t2, C, (int)R, C, C));
            TRY(box_refine_launch(t2, C, bh.w2, bh.b2, ref, nref, R, C, d->inverse_sigmoid_eps, st));
            ref = nref;
        } else {
            VLLM_REQUIRE(hipMemcpyAsync(nref, reference_points, (size_t)R * 16, hipMemcpyDeviceToDevice, st) == hipSuccess,
                         "deform_decoder: copy of the reference points failed");
        }
        x = y;
    }
    return VLLM_OK;
}
