/*
 * vllm_hip.h -- C ABI of libvllm_hip.so: the MI355X (gfx950) image->visual-token hot path of VisionLLMv2.
 *
 * Plain pointers and sizes only (no torch / ATen types).  Every pointer marked "device" is a HIP device
 * pointer owned by the caller (PyTorch's caching allocator in practice); the library never allocates or
 * frees device memory and never synchronises: all work is enqueued on `stream` (a hipStream_t passed as
 * void*; NULL = the legacy default stream).  Thread-safety: entry points are re-entrant.  Global state: the per-thread
 * last-error string, and the PROCESS-WIDE tuning knobs of vllm_set_option() (plain ints read at launch time: change them
 * only while no other thread is launching) plus one-time per-process caches (device CU count, kernel attributes).
 *
 * Return value: 0 on success, negative VLLM_E* on error (vllm_last_error() gives the message).  The Python
 * mirror (visionllm_amd/_lib.py) turns non-zero into RuntimeError, as the reference's C++ exceptions do
 * (AT_ASSERTM in visionllmv2/model/unipose/ops/src/cuda/ms_deform_attn_cuda.cu:28-52).
 *
 * Reference paths are relative to /root/reference/VisionLLMv2/.
 *
 * Alignment: any pointer need only be aligned to its element type unless the declaration says more ("Alignment: ..." below);
 * faster kernels behind an entry point are picked by the pointers' alignment and agree with the others to fp32 rounding.  One with a
 * stated requirement returns VLLM_EINVAL (and writes nothing) for a pointer that misses it, and vllm_last_error() names it.
 * Callers passing views at a storage offset (x[1:], a chunk of one flat buffer) copy such an operand into an aligned tensor first,
 * as the Python mirror does.
 */
#ifndef VLLM_HIP_H
#define VLLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct layout or an entry point's meaning changes.  2 (round 4): VllmVitLayer grew by six pointers
 * (an ARRAY of these is passed, so the stride changed) and VllmMsdaLayerDesc got `geometry` / `reserved0` in front of its
 * pointers -- a caller built against version 1 must not run against this library: check vllm_abi_version() == VLLM_ABI_VERSION
 * at load time and the vllm_*_sizeof() of every descriptor it fills. */
#define VLLM_ABI_VERSION 2

#define VLLM_OK 0
#define VLLM_EINVAL (-1)   /* bad argument (shape / alignment / unsupported size) */
#define VLLM_ELAUNCH (-2)  /* hipLaunchKernel / HIP runtime error */
#define VLLM_ENOTIMPL (-3)

typedef void *vllm_stream_t; /* hipStream_t */

int vllm_abi_version(void);
const char *vllm_last_error(void);
/* Fills name[0..cap) with the device's gcnArchName; returns CU count or negative error. */
int vllm_device_info(char *name, int cap);
/* Tuning / test knobs (process-wide).  "msda_tiled": encoder-shaped (Lq == S) MSDA forward kernel, same results to fp32
 * rounding: 0 plain gather kernel; 1 automatic (default): fp32 values on nested level maps generation 9 (msda_tiled9.hip; decided on
 * the device, no host sync, or by the vllm_msda_forward_f32_geo hint), on any other maps generation 4 (msda_tiled4.hip), bf16 values
 * on exact 2x pyramids generation 6 (msda_tiled6.hip); 21 as 1, with generation 9's phase clock (vllm_debug_counters).  Any other
 * value is rejected (VLLM_EINVAL).  "gemm_variant": 0 auto, 1 128x128 kernel, 2 256x256 8-phase
 * kernel, 4 8-phase kernel on the 32x32x16 MFMA.  "gemm_direct_store": the 8-phase kernel's epilogue goes 0 through LDS
 * (row-contiguous 16-byte stores), 1 straight from the accumulator layout, 2 automatic (default; same results either way).
 * "attn_variant": 32 automatic (default) = 2 | 64 with the class-token split.  bit1 deferred rescale, bit4 do not trim padding keys /
 * padding query waves (and no class-token split), bit6 O leaves through LDS as whole rows, bit7 NO class-token split (S = 64 n + 1:
 * token 0 as the initial softmax state of every query, and -- where the n^2 body rows leave a spare wave in their last block -- as
 * that wave's only query row; round 6), bit10 token 0 out of the key tiling only.  Bits 0, 2, 3 selected rounds 2-5 schedules that
 * never became the default (software-pipelined K, s_setprio, hoisted transpose reads); they are ignored since round 6.
 * "dcnv3_tiled": DCNv3 forward for fp32, group channels 16 / 32, <= 9 points: 1 (default) the pipelined LDS-tiled kernel
 * (dcnv3_pipe.hip), 3 the two-blocks-per-CU LDS-tiled kernel (dcnv3_tiled.hip), 0 the gather kernel (same results to fp32
 * rounding); 2 / 4 = 1 / 3 with the phase clock (vllm_debug_counters then reads IT).
 * "msda_layer_fused": 1 (default) vllm_msda_layer_forward runs sampling_offsets + attention_weights as one GEMM whose
 * epilogue does the softmax and the location arithmetic, and takes the operator's result in bf16 straight from the
 * LDS-tiled kernel (needs L * P == 16, P even; other layers compose automatically); 0 the explicit composition (two GEMMs,
 * prep kernel, fp32 operator, conversion pass) -- the A/B reference, same results to fp32 rounding.
 * "gemm_tile_rb" (round 4; VLLM_GEMM_TILE_RB): tile order of the persistent 8-phase GEMM: -1 automatic (default: bands of 4 row
 * panels when the weight has >= 32 column tiles, 8 when >= 8, else the dense order), 0 dense, RB > 0 bands of RB row panels per
 * XCD rectangle; every order gives the same bits.  "gemm_skinny" (round 4; VLLM_GEMM_SKINNY): 1 (default) K = 256, N = 256 / 256 + 128
 * GEMMs with >= 4096 rows (the linears of a d_model = 256 deformable-attention layer) run on the weight-stationary streaming kernel
 * (gemm_skinny.hip); 0 on the 128 x 128 tile kernel -- the same bits either way.
 * "dcnv3_bwd_tiled" (round 4; VLLM_DCNV3_BWD_TILED): 1 (default) vllm_dcnv3_backward_f32 with group channels 32 runs on the windowed
 * kernel (grad_input as S^T x grad_out on the fp32 MFMA: msda_bwd_mfma.hip with the DCN flag), 0 on the gather kernel (global atomics
 * per (point, corner, channel)); the same gradients to fp32 rounding.
 * "gemm_half_tail" (round 4; VLLM_GEMM_HALF_TAIL): 1 (default) the persistent 8-phase GEMM runs the tiles of its last, incomplete round
 * as two half-height tiles each when they then still fit the grid (qkv at 40 ViT-L tiles: 4.27 rounds of work in 5 -> 4 + a half-tile
 * round); 0 whole tiles.  The same bits either way.
 * "gemm_res_ring" (VLLM_GEMM_RES_RING): 1 (default) the persistent 8-phase GEMM with VLLM_EPI_RESIDUAL and no `scale` takes the residual
 * tile through its operand ring and adds it on the matrix pipe (see VLLM_EPI_RESIDUAL below for the contract); 0 the epilogue reads it.
 * The two differ in the fp32 order of the same three terms (bf16 results differ at ties only).
 * "msda_layer_value_bf16" (round 4; VLLM_MSDA_LAYER_VALUE_BF16): 1 (default) vllm_msda_layer_forward stores the projected value in
 * bf16 when the query set is not the value pyramid (decoder cross-attention: the gather kernel reads bf16 natively; the reference's
 * bf16 module rounds the value to bf16 too) and the streaming value GEMM serves the shape; 0 fp32 value everywhere.
 * "deform_enc_ffn_slab_rows" (VLLM_DEFORM_ENC_FFN_SLAB_ROWS): rows of the FFN intermediate [B S, d_ffn] that vllm_deform_enc_layer_forward
 * computes at a time (linear1 + activation, then linear2, slab by slab): 0 (default, the fastest measured) = the whole tensor in one pair
 * of GEMMs; N > 0 = N rows, which shrinks the workspace to one slab of the intermediate at some cost in time; a negative value is rejected.  vllm_deform_enc_layer_workspace_bytes answers for the current value: query the size after setting it.
 * Environment variables VLLM_MSDA_TILED / VLLM_GEMM_VARIANT / VLLM_ATTN_VARIANT give the initial values.  Returns the
 * previous value or VLLM_EINVAL for an unknown name / value.  (Measured-slower experiments -- MSDA generations 3 and 5, the
 * 4-wave GEMM, the two-row-group attention kernel -- live under tools/experiments/ and are not part of the library.) */
int vllm_set_option(const char *name, int value);
/* Diagnostics.  Process-wide and NOT for production use: VLLM_GEMM_PROF=1 reroutes vllm_debug_counters to the GEMM for the
 * whole process; VLLM_GEMM_TRACE (a raw device address the 8-phase GEMM writes per-block timestamps to) exists only in
 * builds with -DVLLM_GEMM_TRACE_ENABLE, where the address is validated as device memory first.
 * (VLLM_GEMM_PROF=1 in the environment: the 8-phase GEMM's prologue / main loop / epilogue ticks + block count;
 * "dcnv3_tiled" = 2 / 4: the DCNv3 kernel's phases; otherwise:) with "msda_tiled" = 21 the MSDA forward's generation 9 adds
 * per-phase shader-clock ticks to 16 device counters; this reads them into out[0..n) and clears them.  Returns the number of
 * counters written. */
int vllm_debug_counters(long *out, int n);
/* In-step kernel timing (measurement; process-wide, off by default).  vllm_prof_enable(1) starts a recording: every
 * operator the library enqueues is preceded by a HIP event on its stream; vllm_prof_read waits for the last one and returns,
 * per tag (vllm_prof_tag_name), the summed time in microseconds from each mark to the next one and the number of marks --
 * a kernel's duration INSIDE the step, queueing and launch gaps included (bench.py's `us_per_launch`).  Both return the
 * number of tags (read: slots needed); vllm_prof_enable(0) stops and discards. */
int vllm_prof_enable(int on);
int vllm_prof_read(double *us_sum, long *count, int n);
const char *vllm_prof_tag_name(int tag);

/* ------------------------------------------------------------------------------------------------
 * B3. Multi-scale deformable attention (MSDA) operator.
 *
 * Replaces:  ms_deform_attn_forward / ms_deform_attn_backward
 *   visionllmv2/model/unipose/ops/src/ms_deform_attn.h:20-61          (pybind module MultiScaleDeformableAttention,
 *   visionllmv2/model/unipose/ops/src/vision.cpp:13-16)
 *   visionllmv2/model/unipose/ops/src/cuda/ms_deform_attn_cuda.cu:20-80, 83-153  (host launchers)
 *   visionllmv2/model/unipose/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-298     (forward kernel)
 *   mmcv/mmcv/ops/csrc/pytorch/ms_deform_attn.cpp:38-60               (mmcv._ext twins)
 *
 * Layouts (all contiguous, as the reference asserts):
 *   value   [B, S, M, D]          S = sum_l H_l*W_l
 *   shapes  [L, 2] int64 (H, W)   DEVICE memory (read by the kernel with scalar loads, like the reference)
 *   lsi     [L]    int64          DEVICE memory, level start index
 *   loc     [B, Lq, M, L, P, 2]   (x, y) in [0,1] (out-of-range allowed -> zero padding)
 *   attw    [B, Lq, M, L, P]
 *   out     [B, Lq, M*D]          fully overwritten (no pre-zeroing needed)
 * `im2col_step` of the reference only chunks the batch over several launches; here it is one launch and the
 * argument does not exist (the Python mirror accepts and checks it: B % min(B, im2col_step) == 0).
 * ------------------------------------------------------------------------------------------------ */
int vllm_msda_forward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                          const float *loc, const float *attw,
                          int B, int S, int M, int D, int L, int Lq, int P,
                          float *out, vllm_stream_t stream);
int vllm_msda_forward_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                          const double *loc, const double *attw,
                          int B, int S, int M, int D, int L, int Lq, int P,
                          double *out, vllm_stream_t stream);
/* vllm_msda_forward_f32 for a caller that knows the level geometry on the HOST.  `shapes` is device memory (as in the
 * reference), so by itself the library cannot know whether the level maps are nested halves whose cells are the Lq
 * queries (the det heads' 168^2 / 84^2 / 42^2 / 21^2 encoder case, or the ceil-divided 100x167 / 50x84 / ... of a detection
 * backbone: served by the pyramid-item kernel) without a host synchronisation: VLLM_GEO_UNKNOWN enqueues the pyramid
 * kernel's two instantiations AND the any-geometry kernel and the device picks (two empty launches).  The reference's modules synchronise once per forward pass anyway (`(H * W).sum() == Len_in`,
 * ms_deform_attn.py:100); the Python mirror learns the geometry in that same read-back and passes it here: exactly one
 * launch.  A PYRAMID / NESTED hint that the device-side test contradicts traps (the hint is never trusted for addressing). */
#define VLLM_GEO_UNKNOWN 0
#define VLLM_GEO_PYRAMID 1
#define VLLM_GEO_GENERAL 2
#define VLLM_GEO_NESTED 3   /* 1-4 levels, each the previous one halved, rounded either way (ceil- / floor-divided maps), not all exact */
int vllm_msda_forward_f32_geo(const float *value, const int64_t *shapes, const int64_t *lsi,
                              const float *loc, const float *attw,
                              int B, int S, int M, int D, int L, int Lq, int P, int geometry,
                              float *out, vllm_stream_t stream);
/* bf16 value/out, fp32 loc/attw, fp32 accumulation (extension: the reference upcasts bf16 to fp32 first,
 * modeling_ov_grounding_dino_mask_dn.py:764-766; this variant halves the gathered bytes). */
/* Alignment: value and out 16 bytes, loc 8 bytes. */
int vllm_msda_forward_bf16(const uint16_t *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *attw,
                           int B, int S, int M, int D, int L, int Lq, int P,
                           uint16_t *out, vllm_stream_t stream);
/* Integer part of the sampling, for index-exact parity tests: per point (b,q,m,l,p)
 * h_low, w_low (int32) and mask (bit0 accepted, bits1..4 corners 1..4 in bounds), computed by the same
 * device function the forward kernels use. */
int vllm_msda_sample_index_f32(const int64_t *shapes, const float *loc,
                               int B, int M, int L, int Lq, int P,
                               int32_t *h_low, int32_t *w_low, uint8_t *mask, vllm_stream_t stream);
/* Backward (B3, row f1 of SURVEY.md section 8).  grad_* must be zero-filled by the caller, exactly as the
 * reference does with at::zeros (ms_deform_attn_cuda.cu:118-120; mmcv multi_scale_deform_attn.py:80-94). */
int vllm_msda_backward_f32(const float *value, const int64_t *shapes, const int64_t *lsi,
                           const float *loc, const float *attw, const float *grad_out,
                           int B, int S, int M, int D, int L, int Lq, int P,
                           float *grad_value, float *grad_loc, float *grad_attw, vllm_stream_t stream);
/* 1 when vllm_msda_backward_f32 with these arguments writes EVERY element of grad_loc and grad_attw itself (the matrix-core kernel of
 * the encoder self-attention shape: the gradients of a rejected point are stored as zeros), so the caller may pass those two
 * uninitialised -- 460 MB of memset less at BASELINE cfg 4, B = 8; grad_value must be zero-filled in every case.  0: zero-fill all three. */
int vllm_msda_backward_f32_writes_point_grads(const float *value, const float *loc, const float *grad_out, const float *grad_value,
                                              const float *grad_loc, int B, int S, int M, int D, int L, int Lq, int P);
int vllm_msda_backward_f64(const double *value, const int64_t *shapes, const int64_t *lsi,
                           const double *loc, const double *attw, const double *grad_out,
                           int B, int S, int M, int D, int L, int Lq, int P,
                           double *grad_value, double *grad_loc, double *grad_attw, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * a13 / f2. The whole deformable-attention LAYER around the operator, for bf16 (inference-dtype) modules.
 *
 * Replaces the bodies of
 *   MSDeformAttn.forward                                   visionllmv2/model/unipose/ops/modules/ms_deform_attn.py:83-145
 *   MultiScaleDeformableAttention.forward (mmcv)           mmcv/ops/multi_scale_deform_attn.py:262-367
 *   GroundingDinoMultiscaleDeformableAttention.forward     visionllmv2/model/grounding_dino/modeling_grounding_dino_mask_dn.py:706-784
 * i.e. value_proj (+ key-padding zero fill), the sampling_offsets / attention_weights linears, softmax over the
 * L*P logits of a head, the location arithmetic (2-d reference points: ref + off / (W_l, H_l); 4-d: ref_xy +
 * off / P * ref_wh * 0.5, or the UniPose "4D normalizer" form off / (W_l, H_l) * ref_wh * 0.5), the operator and
 * output_proj.  Activations and weights are bf16 (nn.Linear layout [out, in]); every INTERNAL tensor (value, offsets,
 * logits, locations, weights, operator output) is kept in fp32, i.e. at or above the precision the reference has
 * when it upcasts around the operator (ms_deform_attn.py:131-139).
 * ------------------------------------------------------------------------------------------------ */
typedef struct VllmMsdaLayerDesc {
    int32_t d_model, n_heads, n_levels, n_points;
    int32_t ref_dim;             /* last dim of reference_points: 2 or 4 */
    int32_t use_4d_normalizer;   /* ref_dim 4 only: UniPose's use_4D_normalizer */
    int32_t geometry;            /* VLLM_GEO_*: what the host knows about spatial_shapes (0 = nothing) */
    int32_t reserved0;           /* 0 */
    const uint16_t *value_proj_w, *value_proj_b;                  /* [C, C], [C]           (device, bf16) */
    const uint16_t *sampling_offsets_w, *sampling_offsets_b;      /* [M*L*P*2, C], [M*L*P*2] */
    const uint16_t *attention_weights_w, *attention_weights_b;    /* [M*L*P, C], [M*L*P] */
    const uint16_t *output_proj_w, *output_proj_b;                /* [C, C], [C] */
} VllmMsdaLayerDesc;
unsigned long vllm_msda_layer_desc_sizeof(void);
/* Bytes of device scratch vllm_msda_layer_forward needs for (B, Lq, S); negative on a bad descriptor. */
long vllm_msda_layer_workspace_bytes(const VllmMsdaLayerDesc *desc, int B, int Lq, int S);
/* query [B, Lq, C] bf16 (position embedding already added by the caller), reference_points [B, Lq, L, ref_dim] fp32,
 * input_flatten [B, S, C] bf16, padding_mask [B, S] uint8 (non-zero = padded) or NULL, spatial_shapes [L, 2] /
 * level_start_index [L] device int64 (H, W), out [B, Lq, C] bf16.  d_model % 64 == 0, d_model / n_heads % 4 == 0. */
/* Alignment: query, input_flatten and every weight / bias of the descriptor 16 bytes (GEMM operands); reference_points 8 bytes (16
 * with ref_dim 4); workspace 16 bytes. */
int vllm_msda_layer_forward(const VllmMsdaLayerDesc *desc, const uint16_t *query, const float *reference_points,
                            const uint16_t *input_flatten, const uint8_t *padding_mask, const int64_t *spatial_shapes,
                            const int64_t *level_start_index, int B, int Lq, int S, uint16_t *out, void *workspace,
                            long workspace_bytes, vllm_stream_t stream);
/* The two elementwise kernels of the layer, exposed for the parity tests:
 * in place, offsets [R, M, L, P, 2] -> sampling locations and logits [R, M, L*P] -> softmax weights (R = B*Lq rows,
 * reference_points [R, L, ref_dim]); and fp32 -> bf16 (round to nearest even) of n elements. */
int vllm_msda_prep_f32(float *offsets_to_locations, float *logits_to_weights, const float *reference_points,
                       const int64_t *spatial_shapes, long R, int M, int L, int P, int ref_dim, int use_4d_normalizer,
                       vllm_stream_t stream);
/* Alignment (vllm_f32_to_bf16): src 16 bytes, dst 8 bytes. */
int vllm_f32_to_bf16(const float *src, uint16_t *dst, long n, vllm_stream_t stream);

/* Training the layer (bf16 modules): the forward pass above with the tensors its backward needs kept in CALLER memory, and the backward
 * from grad_out to grad_query, grad_input_flatten and the gradients of the eight parameters.  Gradients with respect to
 * reference_points are not computed.
 *
 * vllm_msda_layer_forward_train enqueues exactly the launches of vllm_msda_layer_forward for the same arguments (`out` has the same
 * bits).  `saved` (vllm_msda_layer_saved_bytes(desc, B, Lq, S) bytes, < 0 for a refused descriptor) receives, each piece rounded up
 * to 256 bytes: the projected value [B*S, C] (fp32; bf16 in the first half of the same piece on the decoder route, Lq != S), the
 * sampling locations fp32 [B*Lq, M*L*P*2], the softmax weights fp32 [B*Lq, M*L*P], and the bf16 operator output [B*Lq, C].
 * *value_is_bf16 (HOST memory, may be NULL) is set to 1 where the value was stored as bf16, else 0, before the call returns -- no
 * synchronisation; pass it on to the backward.  workspace: vllm_msda_layer_forward_train_workspace_bytes bytes.
 *
 * vllm_msda_layer_backward: grad_out [B*Lq, C] bf16; grad_query [B*Lq, C], grad_input_flatten [B*S, C] and the members of
 * VllmMsdaLayerGrads (shaped like their parameters) are bf16 and may each be NULL (not needed: the product and whatever only it
 * needed is skipped), except that a bias gradient comes out of its weight gradient's launch (pass both).  Every non-NULL gradient
 * is written completely; rows of grad_input_flatten under a padded key are exact zeros.  B * Lq == 0 zero-fills the parameter
 * gradients and grad_input_flatten.  grad_value is accumulated with float atomics, so grad_input_flatten and the value_proj gradients
 * may differ in the last bits between two runs; every other output is deterministic.  workspace:
 * vllm_msda_layer_backward_workspace_bytes bytes (< 0 for a refused descriptor).  The three size queries are host-only.
 * One stream, no allocation, no synchronisation; a refused call (bad descriptor, NULL or misaligned pointer, short or misaligned
 * saved memory or workspace: VLLM_EINVAL) has enqueued nothing. */
typedef struct VllmMsdaLayerGrads {
    uint16_t *value_proj_w, *value_proj_b;
    uint16_t *sampling_offsets_w, *sampling_offsets_b;
    uint16_t *attention_weights_w, *attention_weights_b;
    uint16_t *output_proj_w, *output_proj_b;
} VllmMsdaLayerGrads;
int vllm_msda_layer_grads_sizeof(void);
long vllm_msda_layer_saved_bytes(const VllmMsdaLayerDesc *desc, int B, int Lq, int S);
long vllm_msda_layer_forward_train_workspace_bytes(const VllmMsdaLayerDesc *desc, int B, int Lq, int S);
long vllm_msda_layer_backward_workspace_bytes(const VllmMsdaLayerDesc *desc, int B, int Lq, int S);
/* Alignment: query, input_flatten, out, every weight / bias of the descriptor, saved and workspace 16 bytes; reference_points 8 bytes
 * (16 with ref_dim 4). */
int vllm_msda_layer_forward_train(const VllmMsdaLayerDesc *desc, const uint16_t *query, const float *reference_points,
                                  const uint16_t *input_flatten, const uint8_t *padding_mask, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, int B, int Lq, int S, uint16_t *out, void *saved,
                                  long saved_bytes, int *value_is_bf16, void *workspace, long workspace_bytes,
                                  vllm_stream_t stream);
/* Alignment: as vllm_msda_layer_forward_train; grad_out and every gradient 16 bytes. */
int vllm_msda_layer_backward(const VllmMsdaLayerDesc *desc, const uint16_t *query, const float *reference_points,
                             const uint16_t *input_flatten, const uint8_t *padding_mask, const int64_t *spatial_shapes,
                             const int64_t *level_start_index, int B, int Lq, int S, const void *saved, long saved_bytes,
                             int value_is_bf16, const uint16_t *grad_out, uint16_t *grad_query, uint16_t *grad_input_flatten,
                             const VllmMsdaLayerGrads *grads, void *workspace, long workspace_bytes, vllm_stream_t stream);
/* The three elementwise kernels of the backward, exposed for the parity tests.
 * vllm_msda_prep_backward_f32: the backward of vllm_msda_prep_f32 -- dq [R, npad] bf16, columns [0, 2 M L P) = grad_loc * (sx, sy)
 * (the location arithmetic's scale), [2 M L P, 3 M L P) = w * (grad_attw - sum_{L*P} grad_attw w) per head (w the softmax weights),
 * [3 M L P, npad) zeros; npad >= 3 M L P.  16-byte aligned operands and npad % 8 == 0 select the vector kernels (same results).
 * vllm_f32_to_bf16_masked: dst [rows, cols] bf16 = src, round to nearest even, rows with a non-zero row_mask byte (row_mask may be
 * NULL) written as zeros whatever src holds there.  vllm_bf16_to_f32: n elements widened. */
/* Alignment: element alignment only (16 bytes for the vector kernels). */
int vllm_msda_prep_backward_f32(const float *grad_loc, const float *grad_attw, const float *attw, const float *reference_points,
                                const int64_t *spatial_shapes, long R, int M, int L, int P, int ref_dim, int use_4d_normalizer,
                                uint16_t *dq, int npad, vllm_stream_t stream);
int vllm_f32_to_bf16_masked(const float *src, uint16_t *dst, long rows, int cols, const uint8_t *row_mask, vllm_stream_t stream);
/* Alignment: src and dst 16 bytes. */
int vllm_bf16_to_f32(const uint16_t *src, float *dst, long n, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f3. DCNv3 forward (InternImage det backbone).
 *
 * Replaces:  dcnv3_forward   visionllmv2/model/ops_dcnv3/src/dcnv3.h:20-39, src/cuda/dcnv3_cuda.cu:20-80
 *            (kernel src/cuda/dcnv3_im2col_cuda.cuh:217-278; Python caller functions/dcnv3_func.py:39-43).
 * input [N, H, W, G*C], offset [N, Ho, Wo, G*kh*kw*2] (x, y pairs, kernel_w-outer / kernel_h-inner point order),
 * mask [N, Ho, Wo, G*kh*kw], out [N, Ho, Wo, G*C]; Ho = (H + 2*ph - (dh*(kh-1)+1)) / sh + 1 (likewise Wo).  All device,
 * contiguous.  im2col_step of the reference is a batching detail of its launch loop and has no counterpart (one launch).
 * ------------------------------------------------------------------------------------------------ */
int vllm_dcnv3_forward_f32(const float *input, const float *offset, const float *mask, int N, int H, int W, int G, int C,
                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale, float *out,
                           vllm_stream_t stream);
int vllm_dcnv3_forward_f64(const double *input, const double *offset, const double *mask, int N, int H, int W, int G, int C,
                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, double offset_scale, double *out,
                           vllm_stream_t stream);
/* Half precision (round 5): the reference dispatches AT_DISPATCH_FLOATING_TYPES_AND_HALF (dcnv3_cuda.cu:69) with opmath_t = float.
 * IEEE binary16 tensors as uint16_t bit patterns; fp32 arithmetic, the output rounded to nearest even once. */
int vllm_dcnv3_forward_f16(const uint16_t *input, const uint16_t *offset, const uint16_t *mask, int N, int H, int W, int G, int C,
                           int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale, uint16_t *out,
                           vllm_stream_t stream);
/* Backward (round 4).  Replaces DCNv3.dcnv3_backward (ops_dcnv3/src/dcnv3.h:41-64, cuda/dcnv3_cuda.cu:92-174; kernels
 * dcnv3_im2col_cuda.cuh:86-146, 279-857), called by DCNv3Function.backward (functions/dcnv3_func.py:51-59).
 * grad_output [N, Ho, Wo, G*C]; grad_input [N, H, W, G*C] MUST BE ZERO-FILLED by the caller (the reference's host code allocates it
 * with at::zeros_like; the sums arrive by floating-point atomics); grad_offset [N, Ho, Wo, G*kh*kw*2] and grad_mask
 * [N, Ho, Wo, G*kh*kw] are written completely.  Any channel count (group channels 4 / 8 / 16 / 32 / 64: the vectorised kernel). */
int vllm_dcnv3_backward_f32(const float *input, const float *offset, const float *mask, const float *grad_output, int N, int H, int W,
                            int G, int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale,
                            float *grad_input, float *grad_offset, float *grad_mask, vllm_stream_t stream);
int vllm_dcnv3_backward_f64(const double *input, const double *offset, const double *mask, const double *grad_output, int N, int H, int W,
                            int G, int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, double offset_scale,
                            double *grad_input, double *grad_offset, double *grad_mask, vllm_stream_t stream);

/* Half-precision backward (round 5; dcnv3_cuda.cu:147 dispatches AND_HALF too): operands and gradients are binary16, the arithmetic
 * is the fp32 backward on widened copies in the CALLER's workspace (vllm_dcnv3_backward_f16_workspace bytes, 16-byte aligned; -1 for
 * an invalid geometry), every gradient rounded once.  grad_input need not be zero-filled here (the fp32 accumulator is). */
/* Alignment (vllm_dcnv3_backward_f16): all seven tensors and the workspace 16 bytes. */
long vllm_dcnv3_backward_f16_workspace(int N, int H, int W, int G, int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw);
int vllm_dcnv3_backward_f16(const uint16_t *input, const uint16_t *offset, const uint16_t *mask, const uint16_t *grad_output, int N, int H,
                            int W, int G, int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, float offset_scale,
                            uint16_t *grad_input, uint16_t *grad_offset, uint16_t *grad_mask, void *workspace, long workspace_bytes,
                            vllm_stream_t stream);
/* Kernel launches of this process per DCNv3 route (tests / tuning), counted on the host where the launch is made: 0 gather forward
 * (every dtype), 1 pipelined forward (dcnv3_tiled 1 / 2), 2 two-blocks-per-CU forward (3 / 4), 3 vectorised backward (4 / 8 / 16 / 32 /
 * 64 group channels), 4 generic backward, 5 windowed matrix-core backward (dcnv3_bwd_tiled 1, group channels 32; the half-precision
 * backward runs the fp32 routes and counts there).  -1 for any other route. */
long vllm_dcnv3_route_launches(int route);

/* ------------------------------------------------------------------------------------------------
 * f2b. The whole deformable ENCODER layer around the attention layer above, bf16 modules (inference).
 *
 * Replaces the bodies of
 *   DeformableTransformerEncoderLayer.forward   visionllmv2/model/unipose/modeling_unipose.py:3132-3186 (without channel attention)
 *   GroundingDinoDeformableLayer.forward        visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1105-1180
 * i.e.  q = src + pos;  x = norm1(src + self_attn(q, reference_points, src));  out = norm2(x + linear2(act(linear1(x))))
 * (dropout is the identity at inference).  The launches: [q = src + pos,] the launches of vllm_msda_layer_forward with `src` added in
 * output_proj's epilogue, LayerNorm, per slab of rows linear1 + activation and linear2 + residual, LayerNorm [+ pos].  Every tensor
 * between two launches is bf16, as in the bf16 module; sums, statistics and activations are fp32 with one rounding per stored tensor.
 * `attn.ref_dim` must be 2 (the encoder's reference points), d_model a multiple of 64 up to 512, d_ffn a multiple of 64.
 * ------------------------------------------------------------------------------------------------ */
typedef struct VllmDeformEncLayerDesc {
    VllmMsdaLayerDesc attn;            /* ref_dim 2 */
    int32_t d_ffn, act;                /* act: 0 = ReLU, VLLM_EPI_GELU = erf GELU */
    float norm1_eps, norm2_eps;
    const uint16_t *norm1_w, *norm1_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *norm2_w, *norm2_b;   /* [C] [C] [d_ffn, C] [d_ffn] [C, d_ffn] [C] [C] [C] */
} VllmDeformEncLayerDesc;
unsigned long vllm_deform_enc_layer_desc_sizeof(void);
/* Bytes of device scratch vllm_deform_enc_layer_forward needs for B images of S tokens under the CURRENT value of the option
 * "deform_enc_ffn_slab_rows"; host-only; 0 for B S == 0, negative for a refused descriptor or sizes. */
long vllm_deform_enc_layer_workspace_bytes(const VllmDeformEncLayerDesc *desc, int B, int S);
long vllm_deform_enc_layer_calls(void);   /* calls of vllm_deform_enc_layer_forward in this process that reached their launches (tests) */
/* src, out [B, S, C] bf16; pos [B, S, C] bf16 or NULL (no position embedding); reference_points [B, S, L, 2] fp32; padding_mask [B, S]
 * uint8 (non-zero = padded) or NULL; spatial_shapes [L, 2] / level_start_index [L] device int64.
 * query_in [B, S, C] or NULL: the attention's query where the caller has it already (the `query_out` of the layer in front) -- else
 *   the call computes src + pos itself (or uses src, without pos).
 * query_out [B, S, C] or NULL: receives bf16(out + pos), the next layer's query, bit-identical to adding pos to `out` (needs pos).
 * `out` may not overlap `src` or `pos`.  One stream, no allocation, no synchronisation.  A refused call (descriptor; NULL or misaligned
 * operand; short or misaligned workspace: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing; B S == 0 returns VLLM_OK. */
/* Alignment: src, pos, query_in, out, query_out, every weight / bias of the descriptor and workspace 16 bytes; reference_points 8 bytes. */
int vllm_deform_enc_layer_forward(const VllmDeformEncLayerDesc *desc, const uint16_t *src, const uint16_t *pos, const uint16_t *query_in,
                                  const float *reference_points, const uint8_t *padding_mask, const int64_t *spatial_shapes,
                                  const int64_t *level_start_index, int B, int S, uint16_t *out, uint16_t *query_out, void *workspace,
                                  long workspace_bytes, vllm_stream_t stream);
/* The kernels of the layer, exposed for the parity tests.
 * vllm_add_layernorm_bf16: y [rows, C] = LayerNorm_C(x + res) * weight + bias; x, res bf16, the sum and the statistics fp32 (second moment
 *   about the mean), one rounding.  res NULL: a plain LayerNorm.  y_pos non-NULL (then pos too): y_pos = bf16(bf16(y) + pos), the bits of
 *   vllm_add_bf16 on the stored y.  Each of x, res, y, pos, y_pos has its own row stride (elements, a multiple of 8, at least C); y may be
 *   x.  C a multiple of 64 in 64 .. 512.  Nothing is written outside the C columns of a row.
 * vllm_add_bf16: out[i] = bf16(a[i] + b[i]), i < n (fp32 sum, round to nearest even); any alignment, 16-byte vectors where all three
 *   pointers are 16-byte aligned.
 * vllm_gemm_bf16_relu: vllm_gemm_bf16 (layouts, alignment) with the layer's ReLU epilogue y = v < 0 ? 0 : v, v = x W^T + bias (a NaN stays
 *   a NaN); force_bits carries VLLM_GEMM_FORCE_128 / _256 / _192 / _MF32 only.  Always one workgroup per tile. */
/* Alignment (vllm_add_layernorm_bf16): every pointer 16 bytes. */
int vllm_add_layernorm_bf16(const uint16_t *x, int ldx, const uint16_t *res, int ldr, const uint16_t *weight, const uint16_t *bias,
                            uint16_t *y, int ldy, const uint16_t *pos, int ldp, uint16_t *y_pos, int ldq, long rows, int C, float eps,
                            vllm_stream_t stream);
int vllm_add_bf16(const uint16_t *a, const uint16_t *b, uint16_t *out, long n, vllm_stream_t stream);
int vllm_gemm_bf16_relu(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y, int M, int N, int K, int ldx, int ldw,
                        int ldy, int force_bits, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f2c. The whole deformable DECODER layer, bf16 modules (inference).
 *
 * Replaces the bodies of
 *   DeformableTransformerDecoderLayer.forward   visionllmv2/model/unipose/modeling_unipose.py:3250-3323
 *   GroundingDinoDecoderLayer.forward           visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1332-1407
 * i.e., batch-first and with dropout the identity,
 *   1. q = tgt + pos;  x = LN_sa(tgt + out_proj(MHA(q Wq, q Wk, tgt Wv, self_attn_mask)))                       (has_self_attn)
 *   2. x = LN_text(x + out_proj_t(MHA((x + pos) Wq, text Wk, text Wv, text_key_padding_mask)))                  (has_text_attn)
 *   3. x = LN_ca(x + cross_attn(x + pos, reference_points, memory, ...))          (the attention layer of section f2, ref_dim 2 or 4)
 *   4. out = LN_ffn(x + fc2(act(fc1(x))))
 * The launches: vllm_add_bf16 forms tgt + pos once, every later x + pos is the y_pos output of the vllm_add_layernorm_bf16 in front of its
 * reader; per attention block two projection GEMMs on pointer-offset slices of the module's own in_proj parameter (self: N = 2C on q
 * and N = C on tgt; text: N = C on x + pos and N = 2C on memory_text), vllm_mha_fwd_bf16 on column slices of their outputs, out_proj with
 * the residual in its epilogue, LayerNorm; the launches of vllm_msda_layer_forward with the residual in output_proj's epilogue,
 * LayerNorm; fc1 + ReLU / GELU, fc2 + residual, LayerNorm.  No weight is copied or repacked.  Every tensor between two launches is
 * bf16, as in the bf16 module; sums, scores, statistics and activations are fp32 with one rounding per stored tensor.
 * d_model a multiple of 64 up to 512, d_ffn a multiple of 64, d_model / n_heads_sa 32 or 64.  No runtime option.
 * ------------------------------------------------------------------------------------------------ */
typedef struct VllmDeformDecLayerDesc {
    VllmMsdaLayerDesc cross_attn;          /* ref_dim 2 or 4, use_4d_normalizer as given */
    int32_t d_ffn, act;                    /* act: 0 = ReLU, VLLM_EPI_GELU = erf GELU */
    int32_t n_heads_sa;                    /* heads of self_attn and of the text attention */
    int32_t has_self_attn, has_text_attn;  /* UniPose: 0 after rm_self_attn_modules() / without use_text_cross_attention */
    float   sa_norm_eps, text_norm_eps, ca_norm_eps, ffn_norm_eps;
    const uint16_t *sa_in_proj_w, *sa_in_proj_b, *sa_out_proj_w, *sa_out_proj_b, *sa_norm_w, *sa_norm_b;         /* [3C, C] [3C] [C, C] [C] [C] [C] */
    const uint16_t *text_in_proj_w, *text_in_proj_b, *text_out_proj_w, *text_out_proj_b, *text_norm_w, *text_norm_b;
    const uint16_t *ca_norm_w, *ca_norm_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ffn_norm_w, *ffn_norm_b;   /* [C] [C] [d_ffn, C] [d_ffn] [C, d_ffn] [C] [C] [C] */
} VllmDeformDecLayerDesc;
unsigned long vllm_deform_dec_layer_desc_sizeof(void);
/* Bytes of device scratch vllm_deform_dec_layer_forward needs for B images of Lq queries, Lt text tokens and S memory tokens; host-only;
 * 0 for B Lq == 0, negative for a refused descriptor or sizes. */
long vllm_deform_dec_layer_workspace_bytes(const VllmDeformDecLayerDesc *desc, int B, int Lq, int Lt, int S);
long vllm_deform_dec_layer_calls(void);   /* calls of vllm_deform_dec_layer_forward in this process that reached their launches (tests) */
/* tgt, out [B, Lq, C] bf16; query_pos [B, Lq, C] bf16 or NULL; reference_points [B, Lq, L, ref_dim] fp32; self_attn_mask [Lq, Lq] uint8
 * (non-zero = may NOT attend) or NULL; memory_text [B, Lt, C] bf16 (read with has_text_attn only); text_key_padding_mask [B, Lt] uint8
 * (non-zero = ignore this token) or NULL; memory [B, S, C] bf16; memory_padding_mask [B, S] uint8 (non-zero = padded) or NULL;
 * spatial_shapes [L, 2] / level_start_index [L] device int64.  A query row whose keys are all masked is NaN, as in the modules.
 * One stream, no allocation, no synchronisation.  A refused call (descriptor; d_model not a multiple of 64 in 64 .. 512; d_ffn not a
 * multiple of 64; head dim not 32 / 64; NULL or misaligned operand; `out` overlapping tgt / query_pos / memory_text / memory; short or
 * misaligned workspace: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing; B Lq == 0 returns VLLM_OK. */
/* Alignment: tgt, query_pos, memory_text, memory, out, every weight / bias of the descriptor and workspace 16 bytes; reference_points
 * 8 bytes, 16 with ref_dim 4; the masks: element alignment. */
int vllm_deform_dec_layer_forward(const VllmDeformDecLayerDesc *desc, const uint16_t *tgt, const uint16_t *query_pos,
                                  const float *reference_points, const uint8_t *self_attn_mask, const uint16_t *memory_text,
                                  const uint8_t *text_key_padding_mask, const uint16_t *memory, const uint8_t *memory_padding_mask,
                                  const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int Lq, int Lt, int S,
                                  uint16_t *out, void *workspace, long workspace_bytes, vllm_stream_t stream);
/* The attention kernel of blocks 1 and 2, exposed for the parity tests: masked multi-head attention for short sequences.
 * Head h of token (b, i) of an operand is D contiguous bf16 at ptr + b * batch_stride + i * ld + h * D (strides in elements), so q, k
 * and v are read in place from column slices of packed projection outputs.  D 32 or 64; Lq, Lk >= 1, neither bounded by a tile; H >= 1.
 *   out[b, i, h, :] = softmax_j(softmax_scale * q . k_j, masked keys at -inf) V
 * attn_mask [Lq, Lk] (non-zero = may NOT attend) or NULL; key_padding_mask [B, Lk] (non-zero = ignore this key) or NULL.  Scores,
 * softmax and accumulation fp32, P rounded to bf16 before P V, one rounding of the result.  A row with EVERY key masked is NaN in all D
 * outputs of that head (softmax of an all -inf row, as in nn.MultiheadAttention).  Nothing is written outside the H D columns of an
 * output row.  No atomics: the same bits on every run.  A refused call (D; a NULL operand; a misaligned pointer or stride; a row stride
 * below H D: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing; B Lq == 0 returns VLLM_OK. */
/* Alignment: q, k, v, out 16 bytes, their row and batch strides multiples of 8 elements; the masks: element alignment. */
int vllm_mha_fwd_bf16(const uint16_t *q, long q_batch_stride, int ldq, const uint16_t *k, long k_batch_stride, int ldk,
                      const uint16_t *v, long v_batch_stride, int ldv, uint16_t *out, long o_batch_stride, int ldo,
                      const uint8_t *attn_mask, const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D,
                      float softmax_scale, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f2d. The whole Grounding-DINO DECODER around the layer above, bf16 modules (inference), 4-d reference points.
 *
 * Replaces the body of
 *   GroundingDinoDecoder.forward   visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:1792-1981
 * without output_attentions / output_hidden_states.  Per layer l, in this order:
 *   1. vllm_refpoint_embed_bf16: reference_points_input = ref * valid_ratios (fp32) and the sine embedding of its level 0 (bf16)
 *   2. reference_points_head: two GEMMs (ReLU, bias) -> query_pos, bf16
 *   3. the launches of vllm_deform_dec_layer_forward for layers[l] on the running hidden state (the un-normed output of layer l - 1)
 *   4. vllm_add_layernorm_bf16 (no residual) -> intermediate[l]
 *   5. with a box head: two ReLU GEMMs and vllm_box_refine_f32 -> intermediate_reference_points[l], the next layer's `ref`;
 *      without one (box_heads NULL) the reference points never change and intermediate_reference_points[l] is a copy of the input.
 * Both outputs are LAYER-MAJOR ([n_layers, B, Lq, .]; the module stacks along dim 1): every launch writes one dense block, nothing is
 * stacked or copied afterwards.  Reference points are fp32 from entry to exit; the box delta is never rounded to bf16.
 * ------------------------------------------------------------------------------------------------ */
typedef struct VllmBoxHead {
    const uint16_t *w0, *b0, *w1, *b1, *w2, *b2;   /* [C, C] [C] [C, C] [C] [4, C] [4]  (device, bf16) */
} VllmBoxHead;
typedef struct VllmDeformDecoderDesc {
    int32_t n_layers;                        /* 1 .. 64 */
    int32_t n_pos_feats;                     /* P: sine features per coordinate; a multiple of 16 (4 P is a GEMM's K) */
    float   layer_norm_eps;
    float   inverse_sigmoid_eps;             /* 1e-5 in the reference (:401) */
    const VllmDeformDecLayerDesc *layers;    /* HOST array [n_layers]; one d_model, n_levels; cross_attn.ref_dim 4 */
    const uint16_t *ref_head_w0, *ref_head_b0, *ref_head_w1, *ref_head_b1;   /* reference_points_head: [C, 4P] [C] [C, C] [C] */
    const uint16_t *layer_norm_w, *layer_norm_b;                             /* [C] [C] */
    const float    *dim_t;                   /* [P] fp32, device: the module's own temperature table (:1761-1762) */
    const VllmBoxHead *box_heads;            /* HOST array [n_layers] (entries may repeat: a shared head) or NULL: no refinement */
} VllmDeformDecoderDesc;
unsigned long vllm_deform_decoder_desc_sizeof(void);
/* Bytes of device scratch vllm_deform_decoder_forward needs; host-only; 0 for B Lq == 0, negative for a refused descriptor or sizes. */
long vllm_deform_decoder_workspace_bytes(const VllmDeformDecoderDesc *desc, int B, int Lq, int Lt, int S);
long vllm_deform_decoder_calls(void);   /* calls of vllm_deform_decoder_forward in this process that reached their launches (tests) */
/* tgt [B, Lq, C] bf16; reference_points [B, Lq, 4] fp32; valid_ratios [B, L, 2] fp32; the masks, memory_text, memory, spatial_shapes and
 * level_start_index as vllm_deform_dec_layer_forward takes them; intermediate [n_layers, B, Lq, C] bf16;
 * intermediate_reference_points [n_layers, B, Lq, 4] fp32.  One stream, no allocation, no synchronisation.  A refused call (NULL or
 * misaligned operand; ref_dim != 4; a layer descriptor its own entry refuses; layers of differing d_model / n_levels; n_pos_feats;
 * an output overlapping an input or the other output; short or misaligned workspace: VLLM_EINVAL, reason in vllm_last_error()) has
 * enqueued nothing; B Lq == 0 returns VLLM_OK.  vllm_deform_dec_layer_calls() is not touched. */
/* Alignment: tgt, memory_text, memory, reference_points, dim_t, both outputs, every weight / bias and workspace 16 bytes; valid_ratios
 * 8 bytes; the masks: element alignment. */
int vllm_deform_decoder_forward(const VllmDeformDecoderDesc *desc, const uint16_t *tgt, const float *reference_points,
                                const float *valid_ratios, const uint8_t *self_attn_mask, const uint16_t *memory_text,
                                const uint8_t *text_key_padding_mask, const uint16_t *memory, const uint8_t *memory_padding_mask,
                                const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int Lq, int Lt, int S,
                                uint16_t *intermediate, float *intermediate_reference_points, void *workspace, long workspace_bytes,
                                vllm_stream_t stream);
/* The two row kernels of the loop, exposed for the parity tests (and for other decoder flavours: the sine formula is DINO's, eps a
 * parameter).  No atomics: the same bits on every run.
 * vllm_refpoint_embed_bf16: rows = B Lq.  reference_points_input [B, Lq, L, 4] fp32 = ref[b, q, k] * valid_ratios[b, l, k & 1], one fp32
 *   product.  sine [B Lq, 4 P] bf16 with row stride ld_sine (elements, a multiple of 8, at least 4 P), from level 0 of that product in
 *   the order (y, x, w, h): element i of a group is sin (i even) or cos (i odd) of (v * 2 pi) / dim_t[i] -- fp32, a true division, the
 *   accurate sinf / cosf, one rounding.  Nothing is written outside the 4 P columns of a row.  ref_dim must be 4, P a multiple of 8.
 * vllm_box_refine_f32: new_ref[r, k] = sigmoid(sum_c h[r, c] W[k, c] + b[k] + log(max(x, eps) / max(1 - x, eps))), x = ref[r, k]
 *   clamped to [0, 1]; h [R, C] bf16 with row stride ldh (a multiple of 8, at least C), W [4, C], b [4] bf16; everything fp32 in a fixed
 *   order, new_ref [R, 4] fp32, which may be `ref` itself.  C a multiple of 64 in 64 .. 512.
 * A refused call (VLLM_EINVAL) has enqueued nothing; no rows returns VLLM_OK. */
/* Alignment: reference_points, dim_t, reference_points_input, sine, h, W, ref, new_ref 16 bytes; valid_ratios, b 8 bytes. */
int vllm_refpoint_embed_bf16(const float *reference_points, const float *valid_ratios, const float *dim_t, int B, int Lq, int L, int ref_dim,
                             int P, float *reference_points_input, uint16_t *sine, int ld_sine, vllm_stream_t stream);
int vllm_box_refine_f32(const uint16_t *h, int ldh, const uint16_t *W, const uint16_t *b, const float *ref, float *new_ref, long R, int C,
                        float eps, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f2e. The two-stage QUERY SELECTION of Grounding-DINO between the encoder and the decoder above, bf16 modules (inference).
 *
 * Replaces gen_encoder_output_proposals and the `two_stage` statements of
 *   OVGroundingDinoModel.forward   visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:2228-2276, :2503-2543
 * with GroundingDinoContrastiveEmbedding (:1410-1428), without the mask heads.  The selection depends only on the row maximum of the class
 * logits; the box head, the logit rows and the proposal logits are formed for the k selected rows only.  In this order:
 *   1. extents: per image and level, valid_height = the unpadded cells of column 0, valid_width = those of row 0 (a fixed-order count)
 *   2. enc_output (GEMM + bias) on the raw memory rows, read in place, then enc_output_norm.  A row the reference zero-fills (padded, or
 *      an invalid proposal) is normalised from the bias itself: it comes out exactly as LayerNorm(bias).  A proposal is
 *      ((x + 0.5) / valid_width, (y + 0.5) / valid_height, 0.05 * 2^level twice) in fp32 with a true division, and valid when all four
 *      values lie strictly inside (0.01, 0.99).
 *   3. vllm_rowmax_dot_bf16: score[b, s] = bf16(max over unmasked text tokens of q[b, s] . text[b, t]) as fp32; no [B, S, Lt] tensor
 *   4. vllm_topk_rows_f32: the k largest per image -- value descending, ties by ascending index, NaN greatest
 *   5. on the B k selected rows: a gather -> target; the box head (two ReLU GEMMs, the last linear in fp32, never rounded) plus the row's
 *      proposal logit log(p / (1 - p)) (+inf for a padded row or an invalid proposal) -> coords_logits; reference_points = its sigmoid
 *      (+inf gives 1.0); class_logits = bf16(target . text^T) widened to fp32, -inf at masked tokens and from Lt up to max_text_len.
 * No atomics on any output: the same bits on every run.
 * ------------------------------------------------------------------------------------------------ */
typedef struct VllmQuerySelectDesc {
    int32_t d_model;                         /* C: a multiple of 64 in 64 .. 512 */
    int32_t max_text_len;                    /* columns of class_logits, 1 .. 256 */
    int32_t n_levels;                        /* rows of spatial_shapes, 1 .. 16 */
    float   layer_norm_eps;
    const uint16_t *enc_output_w, *enc_output_b;             /* [C, C] [C]  (device, bf16) */
    const uint16_t *enc_output_norm_w, *enc_output_norm_b;   /* [C] [C] */
    VllmBoxHead box_head;                    /* encoder_output_bbox_embed */
} VllmQuerySelectDesc;
unsigned long vllm_query_select_desc_sizeof(void);
/* Bytes of device scratch vllm_query_select_forward needs; host-only; 0 for B k == 0, negative for a refused descriptor or sizes. */
long vllm_query_select_workspace_bytes(const VllmQuerySelectDesc *desc, int B, int S, int Lt, int k);
long vllm_query_select_calls(void);   /* calls of vllm_query_select_forward in this process that reached their launches (tests) */
/* memory [B, S, C] bf16; padding_mask [B, S] uint8, 1 = padded; text [B, Lt, C] bf16; text_token_mask [B, Lt] uint8, 1 = a real token;
 * spatial_shapes [n_levels, 2] and level_start_index [n_levels] int64 on the device, describing S rows.  Outputs: topk_index [B, k] int64;
 * target [B, k, C] bf16; coords_logits and reference_points [B, k, 4] fp32; class_logits [B, k, max_text_len] fp32; scores [B, S] fp32,
 * optional (NULL keeps them in the workspace).  Sizes: 1 <= Lt <= max_text_len, 1 <= k <= min(S, 2048), B S C 2 < 2^31.  One stream, no
 * allocation, no synchronisation.  A refused call (NULL or misaligned operand; an output overlapping an input, another output or the
 * workspace; sizes outside the contract; short or misaligned workspace: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing;
 * B k == 0 returns VLLM_OK. */
/* Alignment: memory, text, target, coords_logits, reference_points, every weight / bias and workspace 16 bytes; spatial_shapes,
 * level_start_index, topk_index and the box head's last bias 8 bytes; class_logits, scores 4 bytes; the masks: element alignment. */
int vllm_query_select_forward(const VllmQuerySelectDesc *desc, const uint16_t *memory, const uint8_t *padding_mask, const uint16_t *text,
                              const uint8_t *text_token_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int S,
                              int Lt, int k, int64_t *topk_index, uint16_t *target, float *coords_logits, float *reference_points,
                              float *class_logits, float *scores, void *workspace, long workspace_bytes, vllm_stream_t stream);
/* The three new kernels of the call, exposed for the parity tests and for other selection flavours.  No atomics on an output.
 * vllm_rowmax_dot_bf16: scores [B, S] fp32 = bf16(max over tokens t with text_token_mask[b, t] != 0 of sum_c q[b, s, c] text[b, t, c]),
 *   fp32 accumulation; q [B, S, C], text [B, Lt, C] bf16, dense.  Every token masked: -inf; a NaN logit: NaN.  C a multiple of 64 in
 *   64 .. 512, 1 <= Lt <= 256, any S.
 * vllm_topk_rows_f32: index [B, k] int64 = per row of scores [B, S] the indices of its k largest, value descending, ties by ascending
 *   index, NaN greatest, -0 == +0: torch.sort(scores, descending=True, stable=True).indices[:, :k].  1 <= k <= min(S, 2048), S < 2^31.
 * vllm_query_select_tail_f32: step 1 and the fp32 part of step 5 for rows given by topk_index [B, k]: extents [B, L, 2] int32 (written),
 *   coords_logits[r] = h[r] . W^T + b + proposal logit, reference_points = sigmoid; h [B k, C] bf16 with row stride ldh (a multiple of 8,
 *   at least C), W [4, C], b [4] bf16; valid [B k] uint8 (optional): the proposals' validity flags.
 * A refused call (VLLM_EINVAL) has enqueued nothing; no rows returns VLLM_OK. */
/* Alignment: q, text, h, W, coords_logits, reference_points 16 bytes; b, index, topk_index and the level tensors 8 bytes; scores,
 * extents 4 bytes. */
int vllm_rowmax_dot_bf16(const uint16_t *q, const uint16_t *text, const uint8_t *text_token_mask, int B, int S, int Lt, int C, float *scores,
                         vllm_stream_t stream);
int vllm_topk_rows_f32(const float *scores, int B, int S, int k, int64_t *index, vllm_stream_t stream);
int vllm_query_select_tail_f32(const uint16_t *h, int ldh, const uint16_t *W, const uint16_t *b, const int64_t *topk_index,
                               const uint8_t *padding_mask, const int64_t *spatial_shapes, const int64_t *level_start_index, int B, int S,
                               int L, int k, int C, int32_t *extents, float *coords_logits, float *reference_points, uint8_t *valid,
                               vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f2f. The FUSION LAYER of Grounding-DINO (bi-directional image <-> text attention) in front of every deformable encoder layer, bf16
 * modules (inference).
 *
 * Replaces the bodies of
 *   GroundingDinoBiMultiHeadAttention.forward, GroundingDinoFusionLayer.forward
 *       visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:860-1101
 * with dropout and drop-path the identity and without the two [B, H, ., .] attention-weight tensors, which are never built.  The launches:
 *   1. v = LN_vision(vision), t = LN_text(text)                                                              (vllm_layernorm_bf16)
 *   2. vision_proj(v), values_vision_proj(v), text_proj(t), values_text_proj(t)                   (vllm_gemm_bf16, VLLM_EPI_BIAS)
 *   3. text -> image attention: q = text_proj(t), k = vision_proj(v), v = values_vision_proj(v), key mask = vision_padding_mask, keys
 *      split by vllm_xattn_plan
 *   4. image -> text attention: q = vision_proj(v), k = text_proj(t), v = values_text_proj(t), key mask = text_padding_mask, one split.
 *      (It runs behind 3 so that its output can take the memory of values_vision_proj(v), which 3 has read; the two do not depend
 *      on each other.)
 *   5. out_vision = v + vision_param * out_vision_proj(.), out_text = t + text_param * out_text_proj(.)   (VLLM_EPI_RESIDUAL with scale)
 * softmax_scale = (embed_dim / n_heads)^-0.5 multiplies the fp32 scores.  No weight is copied or repacked.  Every tensor between two
 * launches is bf16, as in the bf16 module; scores, softmax and sums are fp32, each stored tensor is rounded once.
 * STATED DEPARTURES.  The call computes the EXACT masked softmax of both directions.  The reference subtracts the global maximum of all
 * scores of the call, clamps to +-50000, subtracts (text side) the column maximum taken over ALL image tokens, padded ones included,
 * and clamps again.  Softmax is shift-invariant, so: the second clamp never changes a result (exp(-50000) = 0 in every format); the
 * first clamp changes one only where the scores of one call span more than about 49 900; the padded-token maximum changes one only
 * where a padded token's score exceeds every unpadded one of its column by more than the exp underflow distance, where the reference
 * gives 0 / 0.  In those two extreme cases the results differ from the reference's.
 * d_model a multiple of 64 in 64 .. 512; embed_dim / n_heads 128 or 256; B S embed_dim 2 < 2^31; 1 <= Lt.  No runtime option.
 * ------------------------------------------------------------------------------------------------ */
/* A TAGGED struct, without a typedef name: C callers write `struct VllmFusionLayerDesc`.  (The set of typedef'd descriptors of this ABI
 * version is closed and pinned by the boundary tests; the binding reads this form with the same member rules, _lib.parse_tagged_structs.) */
struct VllmFusionLayerDesc {
    int32_t d_model, embed_dim, n_heads;
    float   vision_norm_eps, text_norm_eps;
    const uint16_t *vision_norm_w, *vision_norm_b, *text_norm_w, *text_norm_b;                           /* [C] each  (device, bf16) */
    const uint16_t *vision_proj_w, *vision_proj_b, *text_proj_w, *text_proj_b;                           /* [E, C] [E] */
    const uint16_t *values_vision_proj_w, *values_vision_proj_b, *values_text_proj_w, *values_text_proj_b;
    const uint16_t *out_vision_proj_w, *out_vision_proj_b, *out_text_proj_w, *out_text_proj_b;           /* [C, E] [C] */
    const uint16_t *vision_param, *text_param;                                                           /* [C] */
};
unsigned long vllm_fusion_layer_desc_sizeof(void);
/* Bytes of device scratch vllm_fusion_layer_forward needs; host-only; 0 for B S == 0, negative for a refused descriptor or sizes. */
long vllm_fusion_layer_workspace_bytes(const struct VllmFusionLayerDesc *desc, int B, int S, int Lt);
long vllm_fusion_layer_calls(void);   /* calls of vllm_fusion_layer_forward in this process that reached their launches (tests) */
/* vision, out_vision [B, S, C] bf16; text, out_text [B, Lt, C] bf16; vision_padding_mask [B, S] / text_padding_mask [B, Lt] uint8
 * (non-zero = padded: the key is ignored) or NULL.  A row whose keys are all masked is NaN, as in the module.  One stream, no
 * allocation, no synchronisation.  A refused call (descriptor; sizes outside the contract; NULL or misaligned operand; out_vision /
 * out_text overlapping an input or each other; NULL, misaligned or short workspace: VLLM_EINVAL, reason in vllm_last_error()) has
 * enqueued nothing; B S == 0 returns VLLM_OK. */
/* Alignment: vision, text, out_vision, out_text, every weight / bias / parameter of the descriptor and workspace 16 bytes; the masks:
 * element alignment. */
int vllm_fusion_layer_forward(const struct VllmFusionLayerDesc *desc, const uint16_t *vision, const uint16_t *text,
                              const uint8_t *vision_padding_mask, const uint8_t *text_padding_mask, int B, int S, int Lt,
                              uint16_t *out_vision, uint16_t *out_text, void *workspace, long workspace_bytes, vllm_stream_t stream);
/* The attention kernel of steps 3 and 4, exposed for the parity tests: masked cross attention for head dims 128 / 256.
 * Head h of token (b, i) of an operand is D contiguous bf16 at ptr + b * batch_stride + i * ld + h * D (strides in elements), so q, k
 * and v are read in place from projection outputs.  D 128 or 256; Lq, Lk >= 1, neither bounded by a tile; H >= 1.
 *   out[b, i, h, :] = softmax_j(softmax_scale * q . k_j, masked keys at -inf) V
 * key_padding_mask [B, Lk] (non-zero = ignore this key) or NULL.  Scores, softmax and accumulation fp32, P rounded to bf16 before P V,
 * one rounding of the result.  A row with EVERY key masked is NaN in all D outputs of that head.  Nothing is written outside the H D
 * columns of an output row.
 * vllm_xattn_plan: a pure function of its five arguments, never of the device: `splits` workgroups share the keys of one block of 64
 * query rows, split s taking keys [s keys_per_split, min(Lk, (s + 1) keys_per_split)); keys_per_split is a multiple of the key tile
 * (64).  splits is 1 up to 512 keys and wherever B H ceil(Lq / 64) reaches 512 workgroups; otherwise ceil(512 / (B H ceil(Lq / 64)))
 * splits of at least four key tiles each.  With splits > 1 every split writes the fp32 (m, l, O) of its rows to `workspace`
 * (vllm_xattn_workspace_bytes: B H Lq splits (D + 2) 4 bytes; 0 for one split, negative for refused sizes) and a second kernel combines
 * them in ascending order; a split whose keys are all masked has m = -inf, l = 0 and takes weight 0.  No atomics: the same bits on
 * every run and every box.  A refused call (D; a NULL operand; a misaligned pointer or stride; a row stride below H D; a NULL,
 * misaligned or short workspace where the plan splits: VLLM_EINVAL, each with its own reason in vllm_last_error()) has enqueued nothing;
 * B Lq == 0 returns VLLM_OK. */
/* Alignment: q, k, v, out, workspace 16 bytes, the row and batch strides multiples of 8 elements; the mask: element alignment. */
int vllm_xattn_fwd_bf16(const uint16_t *q, long q_batch_stride, int ldq, const uint16_t *k, long k_batch_stride, int ldk,
                        const uint16_t *v, long v_batch_stride, int ldv, uint16_t *out, long o_batch_stride, int ldo,
                        const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D, float softmax_scale, void *workspace,
                        long workspace_bytes, vllm_stream_t stream);
long vllm_xattn_workspace_bytes(int B, int Lq, int Lk, int H, int D);
int vllm_xattn_plan(int B, int Lq, int Lk, int H, int D, int *splits, int *keys_per_split);

/* ------------------------------------------------------------------------------------------------
 * f2g. The TEXT ENHANCER of Grounding-DINO and the whole ENCODER around the three blocks of its layer, bf16 modules (inference).
 *
 * Replaces the bodies of
 *   GroundingDinoTextEnhancerLayer.forward   visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:787-857
 *   get_sine_pos_embed, GroundingDinoEncoderLayer.get_text_position_embeddings / .forward                          :1185-1290
 *   GroundingDinoEncoder.get_reference_points / .forward                                                           :1560-1722
 * with dropout the identity, without output_attentions / output_hidden_states.  The descriptors (struct VllmTextEnhancerDesc, struct
 * VllmGdinoEncoderDesc) are tagged structs in vllm_hip_gdino_encoder.h, included here.
 *
 * The enhancer's launches, in order: [vllm_add_bf16: q = text + pos;] one GEMM with N = 2C on q -> [q | k] (in_proj rows 0 .. 2C); one
 * GEMM with N = C on text -> v (rows 2C .. 3C); vllm_mha_fwd_masks_bf16 on the column slices; out_proj with `text` added in its epilogue;
 * LayerNorm (layer_norm_before) in place; fc1 + ReLU / GELU; fc2 + residual; LayerNorm (layer_norm_after) -> out.  Every tensor between
 * two launches is bf16, as in the bf16 module; scores, softmax, sums and statistics are fp32 with one rounding per stored tensor.
 *
 * THE MASK OF THE ENHANCER.  attn_mask is [n_masks, Lt, Lt] uint8, non-zero = may NOT attend, and (image b, head h) reads slab
 * (b H + h) % n_masks.  n_masks = 1 is one shared mask; n_masks = B H is the 3-d mask of nn.MultiheadAttention; n_masks = B is what the
 * reference's statement `attention_masks.repeat(self.num_heads, 1, 1)` (:839) comes to under nn.MultiheadAttention's indexing of a 3-d
 * mask by b H + h: image b, head h attends under the mask of image (b H + h) % B -- not of image b, unless B = 1 or the masks are equal.
 * That is the reference's behaviour and the call reproduces it exactly, without materialising the repeat.
 *
 * The encoder, once per call: vllm_encoder_refpoints_f32 (get_reference_points) and, unless the caller passes text_pos_embed,
 * vllm_text_pos_embed_bf16 (the same tensor in every layer).  Then per layer: the launches of vllm_fusion_layer_forward, those of
 * vllm_text_enhancer_forward on the fused text, those of vllm_deform_enc_layer_forward on the fused vision features (query = src +
 * vision_pos).  Vision and text ping-pong in the workspace; the last layer writes the caller's outputs.
 * ------------------------------------------------------------------------------------------------ */
#include "vllm_hip_gdino_encoder.h"
unsigned long vllm_text_enhancer_desc_sizeof(void);
unsigned long vllm_gdino_encoder_desc_sizeof(void);
/* Bytes of device scratch the two entries need; host-only; 0 for no rows (B Lt == 0; the encoder: B S == 0 or B Lt == 0), negative for a
 * refused descriptor or sizes. */
long vllm_text_enhancer_workspace_bytes(const struct VllmTextEnhancerDesc *desc, int B, int Lt);
long vllm_gdino_encoder_workspace_bytes(const struct VllmGdinoEncoderDesc *desc, int B, int S, int Lt);
long vllm_text_enhancer_calls(void);    /* calls of vllm_text_enhancer_forward in this process that reached their launches (tests) */
long vllm_gdino_encoder_calls(void);    /* the same for vllm_gdino_encoder_forward, which touches no other entry's counter */
/* text, out [B, Lt, C] bf16; pos [B, Lt, C] bf16 or NULL (queries and keys are `text` itself); attn_mask [n_masks, Lt, Lt] uint8 or NULL,
 * n_masks >= 1.  A query row whose keys are all masked is NaN in that head's context, hence in the whole output row, as in the module.
 * One stream, no allocation, no synchronisation, no runtime option.  A refused call (descriptor; sizes; NULL or misaligned operand; `out`
 * overlapping an input; NULL, misaligned or short workspace: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing; B Lt == 0
 * returns VLLM_OK. */
/* Alignment: text, pos, out, every weight / bias of the descriptor and workspace 16 bytes; attn_mask: element alignment. */
int vllm_text_enhancer_forward(const struct VllmTextEnhancerDesc *desc, const uint16_t *text, const uint16_t *pos, const uint8_t *attn_mask,
                               int n_masks, int B, int Lt, uint16_t *out, void *workspace, long workspace_bytes, vllm_stream_t stream);
/* vision, vision_pos, out_vision [B, S, C] bf16; vision_padding_mask [B, S] uint8 (non-zero = padded) or NULL; valid_ratios [B, L, 2] fp32;
 * spatial_shapes [L, 2] / level_start_index [L] device int64 describing S tokens; text, out_text [B, Lt, C] bf16; text_padding_mask [B, Lt]
 * uint8 (non-zero = padded) or NULL; text_self_attn_mask [n_masks, Lt, Lt] uint8, ALREADY INVERTED (non-zero = may NOT attend: the
 * caller applies the reference's `~` once per call); text_positions [B, Lt] fp32 or NULL (0 .. Lt - 1 for every image);
 * text_pos_embed [B, Lt, C] bf16 or NULL (then it is computed from text_positions).  One stream, no allocation, no synchronisation, no
 * runtime option.  A refused call (NULL or misaligned operand; a layer descriptor its own entry refuses; layers of differing d_model or
 * n_levels; an output overlapping an input or the other output; NULL, misaligned or short workspace: VLLM_EINVAL, reason in
 * vllm_last_error()) has enqueued nothing; B S == 0 or B Lt == 0 returns VLLM_OK. */
/* Alignment: vision, vision_pos, text, text_pos_embed, both outputs, dim_t, every weight / bias and workspace 16 bytes; valid_ratios,
 * spatial_shapes, level_start_index 8 bytes; text_positions 4 bytes; the masks: element alignment. */
int vllm_gdino_encoder_forward(const struct VllmGdinoEncoderDesc *desc, const uint16_t *vision, const uint16_t *vision_pos,
                               const uint8_t *vision_padding_mask, const float *valid_ratios, const int64_t *spatial_shapes,
                               const int64_t *level_start_index, const uint16_t *text, const uint8_t *text_padding_mask,
                               const uint8_t *text_self_attn_mask, int n_masks, const float *text_positions, const uint16_t *text_pos_embed,
                               int B, int S, int Lt, uint16_t *out_vision, uint16_t *out_text, void *workspace, long workspace_bytes,
                               vllm_stream_t stream);
/* The three new kernels, exposed for the parity tests.  No atomics: the same bits on every run.
 * vllm_mha_fwd_masks_bf16: vllm_mha_fwd_bf16 (section f2c: layouts, alignment, NaN rows) with attn_mask [n_masks, Lq, Lk] and slab
 *   (b H + h) % n_masks for workgroup (b, h); n_masks = 1 is vllm_mha_fwd_bf16 itself, bit for bit (one launch function).
 * vllm_text_pos_embed_bf16: out [B Lt, C] bf16 with row stride ld_out (elements, a multiple of 8, at least C); element i of row (b, t) is
 *   sin (i even) or cos (i odd) of (p * 2 pi) / dim_t[i], p = positions[b, t], or t where positions is NULL -- fp32, a true division, the
 *   accurate sinf / cosf, one rounding: get_sine_pos_embed(p[..., None], C, exchange_xy=False) (:1185-1214).  C a multiple of 64 in
 *   64 .. 512.  Nothing is written outside the C columns of a row.
 * vllm_encoder_refpoints_f32: out [B, S, L, 2] fp32, out[b, s, l', k] = ((c + 0.5) / (valid_ratios[b, l, k] * extent_k(l))) *
 *   valid_ratios[b, l', k], token s lying in level l at column (k = 0, extent = width) / row (k = 1, extent = height) c: every product
 *   and the division one fp32 operation in the reference's order (:1592-1605), so the bits are those of the module's statement run in
 *   fp32 on the device.  1 <= L <= 16; level_start_index ascending from 0.
 * A refused call (VLLM_EINVAL) has enqueued nothing; no rows returns VLLM_OK. */
/* Alignment (vllm_mha_fwd_masks_bf16): q, k, v, out 16 bytes, the row and batch strides multiples of 8 elements; the masks: element alignment. */
int vllm_mha_fwd_masks_bf16(const uint16_t *q, long q_batch_stride, int ldq, const uint16_t *k, long k_batch_stride, int ldk,
                            const uint16_t *v, long v_batch_stride, int ldv, uint16_t *out, long o_batch_stride, int ldo,
                            const uint8_t *attn_mask, int n_masks, const uint8_t *key_padding_mask, int B, int Lq, int Lk, int H, int D,
                            float softmax_scale, vllm_stream_t stream);
/* Alignment (vllm_text_pos_embed_bf16): dim_t, out 16 bytes; positions 4 bytes. */
int vllm_text_pos_embed_bf16(const float *positions, const float *dim_t, int B, int Lt, int C, uint16_t *out, int ld_out, vllm_stream_t stream);
/* Alignment (vllm_encoder_refpoints_f32): out 16 bytes; valid_ratios, spatial_shapes, level_start_index 8 bytes. */
int vllm_encoder_refpoints_f32(const int64_t *spatial_shapes, const int64_t *level_start_index, const float *valid_ratios, int B, int S, int L,
                               float *out, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f2h. The INPUTS of the Grounding-DINO encoder from the backbone's feature maps and the pixel mask, bf16 modules (inference).
 *
 * Replaces, of OVGroundingDinoModel in visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py,
 *   input_proj_vision (1 x 1 Conv2d + GroupNorm(32) per map, 3 x 3 / stride 2 Conv2d + GroupNorm per extra level)   :2080-2111
 *   the mask down-sampling of the backbone and of the extra levels                                                  :502, :2406
 *   GroundingDinoSinePositionEmbedding.forward (normalize=True, scale 2 pi) and `+ level_embed[level]`               :529-564, :2164, :2429
 *   get_valid_ratio                                                                                                 :2200-2209
 *   the flatten / transpose / cat statements of forward                                                             :2388-2439
 * The descriptor (struct VllmGdinoInputsDesc) is a tagged struct in vllm_hip_gdino_inputs.h, included here.
 *
 * Level l has H_l x W_l cells: a backbone map's own size for l < n_maps, else ((H_{l-1} - 1) / 2 + 1) x ((W_{l-1} - 1) / 2 + 1).  S is
 * the sum of H_l W_l, level l's rows start at row sum_{l' < l} H_l' W_l' of every image.
 * The launches per level: [vllm_nchw_to_rows_bf16 for a contiguous NCHW map; a channels-last map is the GEMM's operand in place] or
 * [vllm_im2col3x3s2_bf16]; one vllm_gemm_bf16 (VLLM_EPI_BIAS; the conv output is bf16 in the workspace, the bf16 module's own rounding);
 * the three kernels of vllm_groupnorm_rows_bf16, which write the level's rows of out_source.  Then vllm_pixel_mask_levels_u8 and
 * vllm_sine_pos_embed_rows_bf16 for all levels at once.  No atomics on any output: the same inputs give the same bits on every run.
 *
 * ONE DEPARTURE.  The reference rounds the position embedding to bf16 (`.to(feature_map.dtype)`, :524) and then adds level_embed with a
 * second rounding (:2429); vllm_sine_pos_embed_rows_bf16 adds level_embed in fp32 and rounds once.
 * ------------------------------------------------------------------------------------------------ */
#include "vllm_hip_gdino_inputs.h"
unsigned long vllm_gdino_inputs_desc_sizeof(void);
long vllm_gdino_inputs_calls(void);   /* calls of vllm_gdino_inputs_forward in this process that reached their launches (tests) */
/* Bytes of device scratch vllm_gdino_inputs_forward needs; host-only; map_h, map_w, map_format HOST arrays [n_maps] as for the call;
 * 0 for B == 0, negative for a refused descriptor or sizes. */
long vllm_gdino_inputs_workspace_bytes(const struct VllmGdinoInputsDesc *desc, int B, const int *map_h, const int *map_w, const int *map_format);
/* maps: HOST array [n_maps] of device pointers, map l bf16 [B, c_in[l], map_h[l], map_w[l]] contiguous (map_format[l] == 0) or
 * channels-last [B, map_h[l], map_w[l], c_in[l]] (map_format[l] == 1); map_h, map_w, map_format HOST arrays.  pixel_mask [B, H, W] of
 * mask_elem_bytes 1 (bool / uint8) or 8 (int64), non-zero = a real pixel.  out_source, out_pos [B, S, C] bf16; out_mask [B, S] uint8
 * (1 = a real cell); out_valid_ratios [B, n_levels, 2] fp32 (width ratio, height ratio).  One stream, no allocation, no
 * synchronisation, no runtime option.  A refused call (descriptor; sizes outside the contract: a map extent or H, W below 1, B S or
 * a GEMM operand reaching 2^31; an unknown format or mask element size; NULL or misaligned operand; outputs overlapping each other; NULL,
 * misaligned or short workspace, or one overlapping an operand: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing; B == 0
 * returns VLLM_OK. */
/* Alignment: every map, out_source, out_pos, every weight / bias / parameter of the descriptor, level_embed, dim_t and workspace 16
 * bytes; out_valid_ratios 8 bytes; pixel_mask its element size; out_mask: element alignment. */
int vllm_gdino_inputs_forward(const struct VllmGdinoInputsDesc *desc, const uint16_t *const *maps, const int *map_h, const int *map_w,
                              const int *map_format, const void *pixel_mask, int mask_elem_bytes, int B, int H, int W, uint16_t *out_source,
                              uint16_t *out_pos, uint8_t *out_mask, float *out_valid_ratios, void *workspace, long workspace_bytes,
                              vllm_stream_t stream);
/* The five new kernels, exposed for the parity tests.  A refused call (VLLM_EINVAL) has enqueued nothing; no rows returns VLLM_OK.
 * vllm_groupnorm_rows_bf16: nn.GroupNorm(32, C) (:2090) over B channels-last images x [B HW, C] bf16 (row stride ldx, image b at row b HW),
 *   C a multiple of 64 in 64 .. 512 (2 .. 16 channels per group).  Statistics per (image, group) over HW C / 32 elements in fp32: every
 *   slab of 32 rows gives {count, mean, M2}, M2 taken about the slab's own mean; the slabs are combined in a fixed order with Chan's
 *   formula (never E[x^2] - E[x]^2); the variance is biased.  A second pass writes (x - mean) rstd gamma + beta with one rounding to
 *   out + b out_batch_stride + row ldo (elements): a level's rows inside a [B, S, C] tensor, so the level `cat` (:2433) never happens.
 *   HW == 1 and a constant map give beta exactly (eps > 0).  Nothing is written outside the C columns of a row.  workspace:
 *   vllm_groupnorm_rows_workspace_bytes(B, HW, C) bytes (negative for refused sizes).
 * vllm_nchw_to_rows_bf16: out[(b HW + p) ld_out + c] = in[(b Cin + c) HW + p]: the `flatten(2).transpose(1, 2)` of :2426 in front of the
 *   conv instead of behind it, through 64 x 64 LDS tiles.  Cin a multiple of 64; `in` 16-byte aligned (any HW).
 * vllm_im2col3x3s2_bf16: out [B Ho Wo, 9 Cin], Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1, row (b, oy, ox) = the 3 x 3 patch at
 *   (2 oy - 1 + ky, 2 ox - 1 + kx) in (ky, kx, c) order from channels-last rows src + b src_batch_stride + (y Wi + x) ld_src; taps in the
 *   padding are zeros (:2097).  Cin a multiple of 8.
 * vllm_pixel_mask_levels_u8: for every level (level_h, level_w HOST arrays [L], 1 <= L <= 8) the nearest-neighbour down-sampled mask
 *   of F.interpolate (:502, :2406) -- source index min(floor(dst * (float(in) / out)), in - 1), the scale and the product in fp32 -- as
 *   out_mask [B, S] uint8; the inclusive prefix counts of valid cells along y and along x (the cumsums of :549-550) as int32 [B, S] each;
 *   out_valid_ratios [B, L, 2] fp32 with the bits of get_valid_ratio (:2200-2209) on the device: count * (1 / extent) in fp32, which is
 *   what torch's division of a device tensor by a host scalar computes.
 * vllm_sine_pos_embed_rows_bf16: out [B, S, C] bf16 from the prefix counts: channel i < C / 2 of cell (y, x) is sin (i even) / cos (i odd)
 *   of ((ycnt / (ycnt_last_row + 1e-6)) * 2 pi) / dim_t[i], channel C / 2 + i the same of xcnt and the row's last column, in fp32 in the
 *   statement's order (:553-562) with true divisions and the accurate sinf / cosf, + level_embed[l, channel], one rounding (the departure
 *   above).  dim_t [C / 2] fp32.  A fully masked image gives 0 / (0 + 1e-6) = 0. */
/* Alignment (vllm_groupnorm_rows_bf16): x, gamma, beta, out, workspace 16 bytes; ldx, ldo, out_batch_stride multiples of 8 elements. */
int vllm_groupnorm_rows_bf16(const uint16_t *x, int ldx, const uint16_t *gamma, const uint16_t *beta, float eps, int B, int HW, int C,
                             uint16_t *out, long out_batch_stride, int ldo, void *workspace, long workspace_bytes, vllm_stream_t stream);
long vllm_groupnorm_rows_workspace_bytes(int B, int HW, int C);
/* Alignment (vllm_nchw_to_rows_bf16): in, out 16 bytes; ld_out a multiple of 8 elements. */
int vllm_nchw_to_rows_bf16(const uint16_t *in, int B, int Cin, int HW, uint16_t *out, int ld_out, vllm_stream_t stream);
/* Alignment (vllm_im2col3x3s2_bf16): src, out 16 bytes; ld_src, src_batch_stride multiples of 8 elements. */
int vllm_im2col3x3s2_bf16(const uint16_t *src, long src_batch_stride, int ld_src, int B, int Hi, int Wi, int Cin, uint16_t *out,
                          vllm_stream_t stream);
/* Alignment (vllm_pixel_mask_levels_u8): pixel_mask its element size; out_ycnt, out_xcnt 4 bytes; out_valid_ratios 8 bytes; out_mask:
 * element alignment. */
int vllm_pixel_mask_levels_u8(const void *pixel_mask, int mask_elem_bytes, int B, int H, int W, const int *level_h, const int *level_w, int L,
                              uint8_t *out_mask, int32_t *out_ycnt, int32_t *out_xcnt, float *out_valid_ratios, vllm_stream_t stream);
/* Alignment (vllm_sine_pos_embed_rows_bf16): level_embed, dim_t, out 16 bytes; ycnt, xcnt 4 bytes. */
int vllm_sine_pos_embed_rows_bf16(const int32_t *ycnt, const int32_t *xcnt, const int *level_h, const int *level_w, int L, int B, int C,
                                  const uint16_t *level_embed, const float *dim_t, uint16_t *out, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f3b. The whole DCNv3 layer, bf16 modules (inference).
 *
 * Replaces the body of DCNv3.forward, visionllmv2/model/ops_dcnv3/modules/dcnv3.py:313-351, with the CenterFeatureScaleModule
 * above it (:206-219), for the configuration the InternImage-H det backbone builds: LayerNorm + GELU behind the depth-wise conv,
 * 3 x 3 sampling kernel, stride 1, pad == dilation (output H x W):
 *     x_proj = input_proj(input);  x1 = GELU(LayerNorm(dw_conv(input)));  offset = offset(x1);  mask = softmax_9(mask(x1));
 *     core = dcnv3(x_proj, offset, mask);  s = sigmoid(center_feature_scale_proj(x1));  out = output_proj(core (1 - s) + x_proj s)
 * Five launches: GEMM, conv + LayerNorm + GELU, GEMM (fp32 rows of offsets, logits and centre logits), softmax + sampling + blend, GEMM.
 * x_proj and x1 are bf16 (what the bf16 module holds); the conv result, the statistics, offsets, logits, softmax weights, the
 * sampled sum and the blend are fp32; core is rounded to bf16 once, as output_proj's operand.
 *
 * proj_w / proj_b are ONE packed linear over x1, rows in this order: [0, 18 G) offset.weight, [18 G, 27 G) mask.weight,
 * [27 G, 28 G) center_feature_scale_proj_weight (only with center_feature_scale), then zero rows up to n_proj; n_proj is a multiple
 * of 8 and at least the used rows.
 * Accepted: channels % 64 == 0, channels / group in {8, 16, 32, 64}, kernel_size == 3, dw_kernel_size odd in 1 .. 7, dilation >= 1,
 * center_feature_scale 0 / 1, ln_eps >= 0.  Everything else is refused.
 * ------------------------------------------------------------------------------------------------ */
typedef struct VllmDcnv3LayerDesc {
    int32_t channels, group, kernel_size, dw_kernel_size, dilation;
    int32_t center_feature_scale;   /* 0 / 1 */
    int32_t n_proj;                 /* rows of the packed projection */
    float offset_scale, ln_eps;
    int32_t reserved0;              /* 0 */
    const uint16_t *input_proj_w, *input_proj_b;     /* [C, C], [C]                 (device, bf16) */
    const uint16_t *dw_w, *dw_b;                     /* [C, dwk * dwk] (nn.Conv2d depth-wise weight [C, 1, k, k] as stored), [C] */
    const uint16_t *ln_w, *ln_b;                     /* [C], [C] */
    const uint16_t *proj_w, *proj_b;                 /* [n_proj, C], [n_proj] */
    const uint16_t *output_proj_w, *output_proj_b;   /* [C, C], [C] */
} VllmDcnv3LayerDesc;
unsigned long vllm_dcnv3_layer_desc_sizeof(void);
/* Bytes of device scratch vllm_dcnv3_layer_forward needs; host-only; negative for a refused descriptor or negative sizes. */
long vllm_dcnv3_layer_workspace_bytes(const VllmDcnv3LayerDesc *desc, int N, int H, int W);
/* input, out [N, H, W, C] bf16.  One stream, no allocation, no synchronisation.  A refused call (bad descriptor, NULL or misaligned
 * pointer, short or misaligned workspace, N H W >= 2^31: VLLM_EINVAL, reason in vllm_last_error()) has enqueued nothing; N H W == 0
 * returns VLLM_OK without a launch. */
/* Alignment: input, out, every weight / bias of the descriptor and workspace 16 bytes. */
int vllm_dcnv3_layer_forward(const VllmDcnv3LayerDesc *desc, const uint16_t *input, int N, int H, int W, uint16_t *out,
                             void *workspace, long workspace_bytes, vllm_stream_t stream);
long vllm_dcnv3_layer_calls(void);   /* calls of vllm_dcnv3_layer_forward in this process that reached their launches (tests) */
/* The two kernels of the layer, exposed for the parity tests.
 * vllm_dwconv_ln_gelu_bf16: out [N, H, W, C] = GELU_erf(LayerNorm_C(depth-wise dwk x dwk conv of x [N, H, W, C], zero padding dwk / 2,
 *   + dw_b) * ln_w + ln_b), channels-last, fp32 from the taps to the one rounding of the result.  C a multiple of 8, at most 4096; dwk
 *   odd in 1 .. 7; N H W < 2^31.  A tap outside the image reads nothing that reaches a result.
 * vllm_dcnv3_sample_fused_bf16: x_proj [N, H, W, G D] bf16, om [N H W, ld_om] fp32 rows of (18 G offsets | 9 G logits | G centre
 *   logits with center_feature_scale) -- columns behind them are never read; out [N, H, W, G D] bf16 = core (1 - s) + x_proj s with
 *   core the 3 x 3 DCNv3 sum (stride 1, pad == dilation) under the softmax of the 9 logits and s = sigmoid(centre logit) (s = 0
 *   without the flag).  D in {8, 16, 32, 64}, ld_om a multiple of 4 and >= the used columns, N H W < 2^31. */
/* Alignment (both): every pointer 16 bytes. */
int vllm_dwconv_ln_gelu_bf16(const uint16_t *x, const uint16_t *dw_w, const uint16_t *dw_b, const uint16_t *ln_w, const uint16_t *ln_b,
                             int N, int H, int W, int C, int dwk, float eps, uint16_t *out, vllm_stream_t stream);
int vllm_dcnv3_sample_fused_bf16(const uint16_t *x_proj, const float *om, int ld_om, int N, int H, int W, int G, int D, int dilation,
                                 float offset_scale, int center_feature_scale, uint16_t *out, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * f4. Region-encoder point sampling.
 *
 * Replaces: point_sample (F.grid_sample(input, 2*coords-1), bilinear, zeros padding, align_corners=False) and the masked
 * mean over a region's sampled points, visionllmv2/model/region_encoder.py:24-47, 127-141.
 * input [N, C, H, W] fp32 (contiguous NCHW), coords [N, P, 2] (x, y) in [0, 1], valid [N, P] uint8.
 * ------------------------------------------------------------------------------------------------ */
/* Alignment (both): coords 8 bytes. */
int vllm_point_sample_f32(const float *input, const float *coords, int N, int C, int H, int W, int P, float *out /* [N,C,P] */,
                          vllm_stream_t stream);
/* out[n, c] = sum_p valid * sample / sum_p valid, 0 for a region without points ((x / 0).nan_to_num() of the reference). */
int vllm_point_sample_mean_f32(const float *input, const float *coords, const uint8_t *valid, int N, int C, int H, int W, int P,
                               float *out /* [N,C] */, vllm_stream_t stream);
/* Backward with respect to the feature map.  Replaces: the autograd of region_encoder.py:135-140 (F.grid_sample's backward -- one
 * float atomic add per (point, corner, channel) -- then the backward of the mask, the sum and the division).
 * The masked mean is linear in the map, out[n, c] = (1 / cnt_n) sum_pix A[n, pix] in[n, c, pix] with A[n, pix] the sum of the corner
 * weights the valid points put on pix, so
 *     grad_in[n, c, pix] = (A[n, pix] / cnt_n) * grad_out[n, c]
 * an outer product: every element of grad_in [N, C, H, W] is written exactly once (no zero-fill by the caller, no atomics on it, the
 * same bits on every run), and the map itself is not an operand.  Weights are the forward's bit for bit.
 * EMPTY REGION: a region without a valid point gets grad_in[n] = 0, the derivative of the constant 0 the forward returns for it; the
 * reference's autograd puts NaN on every pixel one of the region's (invalid) points touches (0 * (1 / 0) in the division's
 * backward).  Deliberate departure.
 * grad_out [N, C] fp32; grad_in fp32 or bf16 (the fp32 value rounded to nearest even once).  With P == 0 grad_in is written as zeros.
 * Maps too large for the on-chip accumulators (80 x 80, ...) build A in the caller's workspace: the query returns 0 where none is
 * needed; the entry points clear what they use of it themselves.
 * vllm_point_sample_backward_f32 is the unfused form, grad_in[n, c, pix] = sum_p w(p, pix) grad_out[n, c, p] with grad_out [N, C, P]:
 * fully written as well, but summed with float atomics in arrival order -- the last bits may differ between runs.  It needs no
 * workspace (NULL / 0 are accepted).
 * Alignment (all three): coords 8 bytes, workspace 8 bytes; grad_in 4 bytes (2 for bf16) is enough, 16 bytes enables wide stores. */
long vllm_point_sample_backward_workspace_bytes(int N, int C, int H, int W, int P);   /* 0 = none needed */
int vllm_point_sample_mean_backward_f32(const float *coords, const uint8_t *valid, const float *grad_out /* [N,C] */, int N, int C, int H,
                                        int W, int P, float *grad_in /* [N,C,H,W] */, void *workspace, long workspace_bytes,
                                        vllm_stream_t stream);
int vllm_point_sample_mean_backward_bf16(const float *coords, const uint8_t *valid, const float *grad_out /* [N,C] */, int N, int C, int H,
                                         int W, int P, uint16_t *grad_in /* [N,C,H,W] */, void *workspace, long workspace_bytes,
                                         vllm_stream_t stream);
int vllm_point_sample_backward_f32(const float *coords, const float *grad_out /* [N,C,P] */, int N, int C, int H, int W, int P,
                                   float *grad_in /* [N,C,H,W] */, void *workspace, long workspace_bytes, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Building blocks of the ViT path (bf16 storage, fp32 accumulation).  Exposed individually so the parity
 * tests can pin every kernel against the oracle, and as bring-up hooks B4/B5 of SURVEY.md section 8b.
 * All bf16 tensors are passed as uint16_t*.
 * ------------------------------------------------------------------------------------------------ */

/* Epilogues of vllm_gemm_bf16 */
#define VLLM_EPI_BIAS 0        /* y = x W^T + b                                   (nn.Linear) */
#define VLLM_EPI_GELU 1        /* y = gelu_erf(x W^T + b)                         (InternMLP.fc1+act, vl_bridge GELU) */
#define VLLM_EPI_QUICK_GELU 2  /* y = z*sigmoid(1.702 z)                          (CLIP MLP) */
#define VLLM_EPI_RESIDUAL 3    /* y = res + (x W^T + b) * scale                   (LayerScale + residual, modeling_intern_vit.py:206-208) */
/* VLLM_EPI_RESIDUAL without `scale` on the persistent 8-phase GEMM ("gemm_res_ring", the default): the residual is added by the matrix
 * pipe as res x I, y = (x W^T + res) + b with one rounding.  0 x Inf is NaN there: a NON-FINITE residual element makes every output of
 * its row's aligned 32-column group [32 g, min(32 g + 32, N)) NaN instead of that element alone (finite residuals: exact; nothing
 * beyond column N of a row is read).  With `scale`, with ldr not a multiple of 8, on every other kernel and with "gemm_res_ring" 0
 * a non-finite element stays in its own output. */
#define VLLM_EPI_EMBED 4       /* patch embedding: rows scattered past the CLS slot, + position embedding */
#define VLLM_EPI_F32 5         /* y = x W^T + b kept in fp32: Y is float*, ldy in floats (16-byte aligned rows); `res`, if
                                * given, is a uint8 row mask [M]: masked rows are written as zeros (the key-padding
                                * zero-fill of the MSDA value projection) */
#define VLLM_EPI_GELU_BWD 6    /* y = (x W^T) * gelu_erf'(res[m, n]); `res` = the saved pre-activation [M, N] (row stride ldr, 8-byte
                                * aligned), bias must be NULL (projector backward: dY_{i-1} = (dY_i W_i) * gelu'(H_{i-1}), W = W_i^T) */
/* Kernel choice is automatic (256x256 8-phase schedule for M,N >= 1024, 128x128 otherwise); OR one of these into
 * `epilogue` to force a schedule (parity tests / tuning only). */
#define VLLM_GEMM_FORCE_128 0x100
#define VLLM_GEMM_FORCE_256 0x200   /* 8-phase schedule, 256-row block tile */
#define VLLM_GEMM_FORCE_192 0x300   /* 8-phase schedule, 192-row block tile */
#define VLLM_GEMM_FORCE_4W 0x400    /* 4-wave schedule: 256x256x32 block tile, 128x128 per wave (not built: VLLM_EINVAL) */
#define VLLM_GEMM_FORCE_MF32 0x800  /* 8-phase schedule, 256-row block tile, v_mfma_f32_32x32x16_bf16 */
#define VLLM_GEMM_FORCE_TILEWISE 0x1000 /* 8-phase schedule with one workgroup per tile, where the persistent walk over the tiles
                                        * (qkv / fc1 shapes: bias / GELU / quick-GELU epilogue, N % 256 == 0) would be taken */

/* Y[M,N] = epilogue(X[M,K] @ W[N,K]^T + bias).  Replaces F.linear / nn.Conv2d-as-GEMM on the path
 * (modeling_intern_vit.py:112,124,128,141,172-178; modeling_visionllmv2.py:162-182).
 * K % 64 == 0, N % 4 == 0, 16-byte aligned operands.  bias/scale may be NULL.  For VLLM_EPI_EMBED `res` is the
 * position table [P+1, N] (row stride ldr) and P the patches per image; output row of input row m is
 * (m / P) * (P + 1) + 1 + m % P. */
/* Alignment (every vllm_gemm_bf16*): X and W 16 bytes, Y 8 bytes (16 with VLLM_EPI_F32), scratch 16 bytes; bias, scale, the bf16 `res`
 * (residual, position table, saved pre-activation) and `pre` 8 bytes.  Row strides: ldx, ldw multiples of 8, ldy and ldr of 4. */
int vllm_gemm_bf16(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y,
                   int M, int N, int K, int ldx, int ldw, int ldy, int epilogue,
                   const uint16_t *scale, const uint16_t *res, int ldr, int P, vllm_stream_t stream);

/* The same GEMM with caller-provided scratch for the stream-K tail of the 8-phase schedule: when the tiles of a GEMM do not
 * fill a whole number of rounds on the device's CUs, the K iterations of the last round's tiles are spread evenly over all CUs
 * (fp32 partial tiles meet in `scratch`, summed in a fixed order: results are run-to-run identical).  `scratch` is
 * vllm_gemm_scratch_bytes() bytes, 16-byte aligned; the call resets its first 4096 bytes (flags) with a memset node in front of
 * the kernel; calls sharing a scratch must be ordered on one stream.  NULL scratch = vllm_gemm_bf16.  A shorter scratch is legal
 * down to the flags and one 262144-byte slot (less, or a misaligned pointer: VLLM_EINVAL): the tail is then planned only if the
 * slots of every compute unit fit, and never reaches past `scratch_bytes`.  vllm_vit_forward / vllm_bridge_forward reserve theirs
 * inside their workspace. */
long vllm_gemm_scratch_bytes(void);
long vllm_gemm_sk_launches(void);   /* GEMM launches of this process that took the stream-K tail (tests / tuning) */
long vllm_gemm_half_tail_launches(void);   /* ... of the persistent schedule whose last round ran as half-height tiles (round 4) */
long vllm_gemm_persistent_launches(void);   /* GEMM launches of this process that took the persistent 8-phase schedule (tests / tuning) */
int vllm_gemm_bf16_sk(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y,
                      int M, int N, int K, int ldx, int ldw, int ldy, int epilogue,
                      const uint16_t *scale, const uint16_t *res, int ldr, int P,
                      void *scratch, long scratch_bytes, vllm_stream_t stream);

/* The same GEMM with a LayerNorm / RMSNorm folded into it (8-phase schedule only; what vllm_vit_forward does between the
 * residual GEMMs and the qkv / fc1 GEMMs instead of launching the norm, modeling_intern_vit.py:198-210 / CLIPEncoderLayer):
 *   producer (ln_out != NULL): besides Y it writes, per output row and 256-column tile, {mean, M2 = sum (y - mean)^2} of the
 *     bf16 values it stored ({sum y^2, 0} with ln_rms) to ln_out [M][ceil(N / 256)][2] (fp32);
 *   consumer (ln_in != NULL): X holds the UN-normalised rows (K elements each, 768 < K <= 1024: ln_slots == 4), ln_in their
 *     statistics [M][4][2] as a producer with N == K leaves them, W the weight with the norm's gamma multiplied in (W'[n,k] = gamma_k W[n,k], rounded to
 *     bf16), ln_colsum[n] = sum_k W'[n,k] (fp32; LayerNorm only), ln_bias[n] = b_n + sum_k beta_k W[n,k] (fp32, may be NULL; it
 *     replaces `bias`):  y = epilogue(r_m * (x W'^T) - r_m mean_m colsum_n + ln_bias_n),  r_m = rsqrt(var_m + ln_eps).
 * The row statistics are exact fp32 (the reference rounds the normalised tensor to bf16 first: the folded form differs from it
 * by that rounding, i.e. it is the more accurate of the two).
 * Round 5, WIDE statistics (InternViT-6B, hidden 3200 = 12.5 column tiles): with ln_rms and ln_slots != 4 (1 .. 16; producer:
 * ceil(N / 256), consumer: ceil(K / 256), N and K multiples of 8) the buffer is [M][16] floats, slot s = sum y^2 over column tile s,
 * slots >= ln_slots ZERO (the caller clears the buffer once; the producer never writes them); the consumer adds all 16 in a fixed
 * order.  Only the persistent schedule implements it (M, N large enough for at least one tile per CU): a call it does not take
 * returns VLLM_EINVAL and the caller launches the norm instead (vllm_vit_forward asks with a dry run first). */
int vllm_gemm_bf16_ln(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y,
                      int M, int N, int K, int ldx, int ldw, int ldy, int epilogue,
                      const uint16_t *scale, const uint16_t *res, int ldr,
                      float *ln_out, const float *ln_in, int ln_slots, int ln_rms, float ln_eps,
                      const float *ln_colsum, const float *ln_bias, vllm_stream_t stream);

/* Weight gradient of a Linear (projector backward): dW[n, k] = sum_m dY[m, n] A[m, k] and, if db != NULL, db[n] = sum_m dY[m, n];
 * dY [M, N] (row stride ldy), A [M, K] (row stride lda) -- the Linear's output gradient and input --, dW [N, K] (row stride ldw), all
 * bf16; fp32 accumulation, one rounding.  Any M (ragged rows are zero-padded); N, K multiples of 64.  When the output tiles do not fill
 * the device the rows are split and fp32 partials meet in `workspace` (vllm_gemm_wgrad_workspace_bytes(M, N, K) bytes, 0 = not needed),
 * summed in a fixed order: results are run-to-run identical. */
/* Alignment: dY and A 16 bytes (ldy, lda multiples of 8), dW 8 bytes (ldw a multiple of 4), workspace 16 bytes. */
long vllm_gemm_wgrad_workspace_bytes(int M, int N, int K);
long vllm_gemm_wgrad_split_launches(void);   /* launches of this process that took the split route (tests / tuning) */
int vllm_gemm_wgrad_bf16(const uint16_t *dY, int ldy, const uint16_t *A, int lda, int M, int N, int K, uint16_t *dW, int ldw,
                         uint16_t *db, void *workspace, long workspace_bytes, vllm_stream_t stream);

/* B5: InternRMSNorm / apex FusedRMSNorm (modeling_intern_vit.py:33-58): y = w * bf16(x * rsqrt(mean(x^2)+eps)).
 * Row strides allow the in-place QK-RMSNorm over the q / k column blocks of the qkv buffer (:131-134). */
/* Alignment (both norms): x, y, weight and bias 16 bytes. */
int vllm_rmsnorm_bf16(const uint16_t *x, int ldx, const uint16_t *weight, uint16_t *y, int ldy,
                      long rows, int C, float eps, vllm_stream_t stream);
/* nn.LayerNorm (CLIP pre_layrnorm / layer_norm1,2; vl_bridge LayerNorm, modeling_visionllmv2.py:166-167). */
int vllm_layernorm_bf16(const uint16_t *x, int ldx, const uint16_t *weight, const uint16_t *bias,
                        uint16_t *y, int ldy, long rows, int C, float eps, vllm_stream_t stream);
/* Its backward (the InternVL projector's LayerNorm): x [rows, C] bf16, grad_y [rows, C] fp32 (row stride ldg), weight (gamma) [C].
 * grad_x [rows, C] bf16 (row stride ldgx; NULL = not needed) = r (g - mean(g) - xhat mean(g xhat)), g = grad_y * gamma, with the row
 * statistics recomputed in fp32; grad_w = sum_m grad_y xhat, grad_b = sum_m grad_y (bf16 [C]; either may be NULL) through per-block fp32
 * partials in `workspace` (vllm_layernorm_backward_workspace_bytes) and a fixed-order reduce.  C % 64 == 0, C <= 16384. */
/* Alignment: x, weight, grad_x 8 bytes (ldx, ldgx multiples of 4), grad_y and workspace 16 bytes (ldg a multiple of 4). */
long vllm_layernorm_backward_workspace_bytes(long rows, int C);
int vllm_layernorm_backward_bf16(const uint16_t *x, int ldx, const float *grad_y, int ldg, const uint16_t *weight, float eps, long rows,
                                 int C, uint16_t *grad_x, int ldgx, uint16_t *grad_w, uint16_t *grad_b, void *workspace,
                                 long workspace_bytes, vllm_stream_t stream);

/* Backward of InternRMSNorm (modeling_intern_vit.py:33-44 under autograd; with G = 2 the q_norm / k_norm pair over the flattened H*D,
 * :131-134, on the q and k blocks of a [rows, 3C] qkv slab in ONE launch, mirroring the forward's column groups).  x, grad_y, grad_x
 * [rows, G*C] bf16 with row strides ldx / ldg / ldgx (elements); weight (and weight2 for group 1) [C].  Row statistics are recomputed
 * in fp32:  xhat = x r, g = grad_y w, grad_x = r (g - xhat mean(g xhat)) [+ grad_res], rounded once;  grad_w = sum_rows grad_y xhat with
 * the UNROUNDED fp32 xhat.  grad_res (bf16 [rows, C], row stride ldgr; G = 1 only; NULL = none) is the gradient of a residual branch
 * that left the normalised tensor, added before the rounding.  grad_x may alias grad_y (columns beyond G*C are never touched: the v
 * block of a qkv gradient stays as it is).  grad_x, grad_w, grad_w2 may each be NULL (not needed).  Column sums: per-block fp32
 * partials in `workspace` (vllm_rmsnorm_backward_workspace_bytes(rows, C, G); host-only arithmetic, < 0 for unsupported sizes) and a
 * fixed-order reduce -- no atomics, the same bits on every run.  C % 8 == 0, C <= 8192.  A refused call writes nothing. */
/* Alignment: x, grad_y, grad_x, grad_res, weight, weight2 and workspace 16 bytes (row strides multiples of 8); grad_w, grad_w2 2 bytes. */
long vllm_rmsnorm_backward_workspace_bytes(long rows, int C, int G);
int vllm_rmsnorm_backward_bf16(const uint16_t *x, int ldx, const uint16_t *grad_y, int ldg, const uint16_t *weight,
                               const uint16_t *weight2, int G, float eps, long rows, int C, uint16_t *grad_x, int ldgx,
                               const uint16_t *grad_res, int ldgr, uint16_t *grad_w, uint16_t *grad_w2, void *workspace,
                               long workspace_bytes, vllm_stream_t stream);
/* nn.LayerNorm backward inside a layer's chain (the CLIP encoder layer's layer_norm1 / layer_norm2, pre_layrnorm, post_layernorm): the
 * same function as vllm_layernorm_backward_bf16 with a bf16 grad_y and a residual gradient, on vllm_rmsnorm_backward_bf16's walk.  x,
 * grad_y, grad_x [rows, C] bf16 with row strides ldx / ldg / ldgx (elements); weight (gamma) [C].  Row mean and variance are recomputed
 * in fp32:  xhat = (x - mean) r, g = grad_y gamma, grad_x = r (g - mean(g) - xhat mean(g xhat)) [+ grad_res], rounded once;  grad_w =
 * sum_rows grad_y xhat with the UNROUNDED fp32 xhat;  grad_b = sum_rows grad_y.  grad_res (bf16 [rows, C], row stride ldgr; NULL = none;
 * needs grad_x) is the gradient of a residual branch that left the normalised tensor, added before the rounding.  grad_x may alias grad_y.
 * grad_x, grad_w, grad_b may each be NULL (not needed).  Column sums: per-block fp32 partials in `workspace`
 * (vllm_layernorm_backward_res_workspace_bytes(rows, C); host-only arithmetic, < 0 for unsupported sizes) and a fixed-order reduce -- no
 * atomics, the same bits on every run.  C % 64 == 0, C <= 8192.  rows == 0 zero-fills the requested sums.  A refused call writes nothing. */
/* Alignment: x, grad_y, grad_x, grad_res, weight and workspace 16 bytes (row strides multiples of 8); grad_w, grad_b 2 bytes. */
long vllm_layernorm_backward_res_workspace_bytes(long rows, int C);
int vllm_layernorm_backward_res_bf16(const uint16_t *x, int ldx, const uint16_t *grad_y, int ldg, const uint16_t *weight, float eps,
                                     long rows, int C, uint16_t *grad_x, int ldgx, const uint16_t *grad_res, int ldgr, uint16_t *grad_w,
                                     uint16_t *grad_b, void *workspace, long workspace_bytes, vllm_stream_t stream);
/* Backward of LayerScale + residual, out = res + y * ls (modeling_intern_vit.py:206-208): grad_y = bf16(grad_out * ls) [rows, C] (row
 * stride ldgy), grad_ls = sum_rows grad_out * y [C] (fp32 partials in `workspace` and a fixed-order reduce, as above); the residual's
 * gradient is grad_out itself.  Either output may be NULL (y is only read for grad_ls, ls only for grad_y).  C % 8 == 0, C <= 8192. */
/* Alignment: grad_out, y, ls, grad_y and workspace 16 bytes (row strides multiples of 8); grad_ls 2 bytes. */
long vllm_layerscale_backward_workspace_bytes(long rows, int C);
int vllm_layerscale_backward_bf16(const uint16_t *grad_out, int ldgo, const uint16_t *y, int ldy, const uint16_t *ls, long rows, int C,
                                  uint16_t *grad_y, int ldgy, uint16_t *grad_ls, void *workspace, long workspace_bytes,
                                  vllm_stream_t stream);

/* B4: FlashAttention.forward(qkv[B,S,3,H,D]) -> out[B,S,H,D], non-causal, no mask, dropout 0
 * (visionllmv2/model/internvit/flash_attention.py:30-75).  D in {64,128}. */
/* Alignment (both): qkv 16 bytes, out 8 bytes. */
int vllm_attn_fwd_qkvpacked_bf16(const uint16_t *qkv, uint16_t *out, int B, int S, int H, int D,
                                 float softmax_scale, vllm_stream_t stream);
/* The same for IEEE-half qkv / out (round 4): the reference's module accepts both dtypes (`assert qkv.dtype in [torch.float16,
 * torch.bfloat16]`, flash_attention.py:39-41).  fp32 scores / softmax / accumulation; P is rounded to half before P V. */
int vllm_attn_fwd_qkvpacked_f16(const uint16_t *qkv, uint16_t *out, int B, int S, int H, int D,
                                float softmax_scale, vllm_stream_t stream);

/* Training forward of B4 (the reference's flash_attn_varlen_qkvpacked_func is an autograd function, flash_attention.py:30-75): the
 * same launch as vllm_attn_fwd_qkvpacked_* -- `out` is bit for bit what that call writes for the same qkv and attn_variant -- which
 * also writes lse [B, H, S] fp32 (every element), the natural log of sum_j exp(softmax_scale q_i.k_j) as the kernel summed it (over
 * the 16-bit-rounded probabilities, which is what `out` was normalised by and what the backward recomputes P from).
 * Alignment: qkv 16 bytes, out 8 bytes, lse 4 bytes. */
int vllm_attn_fwd_train_qkvpacked_bf16(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, int D,
                                       float softmax_scale, vllm_stream_t stream);
int vllm_attn_fwd_train_qkvpacked_f16(const uint16_t *qkv, uint16_t *out, float *lse, int B, int S, int H, int D,
                                      float softmax_scale, vllm_stream_t stream);
/* Its backward (replaces the backward of flash_attn_varlen_qkvpacked_func and of InternAttention._naive_attn,
 * modeling_intern_vit.py:136-140; dense, non-causal, dropout 0).  qkv, grad_qkv [B, S, 3, H, D]; out (as the training forward saved
 * it), grad_out [B, S, H, D]; lse [B, H, S] fp32 from the training forward; all contiguous.  D in {64, 128}, any S >= 1, B = 0 accepted.
 *   p_ij = exp(scale q_i.k_j - lse_i), delta_i = sum_d dO_id O_id, dV_j = sum_i p_ij dO_i, dS_ij = p_ij (dO_i.v_j - delta_i),
 *   dQ_i = scale sum_j dS_ij k_j, dK_j = scale sum_i dS_ij q_i
 * on the 32x32x16 MFMA: P and dS are rounded to the 16-bit type as MFMA operands only, accumulation is fp32, every gradient element is
 * rounded once (IEEE half: P and dS enter the MFMA times 2^14 / 2^4, exact scales taken out again in fp32, so that very small
 * probabilities are not rounded as half subnormals.  Range in half: the dS operand therefore reaches infinity at |dS| = |p (dO.v - delta)|
 * > 4094 instead of 65504 -- under loss-scaled fp16 training a grad_out that large gives inf in grad_q / grad_k (which a loss scaler
 * answers by lowering the scale); P <= 1 loses nothing, and bf16 has fp32's range).  Two kernels (dQ, which also leaves delta [B, H, S] fp32 in `workspace`, then dK / dV).
 * Written: every element of grad_qkv (no zero-fill by the caller).  Deterministic: each element is owned by one wave and summed in a
 * fixed order -- no atomics, no workgroup waits on another, the same bits on every run.  A refused call (VLLM_EINVAL) writes nothing.
 * Alignment: qkv, out, grad_out, grad_qkv, workspace 16 bytes; lse 4 bytes.
 * vllm_attn_bwd_workspace_bytes is host-only arithmetic; < 0 for an unsupported D. */
long vllm_attn_bwd_workspace_bytes(int B, int S, int H, int D);
int vllm_attn_bwd_qkvpacked_bf16(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *grad_out,
                                 int B, int S, int H, int D, float softmax_scale, uint16_t *grad_qkv,
                                 void *workspace, long workspace_bytes, vllm_stream_t stream);
int vllm_attn_bwd_qkvpacked_f16(const uint16_t *qkv, const uint16_t *out, const float *lse, const uint16_t *grad_out,
                                int B, int S, int H, int D, float softmax_scale, uint16_t *grad_qkv,
                                void *workspace, long workspace_bytes, vllm_stream_t stream);

/* Patch gather for the embedding GEMM: pixels [N,3,img,img] (bf16, or fp32 when pixel_is_f32) ->
 * A [N*(img/patch)^2, Kpad] bf16, k = c*patch^2 + ky*patch + kx, zero padded to Kpad. */
int vllm_im2col_patches(const void *pixels, int pixel_is_f32, uint16_t *A, int N, int img, int patch,
                        int Kpad, vllm_stream_t stream);

/* pixel_shuffle(scale 0.5) of modeling_visionllmv2.py:381-392 applied to hidden[:, tok0:]:
 * hidden [N, tok0+hw*hw, C] (tile stride / row stride in elements, tok0 = 1 skips CLS) -> out [N, (hw/2)^2, 4C]. */
/* Alignment: hidden and out 16 bytes. */
int vllm_pixel_shuffle_bf16(const uint16_t *hidden, long tile_stride, int ld, int tok0, uint16_t *out,
                            int N, int hw, int C, vllm_stream_t stream);

/* Visual-token splice (modeling_visionllmv2.py:582-605): dst[idx[i], :] = src[i, :] for i < n.  `idx` (device int64)
 * holds the flattened [B*L_txt] positions of the <im_patch> slots; rows with idx outside [0, dst_rows) are skipped. */
/* Alignment: src and dst 16 bytes. */
int vllm_scatter_rows_bf16(const uint16_t *src, const int64_t *idx, uint16_t *dst, long n, int C, long dst_rows,
                           vllm_stream_t stream);

/* The same splice with the index bookkeeping on the device (round 5): no host synchronisation, nothing copied twice.
 *   input_ids [B, L] (device int64), image_features [n_tiles, T, C] bf16 in tile order, tiles_per_sample: HOST int32 [B] ('anyres'
 *   list input; travels as a kernel argument) or NULL (one tile per sample), inputs_embeds [B, L, C] bf16, modified in place.
 * Replaces modeling_visionllmv2.py:582-605: `selected = input_ids == imp_token_id`, `has_image = selected.sum(-1) != 0` (expanded to
 * the tiles of a sample), `vit_embeds = image_features[has_image]`, `inputs_embeds[selected] = ... + vit_embeds`, and the rule of
 * :597-603 when the counts differ: slots a whole multiple of the tokens -> the tokens repeat; any other mismatch is the reference's
 * second failing assignment: NOTHING is written and status[2] = 1.
 * workspace: device int32 [vllm_splice_workspace_ints(B, L, n_tiles)]; its first four words are {rows moved, visual tokens offered
 * (tiles of samples with an image x T), error, <im_patch> slots}; status: device int32 [4] or NULL -> {slots, tokens offered, error,
 * tiles kept}. */
long vllm_splice_workspace_ints(int B, int L, int n_tiles);
/* Alignment: image_features and inputs_embeds 16 bytes. */
int vllm_splice_visual_tokens_bf16(const int64_t *input_ids, long imp_token_id, const uint16_t *image_features,
                                   const int32_t *tiles_per_sample, int B, int L, int n_tiles, int T, int C,
                                   uint16_t *inputs_embeds, int32_t *workspace, int32_t *status, vllm_stream_t stream);
/* Backward of that splice.  Replaces: the autograd of modeling_visionllmv2.py:582-605 (`inputs_embeds[selected] * 0.0 + vit_embeds`,
 * the index assignment, `image_features[has_image]`, the repeat of :597-603) -- several full [B L, C] passes and two host
 * synchronisations there, one pass over grad_out here.
 *   workspace: the forward call's, exactly as it left it (slot list, kept tiles, header): no second scan of input_ids, no host read,
 *   no allocation.  grad_out [B, L, C]: gradient of the spliced embeddings.  B, L, n_tiles, T, C: the forward's.
 *   grad_inputs_embeds [B, L, C]    = grad_out with the rows the forward overwrote set to zero;
 *   grad_image_features [n_tiles, T, C]: visual token j of the kept tiles (tile kept[j / T], token j % T) gets the sum of
 *     grad_out[slots[r]] over r = j, j + n_vit, ... below the rows moved -- one term when the counts were equal (a pure move), k terms
 *     under the repeat rule, added in fp32 in ascending r and rounded to bf16 once; tiles of samples without an image get zero rows.
 * A forward that wrote nothing (error flag set) gives grad_inputs_embeds = grad_out and grad_image_features = 0.
 * Either output may be NULL (not needed: its rows cost no traffic).  An output that is passed is written completely by the call (no
 * zero-fill by the caller, no atomics, the same bits on every run); every grad_out row is read once.  A refused call (VLLM_EINVAL)
 * writes nothing; B L == 0 and n_tiles T == 0 are accepted.
 * NON-FINITE grad_out AT A SLOT ROW: grad_inputs_embeds gets 0 there, the derivative of a row that was overwritten; the reference's
 * autograd gives NaN (0.0 * inf in the backward of `* 0.0`).  Deliberate departure. */
/* Alignment: grad_out, grad_inputs_embeds and grad_image_features 16 bytes. */
int vllm_splice_visual_tokens_backward_bf16(const int32_t *workspace, const uint16_t *grad_out, int B, int L, int n_tiles, int T, int C,
                                            uint16_t *grad_inputs_embeds, uint16_t *grad_image_features, vllm_stream_t stream);

/* The per-sample token loops around the LLM (modeling_visionllmv2.py:440-527 [EMB] splice, :609-715 region features and
 * <region> slots, :775-787 [EMB] hidden states -> text_query) as index bookkeeping + ONE row mover:
 * dst[dst_idx[i], :] = src[src_idx[i], :] for i < n (device int64 indices; NULL = the identity; rows whose index falls
 * outside [0, src_rows) / [0, dst_rows) are skipped).  Rows are C bf16, C % 8 == 0. */
/* Alignment: src and dst 16 bytes. */
int vllm_copy_rows_bf16(const uint16_t *src, const int64_t *src_idx, uint16_t *dst, const int64_t *dst_idx, long n,
                        int C, long src_rows, long dst_rows, vllm_stream_t stream);

/* Backward of those four loops: two row kernels, driven by index arrays the forward built on the device.
 *
 * Segment sum: dst[d, :] = bf16( sum_{k = seg_ptr[d]}^{seg_ptr[d+1]-1} float(src[src_idx[k], :]) ) for d < dst_rows.
 * Replaces the autograd of: the sequential `torch.cat([..., emb_embeddings_*, ...])` of modeling_visionllmv2.py:432-527 (gradient of the
 * query tables: a table row sums grad_out over the positions it was written to), `hidden_states[b, selected]` of :775-787 (gradient of
 * the LLM hidden states: segments of 0 or 1 term) and the per-region tile selection of :644-681 (gradient of the tower's last three
 * levels: a tile row sums grad_out over the regions that read it).
 *   src [src_rows, C] bf16, seg_ptr [dst_rows + 1] and src_idx [n_idx]: DEVICE int64, dst [dst_rows, C] bf16; C % 8 == 0.
 *   Terms are added in fp32 in ascending k and rounded to bf16 once.  An empty segment gives a zero row; a segment of one term is a
 *   bit-exact copy for every finite or infinite value (-0.0 included).  Every dst row is written by the call: no zero-fill by the
 *   caller, no atomics, the same bits on every run.  src is never written.
 *   Each segment is clamped to [0, n_idx] before it is walked; a pair with seg_ptr[d+1] < seg_ptr[d] is an empty segment; a term whose
 *   src_idx[k] lies outside [0, src_rows) contributes nothing (the row mover's "skipped" rule): no content of the index arrays can make
 *   the kernel read or write outside the four buffers.
 *   Refused (VLLM_EINVAL, nothing written, decided before any launch): C <= 0 or C % 8 != 0; a negative size; src or dst off 16 bytes; a
 *   NULL seg_ptr or dst with dst_rows > 0; a NULL src or src_idx with n_idx > 0.  dst_rows == 0 is accepted without a launch; n_idx == 0
 *   with src == NULL is accepted and every row becomes zero. */
/* Alignment: src and dst 16 bytes. */
int vllm_rows_segment_sum_bf16(const uint16_t *src, long src_rows, const int64_t *seg_ptr, const int64_t *src_idx, long n_idx,
                               uint16_t *dst, long dst_rows, int C, vllm_stream_t stream);

/* Masked copy: dst[r, :] = zero_row[r] ? 0 : src[r, :] for r < rows.  Replaces the autograd of the index assignments
 * `inputs_embeds[selected] = region_features` (modeling_visionllmv2.py:688-698) and of the rows the [EMB] splice replaces (:432-527):
 * the gradient of inputs_embeds is grad_out with the overwritten rows set to zero.
 *   src, dst [rows, C] bf16, C % 8 == 0; zero_row [rows]: DEVICE uint8.  A row whose flag is non-zero is stored as zeros and its src
 *   row is NOT read (no read traffic), so non-finite values there do not propagate -- the same deliberate departure as
 *   vllm_splice_visual_tokens_backward_bf16.  Kept rows are bit-exact copies.
 *   Refused (VLLM_EINVAL, nothing written, decided before any launch): C <= 0 or C % 8 != 0; rows < 0; src or dst off 16 bytes; a NULL
 *   pointer with rows > 0.  rows == 0 is accepted without a launch. */
/* Alignment: src and dst 16 bytes. */
int vllm_copy_rows_masked_bf16(const uint16_t *src, const uint8_t *zero_row, uint16_t *dst, long rows, int C, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * B1. Vision encoder (the `vis_encoder` slot): one call runs patch-embed + all layers.
 *
 * Replaces InternVisionModel.forward (modeling_intern_vit.py:305-343: embeddings :82-90, encoder loop
 * :253-270, layer :198-210) and transformers.CLIPVisionModel.forward (call sites
 * visionllmv2/model/modeling_visionllmv2.py:135, 565-568).
 * ------------------------------------------------------------------------------------------------ */
#define VLLM_ARCH_INTERNVIT 0
#define VLLM_ARCH_CLIP 1

typedef struct VllmVitLayer {
    const uint16_t *norm1_w, *norm1_b;   /* RMSNorm weight (InternViT, b NULL) / LayerNorm weight+bias (CLIP) */
    const uint16_t *qkv_w, *qkv_b;       /* [3C, C] fused (CLIP: q,k,v projections concatenated), bias may be NULL */
    const uint16_t *q_norm_w, *k_norm_w; /* QK-RMSNorm weights [C] or NULL */
    const uint16_t *proj_w, *proj_b;     /* [C, C], [C] */
    const uint16_t *ls1;                 /* LayerScale [C] or NULL */
    const uint16_t *norm2_w, *norm2_b;
    const uint16_t *fc1_w, *fc1_b;       /* [I, C], [I] */
    const uint16_t *fc2_w, *fc2_b;       /* [C, I], [C] */
    const uint16_t *ls2;
    /* Optional (all NULL = launch the norms): the norms folded into the GEMMs around them (vllm_gemm_bf16_ln; taken for
     * hidden == 1024 and >= 1024 tokens).  *_w_ln = the weight with the norm's gamma multiplied in, bf16, same shape;
     * *_colsum[n] = sum_k w_ln[n, k], fp32 (LayerNorm; NULL for RMSNorm); *_bias_ln[n] = b_n + sum_k beta_k w[n, k], fp32
     * (NULL = 0).  Prepared once per weight set by the caller (the Python mirrors do it when they pack the parameters). */
    const uint16_t *qkv_w_ln;
    const float *qkv_colsum, *qkv_bias_ln;
    const uint16_t *fc1_w_ln;
    const float *fc1_colsum, *fc1_bias_ln;
} VllmVitLayer;

typedef struct VllmVitDesc {
    int arch;            /* VLLM_ARCH_* */
    int num_layers;      /* layers to run (<= model depth; hidden_states has num_layers+1 entries) */
    int hidden;          /* C */
    int heads;           /* H (C/H in {64,128}) */
    int inter;           /* I */
    int patch;           /* 14 */
    int image;           /* 336 / 448 */
    int kpad;            /* padded K of the patch-embedding GEMM (multiple of 64, >= 3*patch^2) */
    int act;             /* VLLM_EPI_GELU or VLLM_EPI_QUICK_GELU */
    int pixel_is_f32;    /* pixel_values dtype: 0 bf16, 1 fp32 */
    float eps;
    const uint16_t *patch_w;   /* [C, kpad] (Conv2d weight flattened, zero padded) */
    const uint16_t *patch_b;   /* [C] or NULL (CLIP) */
    const uint16_t *cls;       /* [C] */
    const uint16_t *pos;       /* [1+P, C] */
    const uint16_t *pre_ln_w, *pre_ln_b;  /* CLIP pre_layrnorm or NULL */
    const VllmVitLayer *layers;           /* HOST array [num_layers] of device pointers */
} VllmVitDesc;

int vllm_vit_desc_sizeof(void);   /* sizeof(VllmVitDesc): lets the ctypes mirror verify its layout */
int vllm_vit_layer_sizeof(void);
/* Workspace bytes needed by vllm_vit_forward for n_tiles tiles. */
long vllm_vit_workspace_bytes(const VllmVitDesc *desc, int n_tiles);
/* pixels [n_tiles,3,image,image]; hidden_states: HOST array of num_layers+1 DEVICE pointers, each
 * [n_tiles, 1+P, C] bf16 contiguous (entry i = input of layer i, last = final output, exactly the tuple
 * InternVisionEncoder returns with output_hidden_states=True).  Entries may be NULL except the last: the
 * library then keeps that state in its workspace (nobody reads it). */
/* Alignment: every parameter of the descriptor and every hidden-state pointer 16 bytes (GEMM / norm operands); workspace 16
 * bytes.  pixels: element alignment only. */
int vllm_vit_forward(const VllmVitDesc *desc, const void *pixels, int n_tiles,
                     uint16_t *const *hidden_states, void *workspace, long workspace_bytes,
                     vllm_stream_t stream);
/* Cumulative number of GEMM launches of vllm_vit_forward that ran with a norm folded in (test hook: proves which path ran). */
long vllm_vit_folded_gemm_launches(void);

/* ------------------------------------------------------------------------------------------------
 * B2. Projector ("vl_bridge") with the hidden-state select / CLS drop / pixel-shuffle in front of it
 * (modeling_visionllmv2.py:569-579, 162-182, 381-392).
 * ------------------------------------------------------------------------------------------------ */
#define VLLM_BRIDGE_LINEAR 0        /* nn.Linear */
#define VLLM_BRIDGE_MLP_GELU 1      /* mlp{N}x_gelu: Linear (GELU Linear)*(depth-1) */
#define VLLM_BRIDGE_INTERNVL_MLP 2  /* LayerNorm, Linear, GELU, Linear */

typedef struct VllmBridgeDesc {
    int kind;             /* VLLM_BRIDGE_* */
    int depth;            /* number of Linear layers (1 for linear, N for mlpNx_gelu, 2 for internvl_mlp) */
    int in_features;      /* C or 4C */
    int out_features;     /* LLM hidden size */
    int pixel_shuffle;    /* 1: apply pixel_shuffle(0.5) to the token grid first */
    int skip_cls;         /* 1: `hidden` is [n, 1+T, C] and row 0 of every tile (CLS) is skipped (:571); 0: [n, T, C] */
    float ln_eps;
    const uint16_t *ln_w, *ln_b;     /* internvl_mlp LayerNorm or NULL */
    const uint16_t *w[4], *b[4];     /* Linear weights [out,in] / biases */
} VllmBridgeDesc;

int vllm_bridge_desc_sizeof(void);
long vllm_bridge_workspace_bytes(const VllmBridgeDesc *desc, int n_tiles, int tokens_per_tile_in);
/* hidden: the selected hidden state [n_tiles, skip_cls+T, C] bf16; out
 * [n_tiles, T or T/4, out_features] bf16 -- row-major [tile, token, C_llm], the layout the token splice
 * (modeling_visionllmv2.py:582-605) consumes. */
/* Alignment: hidden, out, the LayerNorm and Linear parameters and the workspace 16 bytes. */
int vllm_bridge_forward(const VllmBridgeDesc *desc, const uint16_t *hidden, int n_tiles, int T, int C,
                        uint16_t *out, void *workspace, long workspace_bytes, vllm_stream_t stream);

/* Training the projector (the reference trains it: freeze_vl_bridge=False, visionllmv2/train/train.py:162-170; modeling_visionllmv2.py:579
 * calls it with grad on a frozen input).  Both calls take the projector's input as forward(x) receives it: the descriptor must have
 * pixel_shuffle = skip_cls = 0 (VLLM_EINVAL and a message otherwise).  x [rows, in_features], out [rows, out_features] bf16.
 * Training forward: the GEMMs of vllm_bridge_forward (same schedules, same bits: out is identical to what vllm_bridge_forward writes for
 * the same rows) and it keeps what the backward needs: for Linear i < depth - 1 its output before the GELU H_i (saved_pre[i]) and after
 * it A_i (saved_act[i]), [rows, out_features] each; internvl_mlp: the LayerNorm output (saved_ln [rows, in_features]; NULL otherwise).
 * Backward: grad_out [rows, out_features]; writes grad_w[i] (the Linear weights' shapes) for every Linear, grad_b[i] where it is not
 * NULL, grad_ln_w / grad_ln_b (internvl_mlp; either may be NULL), grad_x [rows, in_features] when not NULL.  All gradients bf16 (fp32
 * accumulation inside, fp32 LayerNorm input gradient), overwritten (the caller accumulates).  Run-to-run identical.
 * workspace: vllm_bridge_backward_workspace_bytes(desc, rows, need_grad_x) bytes for the backward; the same size (with need_grad_x 0)
 * also serves the training forward (which uses only the stream-K scratch at its head, present from 1024 rows on).  Where the query
 * answers 0 (a Linear projector below the split and stream-K sizes with grad_x NULL) a NULL workspace / 0 bytes is accepted; otherwise a
 * NULL, short or misaligned workspace is refused (VLLM_EINVAL) before anything is enqueued.  Nothing is allocated, nothing synchronised;
 * one stream. */
/* Alignment: x, out, grad_out, grad_x, every saved tensor and gradient, the descriptor's parameters and the workspace 16 bytes. */
long vllm_bridge_backward_workspace_bytes(const VllmBridgeDesc *desc, long rows, int need_grad_x);
int vllm_bridge_forward_train(const VllmBridgeDesc *desc, const uint16_t *x, long rows, uint16_t *out, uint16_t *const *saved_pre,
                              uint16_t *const *saved_act, uint16_t *saved_ln, void *workspace, long workspace_bytes, vllm_stream_t stream);
int vllm_bridge_backward(const VllmBridgeDesc *desc, const uint16_t *x, long rows, const uint16_t *grad_out,
                         const uint16_t *const *saved_pre, const uint16_t *const *saved_act, const uint16_t *saved_ln,
                         uint16_t *grad_x, uint16_t *const *grad_w, uint16_t *const *grad_b, uint16_t *grad_ln_w, uint16_t *grad_ln_b,
                         void *workspace, long workspace_bytes, vllm_stream_t stream);

/* Training one InternViT encoder layer (InternVisionEncoderLayer.forward, modeling_intern_vit.py:182-210: norm1 -> InternAttention
 * :93-164 -> ls1 + residual -> norm2 -> InternMLP :167-179 -> ls2 + residual; the encoder runs it under torch.utils.checkpoint,
 * :259-262, and the reference trains the tower with freeze_vis_encoder=False, visionllmv2/train/train.py:163, 534).  Dropout and
 * drop-path are 0.  x, out, grad_out, grad_x [B, S, hidden] bf16, contiguous.  hidden % 64 == 0 (<= 8192), inter % 64 == 0, head_dim
 * 64 or 128.  These structs are additions: VllmVitLayer / VllmVitDesc and vllm_abi_version are unchanged. */
typedef struct VllmVitLayerTrain {
    int hidden, heads, inter;
    float eps;
    const uint16_t *norm1_w;
    const uint16_t *qkv_w, *qkv_b;          /* [3C, C], [3C] or NULL */
    const uint16_t *q_norm_w, *k_norm_w;    /* [C] each, or both NULL (qk_normalization=False) */
    const uint16_t *proj_w, *proj_b, *ls1;
    const uint16_t *norm2_w;
    const uint16_t *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ls2;
} VllmVitLayerTrain;
/* What the training forward keeps for the backward (caller buffers, all written by the forward; M = B * S rows):
 *   qkv [M, 3C] the qkv Linear's output BEFORE the QK-norm;  ctx [M, C] attention output;  lse [B, heads, S] fp32;
 *   y1 [M, C] proj output before LayerScale;  x1 [M, C] the hidden state between the two blocks;  h1 / a1 [M, inter] fc1 output before /
 *   after the GELU;  y2 [M, C] fc2 output before LayerScale  -- (10 C + 4 inter) M bytes + lse.
 * Recomputed by the backward instead of saved, one norm launch each: norm1(x), norm2(x1), the post-norm q / k. */
typedef struct VllmVitLayerSaved {
    uint16_t *qkv, *ctx;
    float *lse;
    uint16_t *y1, *x1, *h1, *a1, *y2;
} VllmVitLayerSaved;
/* Parameter gradients (bf16, the parameters' shapes, overwritten -- the caller accumulates), in the layer's parameter order.  NULL =
 * not needed: that product is skipped, and everything only it needed (a frozen parameter costs no weight-gradient GEMM).  A bias
 * gradient comes out of its weight gradient's launch: it needs the weight's pointer too. */
typedef struct VllmVitLayerGrads {
    uint16_t *norm1_w, *qkv_w, *qkv_b, *q_norm_w, *k_norm_w, *proj_w, *proj_b, *ls1, *norm2_w, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ls2;
} VllmVitLayerGrads;
int vllm_vit_layer_train_sizeof(void);
int vllm_vit_layer_saved_sizeof(void);
int vllm_vit_layer_grads_sizeof(void);
/* Training forward: the statement order of vllm_vit_forward where it does not fold norms (the same kernels; below 1024 rows `out` is
 * bit for bit the inference encoder's next hidden state; from 1024 rows on the two residual GEMMs run one workgroup per tile, where the
 * inference encoder may take the persistent schedule: the same value to within the last bf16 bit).  Backward: grad_out -> grad_x (NULL
 * allowed) and the gradients named in `grads`; fp32 accumulation, every gradient element rounded once, run-to-run identical.
 * workspace: vllm_vit_layer_backward_workspace_bytes(desc, B, S) bytes serve both calls (< 0 for a refused descriptor; host-only
 * arithmetic).  Nothing is allocated, nothing synchronised; one stream.  A refused call (VLLM_EINVAL) writes nothing. */
/* Alignment: x, out, grad_out, grad_x, every saved tensor and gradient, the descriptor's parameters and the workspace 16 bytes. */
long vllm_vit_layer_backward_workspace_bytes(const VllmVitLayerTrain *desc, int B, int S);
int vllm_vit_layer_forward_train(const VllmVitLayerTrain *desc, const uint16_t *x, int B, int S, uint16_t *out,
                                 const VllmVitLayerSaved *saved, void *workspace, long workspace_bytes, vllm_stream_t stream);
int vllm_vit_layer_backward(const VllmVitLayerTrain *desc, const uint16_t *x, int B, int S, const uint16_t *grad_out,
                            const VllmVitLayerSaved *saved, uint16_t *grad_x, const VllmVitLayerGrads *grads, void *workspace,
                            long workspace_bytes, vllm_stream_t stream);
/* Building block of the training forward (tests; the LayerScale + residual statements modeling_intern_vit.py:206-208 behind proj :139 and
 * fc2 :178): vllm_gemm_bf16 with VLLM_EPI_RESIDUAL -- Y is bit for bit what that call stores with
 * VLLM_GEMM_FORCE_TILEWISE set (below the 8-phase kernel's size, simply what it stores) -- which also writes pre [M, N] (row stride ldy)
 * = bf16(x W^T + b), the output before LayerScale and residual.  `epilogue` = VLLM_EPI_RESIDUAL | VLLM_GEMM_FORCE_* bits. */
/* Alignment: X, W 16 bytes; Y, pre, res, bias, scale 8 bytes. */
int vllm_gemm_bf16_residual_save(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y, uint16_t *pre, int M, int N,
                                 int K, int ldx, int ldw, int ldy, int epilogue, const uint16_t *scale, const uint16_t *res, int ldr,
                                 vllm_stream_t stream);

/* Training one CLIP encoder layer (transformers 4.34 CLIPEncoderLayer.forward: layer_norm1 -> CLIPAttention (separate q / k / v
 * projections, here one fused [3C, C] weight; q * scale, softmax, out_proj) -> residual -> layer_norm2 -> CLIPMLP (fc1, quick-GELU or erf
 * GELU, fc2) -> residual; the reference builds CLIPVisionModel in the vis_encoder slot, visionllmv2/train/train.py:382-384, and offers
 * freeze_vis_encoder=False, :163, 534).  No dropout, no attention mask.  x, out, grad_out, grad_x [B, S, hidden] bf16, contiguous.
 * hidden % 64 == 0 (<= 8192), inter % 64 == 0, head_dim 64 or 128.  These structs are additions: VllmVitLayer / VllmVitDesc /
 * VllmVitLayerTrain and vllm_abi_version are unchanged. */
typedef struct VllmClipLayerTrain {
    int hidden, heads, inter;
    int act;                                /* VLLM_EPI_QUICK_GELU or VLLM_EPI_GELU */
    float eps;
    const uint16_t *norm1_w, *norm1_b;      /* layer_norm1 */
    const uint16_t *qkv_w, *qkv_b;          /* [3C, C], [3C]: q, k, v projections concatenated */
    const uint16_t *proj_w, *proj_b;        /* out_proj */
    const uint16_t *norm2_w, *norm2_b;      /* layer_norm2 */
    const uint16_t *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} VllmClipLayerTrain;
/* What the training forward keeps for the backward (caller buffers, all written by the forward; M = B * S rows):
 *   qkv [M, 3C];  ctx [M, C] attention output;  lse [B, heads, S] fp32;  x1 [M, C] the hidden state between the two blocks;  h1 / a1
 *   [M, inter] fc1 output before / after the activation  -- (5 C + 2 inter) M bf16 elements + lse (no LayerScale: no pre-scale outputs).
 * Recomputed by the backward instead of saved, one norm launch each: layer_norm1(x), layer_norm2(x1). */
typedef struct VllmClipLayerSaved {
    uint16_t *qkv, *ctx;
    float *lse;
    uint16_t *x1, *h1, *a1;
} VllmClipLayerSaved;
/* Parameter gradients (bf16, the parameters' shapes, overwritten -- the caller accumulates), in the layer's parameter order.  NULL = not
 * needed: that product is skipped, and everything only it needed.  A bias gradient of a Linear comes out of its weight gradient's launch:
 * it needs the weight's pointer too.  The k block of qkv_b, elements [C, 2C), is written as zero: the k projection's bias shifts every score of
 * a query row alike, which softmax does not see, so its gradient is identically zero (summing the computed dK would store rounding noise). */
typedef struct VllmClipLayerGrads {
    uint16_t *norm1_w, *norm1_b, *qkv_w, *qkv_b, *proj_w, *proj_b, *norm2_w, *norm2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} VllmClipLayerGrads;
int vllm_clip_layer_train_sizeof(void);
int vllm_clip_layer_saved_sizeof(void);
int vllm_clip_layer_grads_sizeof(void);
/* Training forward: the statement order of vllm_vit_forward where it does not fold norms, with the same kernels (where the inference
 * encoder launches its norms, `out` is bit for bit its next hidden state); fc1 runs the *_SAVE form of `act`, whose Y keeps the
 * inference bits.  Backward: grad_out -> grad_x (NULL allowed) and the gradients named in `grads`; fp32 accumulation, every gradient
 * element rounded once, run-to-run identical.  B * S == 0 zero-fills the gradients.
 * workspace: vllm_clip_layer_backward_workspace_bytes(desc, B, S) bytes serve both calls (< 0 for a refused descriptor; host-only
 * arithmetic).  Nothing is allocated, nothing synchronised; one stream.  A refused call (VLLM_EINVAL) writes nothing. */
/* Alignment: x, out, grad_out, grad_x, every saved tensor and gradient, the descriptor's parameters and the workspace 16 bytes. */
long vllm_clip_layer_backward_workspace_bytes(const VllmClipLayerTrain *desc, int B, int S);
int vllm_clip_layer_forward_train(const VllmClipLayerTrain *desc, const uint16_t *x, int B, int S, uint16_t *out,
                                  const VllmClipLayerSaved *saved, void *workspace, long workspace_bytes, vllm_stream_t stream);
int vllm_clip_layer_backward(const VllmClipLayerTrain *desc, const uint16_t *x, int B, int S, const uint16_t *grad_out,
                             const VllmClipLayerSaved *saved, uint16_t *grad_x, const VllmClipLayerGrads *grads, void *workspace,
                             long workspace_bytes, vllm_stream_t stream);
/* Building blocks of that layer's fc1 / fc2 (tests).  `force_bits` = VLLM_GEMM_FORCE_* bits only (no epilogue number).
 * quick_gelu_save: vllm_gemm_bf16 with VLLM_EPI_QUICK_GELU -- Y is bit for bit what that call stores (with VLLM_GEMM_FORCE_TILEWISE where
 *   the persistent schedule would take it) -- which also writes pre [M, N] (row stride ldy) = bf16(x W^T + b), the pre-activation.
 * quick_gelu_bwd: y = (x W^T) * q'(res[m, n]), q'(h) = s (1 + 1.702 h (1 - s)), s = sigmoid(1.702 h); `res` = the saved pre-activation
 *   [M, N] (row stride ldr); `bias` must be NULL (VLLM_EINVAL otherwise: dh1 = (g W2) q'(h1) has none). */
/* Alignment: X, W 16 bytes; Y, pre, res, bias 8 bytes. */
int vllm_gemm_bf16_quick_gelu_save(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y, uint16_t *pre, int M, int N,
                                   int K, int ldx, int ldw, int ldy, int force_bits, vllm_stream_t stream);
int vllm_gemm_bf16_quick_gelu_bwd(const uint16_t *X, const uint16_t *W, const uint16_t *bias, uint16_t *Y, int M, int N, int K, int ldx,
                                  int ldw, int ldy, int force_bits, const uint16_t *res, int ldr, vllm_stream_t stream);

/* Training the embeddings of the vision tower (InternVisionEmbeddings.forward, modeling_intern_vit.py:82-90; HF CLIPVisionEmbeddings
 * with patch_b = NULL): patch Conv2d (kernel = stride = patch) as im2col + GEMM, class embedding in row 0, + position table.  The
 * struct and the calls are additions: VllmVitDesc / VllmVitLayer and vllm_abi_version are unchanged.
 * Forward: the embedding step of vllm_vit_forward with the same kernels -- `out` is bit for bit hidden_states[0] of the InternViT
 * inference encoder for the same parameters and pixels.  The caller passes the Conv2d weight as the module stores it; the K-padded
 * copy the GEMM reads is built in the workspace on every call (nothing to go stale between optimizer steps).
 * Backward, with G = grad_out [n, 1+P, C] and col the im2col matrix of the forward ([n P, 3 patch^2], recomputed from `pixels`, not
 * kept by the forward):
 *     grad_pos[s, c]     = sum_n G[n, s, c]
 *     grad_cls[c]        = sum_n G[n, 0, c]                (the same fp32 sum in the same order: equals grad_pos[0] bit for bit)
 *     grad_patch_b[c]    = sum_n sum_{s >= 1} G[n, s, c]
 *     grad_patch_w[c, k] = sum_n sum_p G[n, 1+p, c] col[n P + p, k]
 * Every gradient is bf16 in the parameter's shape, accumulated in fp32 and rounded once, overwritten (the caller accumulates).  A NULL
 * gradient pointer skips that work and everything only it needed (no im2col and no weight-gradient GEMM without grad_patch_w; no
 * reduction pass when grad_patch_b, grad_cls and grad_pos are all NULL).  No atomics: run-to-run identical.  Pixel gradients are not
 * produced.  n_tiles == 0 zero-fills the requested gradients.  A refused call (VLLM_EINVAL, message in vllm_last_error) writes nothing.
 * workspace: vllm_vit_embed_workspace_bytes(desc, n_tiles) bytes serve both calls (< 0 for a refused descriptor; host-only
 * arithmetic).  Nothing is allocated, nothing synchronised; one stream. */
/* Alignment: out, grad_out, the parameters, the gradients and the workspace 16 bytes.  pixels: element alignment only. */
typedef struct VllmVitEmbed {
    int hidden;          /* C, % 64 == 0, <= 8192 */
    int patch, image;    /* image % patch == 0; P = (image/patch)^2 patches, S = 1 + P rows per tile */
    int pixel_is_f32;    /* 0 bf16, 1 fp32 */
    const uint16_t *patch_w;   /* the Conv2d weight as the module stores it: [C, 3*patch*patch] contiguous (no padding) */
    const uint16_t *patch_b;   /* [C] or NULL (CLIP's conv has no bias) */
    const uint16_t *cls;       /* [C] */
    const uint16_t *pos;       /* [1+P, C] */
} VllmVitEmbed;
int vllm_vit_embed_sizeof(void);
long vllm_vit_embed_workspace_bytes(const VllmVitEmbed *desc, int n_tiles);
int vllm_vit_embed_forward(const VllmVitEmbed *desc, const void *pixels, int n_tiles, uint16_t *out, void *workspace,
                           long workspace_bytes, vllm_stream_t stream);
int vllm_vit_embed_backward(const VllmVitEmbed *desc, const void *pixels, int n_tiles, const uint16_t *grad_out,
                            uint16_t *grad_patch_w, uint16_t *grad_patch_b, uint16_t *grad_cls, uint16_t *grad_pos, void *workspace,
                            long workspace_bytes, vllm_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Region encoder, native route (visionllmv2/model/region_encoder.py:68-147 with mask_pool_type = 'grid_sample', the configuration
 * modeling_visionllmv2.py:247-252 builds; trained by default, freeze_region_encoder=False).  One call forward, one backward, bf16,
 * channels-last throughout.  These structs and calls are additions: no existing struct is touched, vllm_abi_version is unchanged.
 *   forward:  im2col of images + masks (4 channels, kernel = stride = patch / 2) -> GEMM -> LayerNorm + GELU -> GEMM (the 2 x 2 / stride 2
 *     conv: its im2col is a reshape of the first conv's output, whose rows are ordered (n, y2, x2, dy, dx)) -> LayerNorm + GELU -> GEMM (the
 *     1 x 1 conv) = stem [n, h w, embed];  pooling weights w_k[n, pix] = (1 / L) sum_{l >= k} A_l[n, pix] / cnt_l from the sampling points
 *     of every level (A_l: the corner-weight sums of vllm_point_sample_mean_f32, bit for bit; a level whose region has no valid point adds
 *     0);  pooled[n, c] = sum_pix (w_0 stem + sum_k w_k level_k)[n, pix, c] in fp32, rounded once;  out = pooled up_w^T + up_b.
 *     The reference accumulates feat = feat + level and pools every prefix sum: level k is part of every pooled map l >= k, hence the
 *     suffix sum; its mean over the levels is inside the weights because up_dim is affine.  feat is never materialised.
 *   backward: grad_out [n, out_dim] -> the parameter gradients and grad_level_k = bf16(w_k (x) (grad_out up_w)) named in `grads` (NULL =
 *     not needed: that product is skipped and everything only it needed; a bias gradient comes out of its weight gradient's launch and
 *     needs the weight's pointer too).  The weights are recomputed from the points.  No gradient for images, masks or points.
 *     Every gradient is accumulated in fp32, rounded once, overwritten (the caller accumulates); no atomics on any output: run-to-run
 *     identical.
 * hidden / 4, hidden, embed, out_dim multiples of 64 (hidden <= 2048); patch even; H, W multiples of patch; h w = (H / patch)(W / patch)
 * <= 4096; 1 .. 4 levels, each [n, h w, embed] bf16 with its own row and image strides (elements, multiples of 8; 16-byte aligned);
 * points [levels, n, P, 2] fp32 (x, y) in [0, 1]^2 and valid [levels, n, P] uint8, as vllm_point_sample_mean_f32 takes them per level.
 * images [n, 3, H, W] and masks [n, 1, H, W] contiguous, bf16 or fp32 (pixel_is_f32), rounded to bf16 on the way in.
 * conv1_w [hidden/4, 4, k, k] (k = patch / 2), conv2_w [hidden, hidden/4, 2, 2], conv3_w [embed, hidden], up_w [out_dim, embed], as the
 * modules store them; the padded / permuted copies the GEMMs read are rebuilt in the workspace on every call. */
typedef struct VllmRegionEncoder {
    int hidden, embed, out_dim, patch;
    int n, H, W;                 /* regions; pixels per side */
    int levels, points;          /* L; P */
    int pixel_is_f32;            /* 0 bf16, 1 fp32 */
    float eps;                   /* LayerNorm2d: 1e-6 */
    int reserved0;
    const uint16_t *conv1_w, *conv1_b, *ln1_w, *ln1_b, *conv2_w, *conv2_b, *ln2_w, *ln2_b, *conv3_w, *conv3_b, *up_w, *up_b;
    const uint16_t *level[4];
    long level_row_stride[4], level_image_stride[4];
} VllmRegionEncoder;
/* What the forward keeps for the backward (caller buffers, all written by the forward; M1 = n (2H/patch)(2W/patch), M2 = M1 / 4 rows):
 *   a1 [M1, Kpad] the im2col matrix (Kpad = patch^2 rounded up to 64);  y1 / pre1 / g1 [M1, hidden/4] the first conv's output, its
 *   LayerNorm and the GELU of that;  y2 / pre2 / g2 [M2, hidden];  stem [M2, embed];  pooled [n, embed].  All bf16. */
typedef struct VllmRegionEncoderSaved {
    uint16_t *a1, *y1, *pre1, *g1, *y2, *pre2, *g2, *stem, *pooled;
} VllmRegionEncoderSaved;
typedef struct VllmRegionEncoderGrads {
    uint16_t *conv1_w, *conv1_b, *ln1_w, *ln1_b, *conv2_w, *conv2_b, *ln2_w, *ln2_b, *conv3_w, *conv3_b, *up_w, *up_b;
    uint16_t *level[4];          /* [n, h w, embed] contiguous */
} VllmRegionEncoderGrads;
int vllm_region_encoder_sizeof(void);
int vllm_region_encoder_saved_sizeof(void);
int vllm_region_encoder_grads_sizeof(void);
/* workspace: vllm_region_encoder_workspace_bytes(desc) bytes serve both calls (< 0 for a refused descriptor; host-only arithmetic; the
 * pointers of the descriptor are not read).  Its content is ignored and nothing is written beyond it; a short, misaligned or missing
 * workspace is refused before any launch.  Nothing is allocated, nothing synchronised; one stream.  n == 0: the forward does nothing,
 * the backward zero-fills the parameter gradients.  A refused call (VLLM_EINVAL, message in vllm_last_error) writes nothing. */
/* Alignment: the workspace, the parameters, the levels, every saved tensor, out, grad_out and every gradient 16 bytes; points 8 bytes;
 * images and masks element alignment. */
long vllm_region_encoder_workspace_bytes(const VllmRegionEncoder *desc);
int vllm_region_encoder_forward(const VllmRegionEncoder *desc, const void *images, const void *masks, const float *points,
                                const uint8_t *valid, uint16_t *out, const VllmRegionEncoderSaved *saved, void *workspace,
                                long workspace_bytes, vllm_stream_t stream);
int vllm_region_encoder_backward(const VllmRegionEncoder *desc, const float *points, const uint8_t *valid, const uint16_t *grad_out,
                                 const VllmRegionEncoderSaved *saved, const VllmRegionEncoderGrads *grads, void *workspace,
                                 long workspace_bytes, vllm_stream_t stream);
long vllm_region_encoder_calls(void);           /* forward + backward calls of this process that reached their launches (tests) */
long vllm_region_encoder_wgrad_launches(void);  /* weight-gradient GEMMs the backward calls of this process launched (tests) */
/* Its building blocks (tests, tools).
 * layernorm_gelu: pre = bf16(LayerNorm(x)), y = bf16(gelu_erf(pre)) -- the GELU of the ROUNDED value, which is what torch's bf16 modules
 *   compute and what the backward's gelu'(saved pre) differentiates; fp32 statistics.  x [rows, C] with row stride ldx, pre_out (NULL =
 *   not kept; y has the same bits either way) and y [rows, C] dense.  C a multiple of 64: 64 .. 512, or up to 4096 where C / 8 splits
 *   over 8 .. 64 lanes with at most 8 chunks each.  x, weight, bias, pre_out, y 16-byte aligned, ldx a multiple of 8.
 * region_im2col: A [n (2H/patch)(2W/patch), Kpad], rows (n, y2, x2, dy, dx), columns (c, ky, kx) with c = 3 the mask, pad columns zero.
 * region_pool_weights: weights [levels, n, h w] fp32.  region_pool: `levels` = n_levels device pointers in a HOST array, strides in
 *   elements.  region_outer: grad_map [n, hw, C] = bf16(weights[n, pix] g[n, c]). */
int vllm_layernorm_gelu_bf16(const uint16_t *x, int ldx, const uint16_t *weight, const uint16_t *bias, uint16_t *pre_out, uint16_t *y,
                             long rows, int C, float eps, vllm_stream_t stream);
int vllm_region_im2col_bf16(const void *images, const void *masks, int pixel_is_f32, uint16_t *A, int n, int H, int W, int patch, int Kpad,
                            vllm_stream_t stream);
int vllm_region_pool_weights_f32(const float *points, const uint8_t *valid, float *weights, int n, int levels, int h, int w, int P,
                                 vllm_stream_t stream);
int vllm_region_pool_bf16(const float *weights, const uint16_t *stem, const uint16_t *const *levels, const long *level_row_stride,
                          const long *level_image_stride, int n, int n_levels, int hw, int C, uint16_t *pooled, vllm_stream_t stream);
int vllm_region_outer_bf16(const float *weights, const uint16_t *g, uint16_t *grad_map, int n, int hw, int C, vllm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VLLM_HIP_H */
