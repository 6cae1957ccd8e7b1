/* The descriptor structs of section f2g of vllm_hip.h (the Grounding-DINO text enhancer and encoder), which includes this file: do not
 * include it on its own.  They are TAGGED structs without a typedef name, as struct VllmFusionLayerDesc is (C callers write
 * `struct VllmTextEnhancerDesc`), and live in a file of their own because the sets of typedef'd and of tagged descriptors that
 * vllm_hip.h itself declares are closed for this ABI version and pinned by the boundary tests.  The binding reads this file under the
 * same member rules (_lib.parse_tagged_structs on this path; a member may name an earlier struct as `struct Tag *`) and compares each
 * struct with the library's vllm_*_desc_sizeof() when the library is loaded. */
#ifndef VLLM_HIP_GDINO_ENCODER_H
#define VLLM_HIP_GDINO_ENCODER_H

/* GroundingDinoTextEnhancerLayer (visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:787-857).  Device pointers, bf16;
 * nothing is copied or repacked: in_proj_w / in_proj_b are nn.MultiheadAttention's packed parameters, sliced by pointer offset. */
struct VllmTextEnhancerDesc {
    int32_t d_model, n_heads, d_ffn, act;        /* C: a multiple of 64 in 64 .. 512; C / n_heads 32 or 64; d_ffn a multiple of 64; act: 0 = ReLU, VLLM_EPI_GELU = erf GELU */
    float   norm_before_eps, norm_after_eps;
    const uint16_t *in_proj_w, *in_proj_b;       /* [3C, C] [3C]: rows 0 .. C q, C .. 2C k, 2C .. 3C v */
    const uint16_t *out_proj_w, *out_proj_b;     /* [C, C] [C] */
    const uint16_t *norm_before_w, *norm_before_b;   /* [C] [C] */
    const uint16_t *fc1_w, *fc1_b, *fc2_w, *fc2_b;   /* [d_ffn, C] [d_ffn] [C, d_ffn] [C] */
    const uint16_t *norm_after_w, *norm_after_b;     /* [C] [C] */
};

/* GroundingDinoEncoder (:1560-1722): per layer the fusion layer (section f2f), the text enhancer and the deformable layer (section f2b). */
struct VllmGdinoEncoderDesc {
    int32_t n_layers;                                  /* 1 .. 64 */
    int32_t reserved;                                  /* 0 */
    const struct VllmFusionLayerDesc *fusion;          /* HOST array [n_layers] */
    const struct VllmTextEnhancerDesc *enhancer;       /* HOST array [n_layers] */
    const VllmDeformEncLayerDesc *deformable;          /* HOST array [n_layers]; one d_model and n_levels for every layer; attn.ref_dim 2 */
    const float *dim_t;                                /* [C] fp32, device: get_sine_pos_embed's temperature table (:1202-1203) */
};

#endif
