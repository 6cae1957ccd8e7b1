/* The descriptor struct of section f2h of vllm_hip.h (the inputs of the Grounding-DINO encoder), which includes this file: do not include
 * it on its own.  A TAGGED struct without a typedef name, as the descriptors of vllm_hip_gdino_encoder.h are, in a file of its own for
 * the same reason: the sets of descriptors that vllm_hip.h and vllm_hip_gdino_encoder.h declare are closed for this ABI version and
 * pinned by the boundary tests.  The binding reads this file under the same member rules (_lib.parse_tagged_structs on this path) and
 * compares the struct with the library's vllm_gdino_inputs_desc_sizeof() when the library is loaded. */
#ifndef VLLM_HIP_GDINO_INPUTS_H
#define VLLM_HIP_GDINO_INPUTS_H

/* input_proj_vision, level_embed and the sine position embedding of OVGroundingDinoModel
 * (visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:2080-2111, :2164, :529-564).  Device pointers, bf16 unless said
 * otherwise.  Level l < n_maps is a 1 x 1 conv on backbone map l; level l >= n_maps a 3 x 3 / stride 2 / padding 1 conv on the last map
 * (l == n_maps) or on level l - 1's output.  Up to 8 levels. */
struct VllmGdinoInputsDesc {
    int32_t d_model, n_levels, n_maps, reserved;   /* C: a multiple of 64 in 64 .. 512; 1 <= n_maps <= n_levels <= 8; reserved 0 */
    int32_t c_in[8];                               /* input channels of level l's conv, a multiple of 64; an extra level's: c_in[n_maps - 1] for l == n_maps, else C */
    float   gn_eps[8];                             /* GroupNorm(32, C) eps of level l */
    const uint16_t *conv_w[8];                     /* l < n_maps: [C, c_in] (the [C, c_in, 1, 1] weight as stored); else [C, 3, 3, c_in]: the [C, c_in, 3, 3] weight PERMUTED to (ky, kx, c) */
    const uint16_t *conv_b[8];                     /* [C] */
    const uint16_t *gn_w[8], *gn_b[8];             /* [C] [C] */
    const uint16_t *level_embed;                   /* [n_levels, C] */
    const float *dim_t;                            /* [C / 2] fp32: GroundingDinoSinePositionEmbedding's temperature table (:556-557) */
};

#endif
