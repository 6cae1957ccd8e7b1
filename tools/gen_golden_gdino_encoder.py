#!/usr/bin/env python3
"""Generates tests/golden/gdino_encoder.npz by RUNNING THE REFERENCE's GroundingDinoEncoderLayer (twice, chained) in fp64 on the CPU.

    python tools/gen_golden_gdino_encoder.py <root of the VisionLLMv2 reference tree>

The classes and functions are taken out of visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py at run time (parsed and
exec'd with a handful of names; the file itself imports packages a test box does not have) -- nothing of the reference is copied into
the repository.  ``GroundingDinoEncoder`` derives from a transformers class, so its static ``get_reference_points`` (:1578-1606) is
taken out of the class body and run as a plain function, and its loop (:1681-1698) is the two calls below.
``disable_custom_kernels=True``: the pure-PyTorch operator runs.

Shape: B 2, d_model 64, encoder_attention_heads 4 (the enhancer and the fusion layer use 2), encoder_ffn_dim 512, levels [[6, 5], [3, 2]]
(36 tokens), 4 points, Lt 5 with two phrases per image (split behind token 2 in image 0, behind token 3 in image 1), position ids that
restart per phrase, a vision padding tail on image 1, the last text token of image 1 padded.  Parameters are the constructors' values
plus 0.2 randn (``vision_param`` / ``text_param`` from [0.5, 1.5]), rounded to bf16 and stored as fp32.  Stored: the state dict of the
two layers (``sd.layers.N.<name>``), the inputs, get_reference_points' output, the outputs after layer 1 and after layer 2.  Data only."""
import ast
import math
import os
import sys
import types
import warnings
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

REL = "visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py"
NAMES = ("multi_scale_deformable_attention", "GroundingDinoMultiscaleDeformableAttention", "GroundingDinoTextEnhancerLayer",
         "GroundingDinoBiMultiHeadAttention", "drop_path", "GroundingDinoDropPath", "GroundingDinoFusionLayer", "GroundingDinoDeformableLayer",
         "get_sine_pos_embed", "GroundingDinoEncoderLayer")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "gdino_encoder.npz")
B, LT, C, FFN, HEADS, POINTS = 2, 5, 64, 512, 4, 4
MAPS = [[6, 5], [3, 2]]
SPLITS = (2, 3)   # image b's first phrase is tokens [0, SPLITS[b])


def extract(path):
    glb = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor, "Optional": Optional, "Tuple": Tuple, "math": math, "warnings": warnings,
           "GroundingDinoConfig": object, "meshgrid": torch.meshgrid,
           "ACT2FN": {"relu": F.relu, "gelu": F.gelu}}
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in NAMES:
            node.decorator_list = []
            mod = ast.Module(body=[node], type_ignores=[])
            ast.fix_missing_locations(mod)
            exec(compile(mod, path, "exec"), glb)
        if isinstance(node, ast.ClassDef) and node.name == "GroundingDinoEncoder":
            fn = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "get_reference_points")
            fn.decorator_list = []
            mod = ast.Module(body=[fn], type_ignores=[])
            ast.fix_missing_locations(mod)
            exec(compile(mod, path, "exec"), glb)
    missing = [n for n in NAMES + ("get_reference_points",) if n not in glb]
    assert not missing, missing
    return glb


def main(root):
    glb = extract(os.path.join(root, REL))
    cfg = types.SimpleNamespace(d_model=C, encoder_ffn_dim=FFN, encoder_attention_heads=HEADS, fusion_dropout=0.0, fusion_droppath=0.1,
                                text_enhancer_dropout=0.0, activation_function="relu", num_feature_levels=len(MAPS), encoder_n_points=POINTS,
                                dropout=0.1, activation_dropout=0.0, disable_custom_kernels=True)
    torch.manual_seed(17)
    layers = nn.ModuleList([glb["GroundingDinoEncoderLayer"](cfg) for _ in range(2)]).double().eval()
    g = torch.Generator().manual_seed(170)
    with torch.no_grad():
        for p in layers.parameters():
            p.add_(0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64))
        for layer in layers:
            layer.fusion_layer.vision_param.copy_(0.5 + torch.rand(C, generator=g, dtype=torch.float64))
            layer.fusion_layer.text_param.copy_(0.5 + torch.rand(C, generator=g, dtype=torch.float64))
        for p in layers.parameters():   # bf16 VALUES held in fp64: a bf16 module holds the same numbers
            p.copy_(p.to(torch.bfloat16).double())
    S = sum(h * w for h, w in MAPS)
    rb = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g, dtype=torch.float64)).to(torch.bfloat16).double()
    vision, vision_pos, text = rb(B, S, C), rb(B, S, C, s=0.5), rb(B, LT, C)
    spatial_shapes = torch.tensor(MAPS, dtype=torch.int64)
    level_start_index = torch.cat((spatial_shapes.new_zeros(1), (spatial_shapes[:, 0] * spatial_shapes[:, 1]).cumsum(0)[:-1]))
    valid_ratios = (0.5 + 0.5 * torch.rand(B, len(MAPS), 2, generator=g)).float()
    valid_ratios[0, 0, 0] = 1.0
    vmask = torch.zeros(B, S, dtype=torch.bool)
    vmask[1, S - 7:] = True
    tmask = torch.zeros(B, LT, dtype=torch.bool)
    tmask[1, LT - 1] = True
    self_masks = torch.zeros(B, LT, LT, dtype=torch.bool)     # True = may attend
    ids = torch.zeros(B, LT, dtype=torch.int64)
    for b in range(B):
        for lo, hi in ((0, SPLITS[b]), (SPLITS[b], LT)):
            self_masks[b, lo:hi, lo:hi] = True
            ids[b, lo:hi] = torch.arange(hi - lo)
    with torch.no_grad():
        ref = glb["get_reference_points"](spatial_shapes, valid_ratios.double(), "cpu")
        outs, v, t = [], vision, text
        for layer in layers:
            (v, t), _ = layer(vision_features=v, vision_position_embedding=vision_pos, spatial_shapes=spatial_shapes,
                              level_start_index=level_start_index, key_padding_mask=vmask, reference_points=ref, text_features=t,
                              text_attention_mask=tmask, text_position_embedding=None, text_self_attention_masks=self_masks,
                              text_position_ids=ids)
            outs.append((v, t))
    data = {"sd.layers." + k: v.float().numpy() for k, v in layers.state_dict().items()}
    data.update(vision=vision.float().numpy(), vision_pos=vision_pos.float().numpy(), text=text.float().numpy(),
                spatial_shapes=spatial_shapes.numpy(), level_start_index=level_start_index.numpy(), valid_ratios=valid_ratios.numpy(),
                vision_attention_mask=vmask.numpy(), text_attention_mask=tmask.numpy(), text_self_attention_masks=self_masks.numpy(),
                text_position_ids=ids.numpy(), reference_points=ref.numpy(),
                out_vision_1=outs[0][0].numpy(), out_text_1=outs[0][1].numpy(), out_vision_2=outs[1][0].numpy(), out_text_2=outs[1][1].numpy(),
                config=np.array([C, FFN, HEADS, POINTS], dtype=np.int64))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["VISIONLLM_REFERENCE"])
