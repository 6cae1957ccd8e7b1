#!/usr/bin/env python3
"""Generates tests/golden/fusion_layer.npz by RUNNING THE REFERENCE's GroundingDinoFusionLayer in fp64 on the CPU.

    python tools/gen_golden_fusion.py <root of the VisionLLMv2 reference tree>

The three classes and ``drop_path`` are taken out of
visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py:860-1101 at run time (parsed and exec'd with {torch, nn, F,
Optional, Tuple}; the file itself imports packages a test box does not have) -- nothing of the reference is copied into the repository.
Shape: B 2, S 37, Lt 5, d_model 64, embed 256 over 2 heads, both masks; ``vision_param`` / ``text_param`` redrawn from [0.5, 1.5] (at the
constructor's 1e-4 the attention output would be invisible).  Stored: the state dict (``sd.<name>``), the inputs, both outputs.  Data only."""
import ast
import os
import sys
import types
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

REL = "visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py"
NAMES = ("GroundingDinoBiMultiHeadAttention", "drop_path", "GroundingDinoDropPath", "GroundingDinoFusionLayer")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "fusion_layer.npz")
B, S, LT, C, FFN, HEADS = 2, 37, 5, 64, 512, 4   # embed = FFN / 2 = 256, heads = HEADS / 2 = 2


def extract(path):
    glb = {"torch": torch, "nn": nn, "F": F, "Optional": Optional, "Tuple": Tuple}
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in NAMES:
            node.decorator_list = []
            mod = ast.Module(body=[node], type_ignores=[])
            ast.fix_missing_locations(mod)
            exec(compile(mod, path, "exec"), glb)
    missing = [n for n in NAMES if n not in glb]
    assert not missing, missing
    return glb


def main(root):
    glb = extract(os.path.join(root, REL))
    cfg = types.SimpleNamespace(d_model=C, encoder_ffn_dim=FFN, encoder_attention_heads=HEADS, fusion_dropout=0.0, fusion_droppath=0.1)
    torch.manual_seed(7)
    m = glb["GroundingDinoFusionLayer"](cfg).double().eval()
    g = torch.Generator().manual_seed(70)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
        m.vision_param.copy_(0.5 + torch.rand(C, generator=g, dtype=torch.float64))
        m.text_param.copy_(0.5 + torch.rand(C, generator=g, dtype=torch.float64))
        for p in m.parameters():   # bf16 VALUES held in fp64: a bf16 module holds the same numbers, and the file compresses
            p.copy_(p.to(torch.bfloat16).double())
    vision = torch.randn(B, S, C, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    text = torch.randn(B, LT, C, generator=g, dtype=torch.float64).to(torch.bfloat16).double()
    vmask = torch.zeros(B, S, dtype=torch.bool)
    vmask[1, 30:] = True
    vmask[0, 3] = True
    tmask = torch.zeros(B, LT, dtype=torch.bool)
    tmask[1, 3:] = True
    with torch.no_grad():
        (ov, _), (ot, _) = m(vision, text, vmask, tmask)
    data = {"sd." + k: v.numpy() for k, v in m.state_dict().items()}
    data.update(vision=vision.numpy(), text=text.numpy(), attention_mask_vision=vmask.numpy(), attention_mask_text=tmask.numpy(),
                out_vision=ov.numpy(), out_text=ot.numpy(),
                config=np.array([C, FFN, HEADS], dtype=np.int64))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["VISIONLLM_REFERENCE"])
