#!/usr/bin/env python3
"""Generates tests/golden/gdino_inputs.npz by RUNNING THE REFERENCE's encoder-input step in fp64 on the CPU.

    python tools/gen_golden_gdino_inputs.py <root of the VisionLLMv2 reference tree>

Taken out of visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py at run time (parsed and exec'd with a handful of
names; the file itself imports packages a test box does not have) -- nothing of the reference is copied into the repository:
``GroundingDinoSinePositionEmbedding`` (:529-564), the mask statement of ``GroundingDinoConvEncoder.forward`` (:502),
``OVGroundingDinoModel.get_valid_ratio`` (:2200-2209) and the statements of ``OVGroundingDinoModel.forward`` from
``vision_features_input = vision_features[1:]`` to ``valid_ratios = valid_ratios.float()`` (:2388-2439), run against a stub ``self``
whose ``input_proj_vision`` is torch's own Conv2d / GroupNorm modules.

Shape (tests/gdino_inputs_inputs.py): B 2, in_channels (64, 128), d_model 64, 4 levels (two extra); maps 7 x 5 and 4 x 3; pixel mask
29 x 19 with a ragged valid rectangle per image and one interior hole.  Stored: the state dict (``sd.<name>``), the maps, the mask, the
six outputs.  Data only."""
import ast
import math
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), os.path.join(HERE, "..", "tests")]
import gdino_inputs_inputs as I  # noqa: E402

REL = "visionllmv2/model/grounding_dino/modeling_ov_grounding_dino_mask_dn.py"
OUT = os.path.join(HERE, "..", "tests", "golden", "gdino_inputs.npz")
RETURNS = "source_flatten, mask_flatten, lvl_pos_embed_flatten, spatial_shapes, level_start_index, valid_ratios"


def run(nodes, path, glb):
    mod = ast.Module(body=nodes, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), glb)


def function_of(name, args, body, returns):
    """``def name(args): body; return returns`` as an ast node"""
    fn = ast.parse(f"def {name}({args}):\n    pass\n    return {returns}").body[0]
    fn.body[0:1] = body
    return fn


def extract(path):
    glb = {"torch": torch, "nn": nn, "math": math}
    tree = ast.parse(open(path).read())
    classes = {n.name: n for n in tree.body if isinstance(n, ast.ClassDef)}
    method = lambda cls, name: next(n for n in classes[cls].body if isinstance(n, ast.FunctionDef) and n.name == name)
    run([classes["GroundingDinoSinePositionEmbedding"]], path, glb)
    loop = next(n for n in method("GroundingDinoConvEncoder", "forward").body if isinstance(n, ast.For))
    run([function_of("downsample_mask", "pixel_mask, feature_map", [loop.body[0]], "mask")], path, glb)
    gvr = method("OVGroundingDinoModel", "get_valid_ratio")
    gvr.decorator_list = []
    run([gvr], path, glb)
    body = method("OVGroundingDinoModel", "forward").body
    text = [ast.unparse(s) for s in body]
    first = next(i for i, s in enumerate(text) if s.startswith("vision_features_input = vision_features[1:]"))
    last = next(i for i, s in enumerate(text) if s == "valid_ratios = valid_ratios.float()")
    run([function_of("inputs_step", "self, vision_features, position_embeddings_list, pixel_mask", body[first:last + 1], RETURNS)], path, glb)
    return glb


def main(root):
    glb = extract(os.path.join(root, REL))
    mirror = I.make_module()   # torch's Conv2d / GroupNorm modules and level_embed with the test's parameter values; its forward is not run
    cfg = I.config(embedding_init_target=False, two_stage=False)
    pe = glb["GroundingDinoSinePositionEmbedding"](cfg.d_model // 2, cfg.positional_embedding_temperature, normalize=True)
    stub = types.SimpleNamespace(config=cfg, input_proj_vision=mirror.input_proj_vision, level_embed=mirror.level_embed,
                                 backbone=types.SimpleNamespace(position_embedding=pe), query_position_embeddings=None)
    stub.get_valid_ratio = lambda mask: glb["get_valid_ratio"](stub, mask)
    maps, pixel_mask = I.make_maps(), I.pixel_mask()
    with torch.no_grad():
        # the backbone (:495-504) and GroundingDinoConvModel (:518-526); element 0 is the map the model drops (`[1:]`)
        features = [(None, None)] + [(m, glb["downsample_mask"](pixel_mask, m)) for m in maps]
        pos = [None] + [pe(m, mask).to(m.dtype) for m, mask in features[1:]]
        outs = glb["inputs_step"](stub, features, pos, pixel_mask)
    data = {"sd." + k: v.detach().float().numpy() for k, v in mirror.state_dict().items()}
    data.update({f"map{i}": m.float().numpy() for i, m in enumerate(maps)})
    data["pixel_mask"] = pixel_mask.numpy()
    for name, t in zip(RETURNS.split(", "), outs):
        data[name] = t.detach().numpy()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes", {k: (v.dtype.name, v.shape) for k, v in data.items() if not k.startswith("sd.")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["VISIONLLM_REFERENCE"])
