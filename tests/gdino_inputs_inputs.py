"""Inputs shared by the tests of the Grounding-DINO encoder inputs (test_gdino_inputs_cpu.py, test_gdino_inputs_gpu.py) and by
tools/gen_golden_gdino_inputs.py: the golden's shape, its pixel mask, a perturbed module, feature maps.  Everything is drawn in fp64 and
rounded to bf16 VALUES, so an fp64, an fp32 and a bf16 module hold the same numbers."""
import types

import torch

from visionllm_amd.gdino_inputs import GroundingDinoEncoderInputs

B, D_MODEL, IN_CHANNELS, N_LEVELS = 2, 64, (64, 128), 4
MAP_SIZES = ((7, 5), (4, 3))                       # the two backbone maps; the extra levels are 2 x 2 and 1 x 1
LEVEL_SIZES = ((7, 5), (4, 3), (2, 2), (1, 1))
MASK_SIZE = (29, 19)
# image b's valid rectangle [0, rows) x [0, cols), and the hole of image 0 (rows, cols): inside the rectangle, so the cumsums are no ramp
VALID = ((22, 13), (29, 9))
HOLE = ((8, 13), (4, 9))
TEMPERATURE = 20


def config(d_model=D_MODEL, n_levels=N_LEVELS, temperature=TEMPERATURE, **kw):
    return types.SimpleNamespace(**{**dict(d_model=d_model, num_feature_levels=n_levels, positional_embedding_temperature=temperature,
                                           position_embedding_type="sine"), **kw})


def pixel_mask(dtype=torch.int64):
    m = torch.zeros((B,) + MASK_SIZE, dtype=torch.int64)
    for b, (r, c) in enumerate(VALID):
        m[b, :r, :c] = 1
    m[0, HOLE[0][0]:HOLE[0][1], HOLE[1][0]:HOLE[1][1]] = 0
    return m.to(dtype)


def bf16_values(t):
    return t.to(torch.bfloat16).to(t.dtype)


def perturb_(module, seed):
    """the constructor's values + noise, as bf16 values: GroupNorm's weight around 1, every bias and level_embed away from 0"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name != "level_embed":
                p.add_(0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64).to(p.dtype))
            p.copy_(bf16_values(p))
    return module


def make_module(n_levels=N_LEVELS, in_channels=IN_CHANNELS, d_model=D_MODEL, seed=31, dtype=torch.float64):
    torch.manual_seed(seed)
    m = GroundingDinoEncoderInputs(config(d_model, n_levels), in_channels).to(dtype).eval()
    return perturb_(m, seed + 1)


def make_maps(sizes=MAP_SIZES, in_channels=IN_CHANNELS, batch=B, seed=33, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [bf16_values(torch.randn(batch, c, h, w, generator=g, dtype=torch.float64)).to(dtype) for c, (h, w) in zip(in_channels, sizes)]


def extra_sizes(last, n):
    out = []
    for _ in range(n):
        last = ((last[0] - 1) // 2 + 1, (last[1] - 1) // 2 + 1)
        out.append(last)
    return out
