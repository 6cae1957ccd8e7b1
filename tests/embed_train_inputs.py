"""Inputs, yardstick and bounds of the vision-tower embedding training tests (test_embed_train_cpu.py, test_embed_train_gpu.py).

A torch RESTATEMENT of InternVisionEmbeddings.forward (VisionLLMv2/visionllmv2/model/internvit/modeling_intern_vit.py:82-90), written
for any floating dtype: ``F.conv2d(stride = patch)``, ``flatten(2).transpose(1, 2)``, ``cat`` with the expanded class embedding,
``+ position_embedding``.  HF CLIPVisionEmbeddings is the same function without the conv bias.  It never calls the code under test.  The
fp64 yardstick runs on the CPU (the shapes are tiny, and it must not depend on the GPU convolution library having fp64).

Inputs: pixels randn (bf16; the fp32 case keeps the bf16-rounded values in fp32), grad_out randn / sqrt(C), conv weight randn / sqrt(K),
bias / class embedding / position table 0.1 randn -- all rounded to bf16.

Per-element bound, the project's form (``excess_ulp``): |err| <= 1 bf16 ulp(ref) + 2^-17 mag, mag = sum |terms| of each sum:
    grad_pos, grad_cls   sum_n |G|
    grad_patch_b         sum_{n, s >= 1} |G|
    grad_patch_w         |G|^T |col|
``emulate_*`` walk the kernels' arithmetic in fp32 on the CPU (the tile sums in tile order; the bias through the tile-sum kernel's block
partials: two positions per wave, four waves, blocks in order; the weight gradient as an fp32 product), one rounding to bf16 each:
test_embed_train_cpu.py keeps them inside the bounds at every case, so the bounds are ones a faithful implementation meets.
Nothing here touches torch.cuda at import."""
import math

import torch
import torch.nn.functional as F

from bounds import bf16_ulp, excess_ulp, rel_rms  # noqa: F401  (the project's bound, re-exported)

# (n, image, patch, C, bias, pixel dtype)
CASES = [(3, 70, 14, 128, True, torch.bfloat16),     # S = 26, ragged everywhere, 78 rows: less than one wgrad tile
         (2, 56, 14, 192, False, torch.bfloat16),    # CLIP form; C = 3 x 64
         (5, 224, 14, 256, True, torch.float32),     # 1285 rows over several M tiles: the split weight-gradient route
         (2, 64, 16, 64, True, torch.bfloat16),      # K = 768 = kpad: the no-padding edge
         (1, 28, 14, 3200, True, torch.bfloat16),    # the 6B width; 400 column chunks
         (40, 28, 14, 128, True, torch.bfloat16)]    # the workload's tile count in the reduction
SPLIT_CASE = 2
TS_ROWS = 8      # positions per block of the tile-sum kernel (embed_train.hip)


def kpad_for(patch):
    return (3 * patch * patch + 63) // 64 * 64


def embeddings(pix, w, b, cls, pos, patch):
    """:82-90.  w [C, 3, ps, ps], b [C] or None, cls [1, 1, C], pos [1, 1 + P, C]"""
    patch_embeds = F.conv2d(pix, w, b, stride=patch)
    patch_embeds = patch_embeds.flatten(2).transpose(1, 2)
    class_embeds = cls.expand(pix.shape[0], 1, -1)
    return torch.cat([class_embeds, patch_embeds], dim=1) + pos


def make_case(n, image, patch, C, bias, pix_dtype, seed=0, device="cpu"):
    """-> dict(pix, w, b, cls, pos, gout) on `device`; parameters and grad_out bf16, pixels `pix_dtype` holding bf16 values"""
    g = torch.Generator().manual_seed(5000 + seed + 7 * n + image + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    K, S = 3 * patch * patch, (image // patch) ** 2 + 1
    bf = lambda t: t.to(torch.bfloat16)
    c = dict(pix=bf(rn(n, 3, image, image)).to(pix_dtype), w=bf(rn(C, 3, patch, patch) / math.sqrt(K)), b=bf(0.1 * rn(C)) if bias else None,
             cls=bf(0.1 * rn(1, 1, C)), pos=bf(0.1 * rn(1, S, C)), gout=bf(rn(n, S, C) / math.sqrt(C)))
    return {k: (v.to(device) if v is not None else None) for k, v in c.items()}


def autograd_embeddings(c, patch, dtype, device="cpu"):
    """torch autograd of ``embeddings`` in ``dtype`` on copies of the values -> (out, dict(w, b, cls, pos) of gradients)"""
    p = {k: (c[k].detach().to(device=device, dtype=dtype).requires_grad_(True) if c[k] is not None else None) for k in ("w", "b", "cls", "pos")}
    out = embeddings(c["pix"].detach().to(device=device, dtype=dtype), p["w"], p["b"], p["cls"], p["pos"], patch)
    out.backward(c["gout"].to(device=device, dtype=dtype))
    return out.detach(), {k: (v.grad if v is not None else None) for k, v in p.items()}


def im2col(pix, patch):
    """[n, 3, image, image] -> [n, P, 3 ps^2] with k = c ps^2 + ky ps + kx (the Conv2d weight's flattening), p = py g + px"""
    return F.unfold(pix, kernel_size=patch, stride=patch).transpose(1, 2)


def reference(c, patch):
    """fp64 on the CPU -> (grads dict(w, b, cls, pos) in the parameters' shapes, mags dict) ; b entries None without a bias"""
    G = c["gout"].detach().cpu().double()
    col = im2col(c["pix"].detach().cpu().double(), patch)
    n, S, C = G.shape
    gpos, mpos = G.sum(0), G.abs().sum(0)
    gw = torch.einsum("npc,npk->ck", G[:, 1:], col)
    mw = torch.einsum("npc,npk->ck", G[:, 1:].abs(), col.abs())
    has_b = c["b"] is not None
    grads = dict(w=gw.view(C, 3, patch, patch), b=G[:, 1:].sum((0, 1)) if has_b else None, cls=gpos[0].view(1, 1, C), pos=gpos.view(1, S, C))
    mags = dict(w=mw.view(C, 3, patch, patch), b=G[:, 1:].abs().sum((0, 1)) if has_b else None, cls=mpos[0].view(1, 1, C), pos=mpos.view(1, S, C))
    return grads, mags


def emulate_tile_sums(gout):
    """the tile-sum kernel in fp32 -> (grad_pos [S, C] bf16, grad_cls [C] bf16, grad_patch_b [C] bf16)"""
    G = gout.detach().cpu().float()
    n, S, C = G.shape
    acc = torch.zeros(S, C)
    for t in range(n):          # tile order
        acc = acc + G[t]
    nb = (S + TS_ROWS - 1) // TS_ROWS
    bias = torch.zeros(C)
    for blk in range(nb):
        waves = []
        for w in range(4):
            b = torch.zeros(C)
            for s in range(blk * TS_ROWS + w, min((blk + 1) * TS_ROWS, S), 4):
                if s >= 1:
                    b = b + acc[s]
            waves.append(b)
        bias = bias + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return acc.to(torch.bfloat16), acc[0].to(torch.bfloat16), bias.to(torch.bfloat16)


def emulate_wgrad(gout, pix, patch):
    """fp32 products and sums of the bf16 operands, one rounding -> [C, 3 ps^2] bf16"""
    G = gout.detach().cpu().float()
    col = im2col(pix.detach().cpu().to(torch.bfloat16).float(), patch)
    n, S, C = G.shape
    return (G[:, 1:].reshape(-1, C).T @ col.reshape(-1, col.shape[-1])).to(torch.bfloat16)
