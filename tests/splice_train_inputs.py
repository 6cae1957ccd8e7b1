"""Inputs and the yardstick of the visual-token splice's training tests (test_splice_train_gpu.py).

``reference_splice`` re-types the reference's statements (modeling_visionllmv2.py:582-605) as a torch expression: ``has_image``
and its expansion to tiles, ``image_features[has_image]``, the ``try`` / ``except`` repeat branch and the masked assignment.
torch's own autograd of it -- on a non-leaf clone of the embeddings, in bf16 or fp64 -- is what the native backward is compared
with; it never calls the code under test."""
import torch

IMP = 7        # id of the <im_patch> token in these inputs (every other id is drawn from [10, 50))


def reference_splice(inputs_embeds, input_ids, image_features, split_sizes):
    B, L, C = inputs_embeds.shape
    inputs_embeds = inputs_embeds.reshape(B * L, C)
    selected = input_ids == IMP
    has_image = selected.sum(-1) != 0
    if split_sizes is not None:
        has_image = torch.cat([has_image[i][None].repeat(split_sizes[i]) for i in range(B)], dim=0)
    selected = selected.reshape(-1)
    try:
        vit_embeds = image_features[has_image].reshape(-1, C)
        inputs_embeds[selected] = inputs_embeds[selected] * 0.0 + vit_embeds
    except Exception:
        vit_embeds = image_features[has_image].reshape(-1, C)
        n_selected_token = selected.sum()
        n_vit_token = vit_embeds.shape[0]
        vit_embeds = vit_embeds.repeat(n_selected_token // n_vit_token, 1) if n_selected_token > n_vit_token \
            else vit_embeds[:n_vit_token]
        inputs_embeds[selected] = inputs_embeds[selected] * 0.0 + vit_embeds
    return inputs_embeds.reshape(B, L, C)


def reference_grads(emb, ids, feats, split, grad_out, dtype=torch.bfloat16, need=(True, True)):
    """-> (spliced, d/d emb, d/d feats) by torch's autograd of the reference's statements in ``dtype`` (None where not needed)."""
    e = emb.detach().to(dtype).clone().requires_grad_(need[0])
    f = feats.detach().to(dtype).clone().requires_grad_(need[1])
    out = reference_splice(e.clone(), ids, f, split)
    out.backward(grad_out.to(dtype))
    return out.detach(), e.grad, f.grad


def case(name, C, device, seed=0):
    """-> dict(ids [B, L], split, emb [B, L, C], feats [n_tiles, T, C], grad_out [B, L, C], dropped: tiles of samples without an
    image); bf16 tensors on ``device``."""
    g = torch.Generator().manual_seed(seed)
    dropped = []
    if name == "equal":                 # every sample has its image; sample 0's slots are every second position
        B, L, T, split = 3, 40, 6, [2, 1, 1]
        ids = torch.randint(10, 50, (B, L), generator=g)
        ids[0, 3:3 + 4 * T:2] = IMP
        ids[1, 20:20 + T] = IMP
        ids[2, L - T:] = IMP
    elif name == "anyres_dropped":      # sample 1 has tiles but no <im_patch>: its two tiles are dropped
        B, L, T, split = 4, 40, 6, [2, 2, 1, 3]
        ids = torch.randint(10, 50, (B, L), generator=g)
        ids[0, 3:3 + 2 * T] = IMP
        ids[2, 0:T] = IMP
        ids[3, 1:4] = IMP
        ids[3, 9:9 + 3 * T - 3] = IMP
        dropped = [2, 3]
    elif name == "one_tile_per_sample":  # tensor `images` input: split_sizes None; sample 1 has no image
        B, L, T, split = 3, 40, 6, None
        ids = torch.randint(10, 50, (B, L), generator=g)
        ids[0, 5:5 + T] = IMP
        ids[2, L - T:] = IMP
        dropped = [1]
    elif name == "no_slot":
        B, L, T, split = 3, 40, 6, [1, 2, 1]
        ids = torch.randint(10, 50, (B, L), generator=g)
        dropped = [0, 1, 2, 3]
    elif name == "bench":               # bench.py's splice: 8 x 4096 positions, 40 tiles x 576 tokens
        B, L, T, split = 8, 4096, 576, [5] * 8
        ids = torch.randint(10, 50, (B, L), generator=g)
        for b in range(B):
            ids[b, 17 * b + 3:17 * b + 3 + 5 * T] = IMP
    elif name in ("repeat2", "repeat3"):   # :597-603: the slots are 2 x / 3 x the tokens, so the tokens repeat
        k = int(name[-1])
        B, L, T, split = 2, 64, 6, [1, 1]
        ids = torch.randint(10, 50, (B, L), generator=g)
        ids[0, 1:1 + 2 * (5 * k + 2):2] = IMP           # 5 k + 2 slots, every second position
        ids[1, 30:30 + 7 * k - 2] = IMP                 # 7 k - 2 slots: 12 k in all for 12 tokens
    elif name == "mismatch":            # 13 slots for 6 tokens: the reference's second assignment fails, nothing is written
        B, L, T, split = 1, 40, 6, [1]
        ids = torch.randint(10, 50, (B, L), generator=g)
        ids[0, 2:2 + 2 * T + 1] = IMP
    else:
        raise KeyError(name)
    n_tiles = B if split is None else sum(split)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(torch.bfloat16).to(device)
    return dict(ids=ids.to(device), split=split, emb=rnd(B, L, C), feats=rnd(n_tiles, T, C), grad_out=rnd(B, L, C), dropped=dropped,
                B=B, L=L, T=T, C=C, n_tiles=n_tiles)
