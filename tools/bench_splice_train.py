"""Visual-token splice under training (forward + backward) at bench.py's shape: 8 x 4096 positions x 4096 channels, 40 tiles x 576
tokens, split_sizes [5] * 8 (23040 of the 32768 rows are <im_patch> slots):
  (a) native: visionllm_amd.splice.splice_visual_tokens under autograd (in-place node, one native call each way; check=True, so
      the status read-back -- one host synchronisation -- is inside the timing, as in bench.py);
  (b) torch's autograd of the reference's statements (modeling_visionllmv2.py:582-605) in bf16 on the same tensors -- what the
      reference runs, independent of the code under test;
  (c) the native backward alone through the C ABI, as a share of the HBM copy rate: bytes from shapes (grad_out read once + the
      embedding gradient written + n_vit feature rows written) over the time, against the measured float4-copy rate of 6.29 TB/s.
Both (a) and (b) start from a non-leaf clone of the embeddings (the splice is in place) and end with backward() into the embedding
and feature leaves.  Device events around >= --seconds of work per timing after warm-up, the paths alternated in one process, three
rounds; the minimum and all rounds are printed.

    python tools/bench_splice_train.py [--seconds 0.5] [--backward-only]
"""
import argparse
import ctypes
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd.splice import splice_visual_tokens  # noqa: E402

HBM = 6.29e12          # measured float4 copy rate of the MI355X, bytes / s
IMP = 7
B, L, C, T, SPLIT = 8, 4096, 4096, 576, [5] * 8


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def composed(inputs_embeds, input_ids, image_features, split_sizes):
    """The reference's statements, re-typed."""
    inputs_embeds = inputs_embeds.reshape(B * L, C)
    selected = input_ids == IMP
    has_image = selected.sum(-1) != 0
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--backward-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L_ = _lib.lib()
    torch.manual_seed(0)
    n_tiles = sum(SPLIT)
    ids = torch.randint(10, 50, (B, L), device=dev)
    for b in range(B):
        ids[b, 17 * b + 3:17 * b + 3 + SPLIT[b] * T] = IMP
    emb = torch.randn(B, L, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    feats = torch.randn(n_tiles, T, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    g = torch.randn(B, L, C, device=dev).to(torch.bfloat16)
    n_vit = int((ids == IMP).sum())
    assert n_vit == n_tiles * T

    # (c): the workspace of one forward call, then the backward call alone
    ws = torch.empty(int(L_.vllm_splice_workspace_ints(B, L, n_tiles)), dtype=torch.int32, device=dev)
    tps = (ctypes.c_int32 * B)(*SPLIT)
    st = _lib.current_stream(dev)
    x = emb.detach().clone()
    _lib.check(L_.vllm_splice_visual_tokens_bf16(_lib.ptr(ids), IMP, _lib.ptr(feats), tps, B, L, n_tiles, T, C, _lib.ptr(x), _lib.ptr(ws),
                                                 None, st))
    ge, gf = torch.empty_like(g), torch.empty(n_tiles, T, C, dtype=torch.bfloat16, device=dev)

    def bwd_only():
        _lib.check(L_.vllm_splice_visual_tokens_backward_bf16(_lib.ptr(ws), _lib.ptr(g), B, L, n_tiles, T, C, _lib.ptr(ge), _lib.ptr(gf), st))

    def native():
        emb.grad = feats.grad = None
        splice_visual_tokens(emb.clone(), ids, IMP, feats, SPLIT).backward(g)

    def torch_ref():
        emb.grad = feats.grad = None
        composed(emb.clone(), ids, feats, SPLIT).backward(g)

    paths = {"native_backward_only": bwd_only}
    if not args.backward_only:
        paths["native_fwd_bwd"] = native
        paths["torch_autograd_fwd_bwd"] = torch_ref
        native()
        nat = (emb.grad.clone(), feats.grad.clone())
        torch_ref()
        assert torch.equal(nat[0], emb.grad) and torch.equal(nat[1], feats.grad), "native and torch gradients differ"
        bwd_only()
        assert torch.equal(ge, nat[0]) and torch.equal(gf, nat[1])
    iters = {}
    for k, f in paths.items():              # warm-up, and the iteration count that fills --seconds
        for _ in range(3):
            f()
        iters[k] = max(10, math.ceil(args.seconds * 1e6 / timed(f, 5)))
    rounds = {k: [] for k in paths}
    for _ in range(3):                      # alternated
        for k, f in paths.items():
            rounds[k].append(timed(f, iters[k]))
    out = {"lib": os.path.relpath(_lib.lib_path(), ROOT), "hbm_copy_bytes_per_s": HBM, "shape": {"B": B, "L": L, "C": C, "n_tiles": n_tiles, "T": T, "slots": n_vit}}
    for k, t in rounds.items():
        out[k] = {"us": round(min(t), 1), "all_us": [round(u, 1) for u in t], "iters": iters[k]}
    nbytes = (2 * B * L + n_vit) * C * 2    # grad_out read once (slot rows by the feature half, the others by the embedding half) + both outputs written
    out["native_backward_only"]["bytes"] = nbytes
    out["native_backward_only"]["us_at_the_copy_rate"] = round(nbytes / HBM * 1e6, 1)
    out["native_backward_only"]["share_of_hbm_copy_rate"] = round(nbytes / (min(rounds["native_backward_only"]) * 1e-6) / HBM, 3)
    if not args.backward_only:
        out["native_over_torch"] = round(min(rounds["native_fwd_bwd"]) / min(rounds["torch_autograd_fwd_bwd"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
