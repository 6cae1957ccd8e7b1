"""One InternViT encoder layer, training step (forward + backward): the native path (vllm_vit_layer_forward_train /
vllm_vit_layer_backward behind InternVisionEncoderLayer.forward) against torch's own bf16 autograd of the reference's statements
(tests/vit_layer_train_inputs.py: ``layer``) on the same parameters -- with the reference's naive attention and with
F.scaled_dot_product_attention.  Device events, warm-up first, the paths alternated in one process.  Also the two new row-wise kernels
alone (fraction of the 6.29 TB/s copy rate the README uses) and the bytes a layer keeps between forward and backward.

    python tools/bench_vit_layer_train.py [--iters 10] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vit_layer_train_inputs as I  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd.intern_vit import InternVisionConfig, InternVisionEncoderLayer  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README
# (name, hidden, heads, inter, tiles, tokens, qk_normalization)
SHAPES = [("internvit_6b", 3200, 25, 12800, 40, 1025, True), ("internvit_300m", 1024, 16, 4096, 40, 577, False)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    L = _lib.lib()
    out = {}
    for name, C, H, inter, B, S, qkn in SHAPES:
        cfg = InternVisionConfig(hidden_size=C, num_attention_heads=H, intermediate_size=inter, num_hidden_layers=1, qk_normalization=qkn,
                                 layer_norm_eps=I.EPS)
        params = I.make_params(C, inter, qkn, False, seed=0, device=dev)
        layer = InternVisionEncoderLayer(cfg).to(dev).to(torch.bfloat16)
        layer.load_state_dict(params)
        x, g = I.make_io(B, S, C, seed=0, device=dev)
        x.requires_grad_(True)
        tp = {k: v.clone().requires_grad_(True) for k, v in params.items()}

        def native():
            layer.zero_grad(set_to_none=True)
            x.grad = None
            layer(x).backward(g)

        def native_fwd():
            with torch.no_grad():
                layer(x)

        def torch_with(attn):
            def run():
                for v in tp.values():
                    v.grad = None
                x.grad = None
                I.layer(tp, x, H, I.EPS, attn).backward(g)
            return run
        paths = {"native": native, "torch_naive_attn": torch_with(I.naive_attn), "torch_sdpa": torch_with(I.sdpa_attn), "native_forward_only": native_fwd}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        times = {k: [] for k in paths}
        for _ in range(3):   # alternated
            for k, fn in paths.items():
                times[k].append(timed(fn, args.iters))
        M = B * S
        rec = {"rows": M, "hidden": C, "heads": H, "inter": inter}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_torch_naive"] = round(min(times["native"]) / min(times["torch_naive_attn"]), 3)
        rec["native_over_torch_sdpa"] = round(min(times["native"]) / min(times["torch_sdpa"]), 3)
        rec["saved_bytes_per_layer"] = M * (10 * C + 4 * inter) + B * H * S * 4 + M * C * 2   # VllmVitLayerSaved + lse + the layer input
        # the two row-wise kernels alone, on tensors of this shape
        st = _lib.current_stream(torch.device(dev))
        a, b_, c_, w = I.norm_case(M, C, device=dev)
        gx, gw = torch.empty_like(a), torch.empty_like(w)
        wsb = L.vllm_rmsnorm_backward_workspace_bytes(M, C, 1)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def rms():
            _lib.check(L.vllm_rmsnorm_backward_bf16(P(a), C, P(b_), C, P(w), None, 1, I.EPS, M, C, P(gx), C, P(c_), C, P(gw), None, P(ws), wsb, st))

        def ls():
            _lib.check(L.vllm_layerscale_backward_bf16(P(a), C, P(b_), C, P(w), M, C, P(gx), C, P(gw), P(ws), wsb, st))
        for nm, fn, nbytes in (("rmsnorm_backward", rms, 4 * M * C * 2), ("layerscale_backward", ls, 3 * M * C * 2)):
            for _ in range(3):
                fn()
            us = min(timed(fn, args.iters) for _ in range(3))
            rec[nm] = {"us": round(us, 1), "bytes": nbytes, "frac_copy_rate": round(nbytes / (us * 1e-6) / COPY_RATE, 3)}
        out[name] = rec
        del layer, params, tp, x, g
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
