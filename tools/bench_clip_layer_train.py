"""One CLIP encoder layer, training step (forward + backward): the native path (vllm_clip_layer_forward_train /
vllm_clip_layer_backward behind _CLIPEncoderLayer.forward) against torch's own bf16 autograd of HF's statements
(tests/clip_layer_train_inputs.py: ``layer``) on the same parameters -- with HF's bmm / softmax / bmm attention and with
F.scaled_dot_product_attention.  Device events, warm-up first, the paths alternated in one process, the shader clock sampled meanwhile
(bench.py's ClockSampler).  Also the new LayerNorm backward kernel alone (fraction of the 6.29 TB/s copy rate the README uses) and the
bytes a layer keeps between forward and backward.

    python tools/bench_clip_layer_train.py [--iters 10] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_layer_train_inputs as I  # noqa: E402
from bench import ClockSampler  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd.clip_vit import _CLIPEncoderLayer  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README
# (name, hidden, heads, inter, tiles, tokens, act): the bench workload's tower, 40 tiles of ViT-L/14-336
SHAPES = [("clip_vit_l", 1024, 16, 4096, 40, 577, "quick_gelu")]


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
    for name, C, H, inter, B, S, act in SHAPES:
        cfg = SimpleNamespace(hidden_size=C, num_attention_heads=H, intermediate_size=inter, num_hidden_layers=1, layer_norm_eps=I.EPS,
                              hidden_act=act)
        params = I.make_params(C, inter, seed=0, device=dev)
        layer = _CLIPEncoderLayer(cfg).to(dev).to(torch.bfloat16)
        layer.load_state_dict(params)
        x, g = I.make_io(B, S, C, seed=0, device=dev)
        x.requires_grad_(True)
        tp = {k: v.clone().requires_grad_(True) for k, v in params.items()}

        def native():
            layer.zero_grad(set_to_none=True)
            x.grad = None
            layer(x)[0].backward(g)

        def native_fwd():
            with torch.no_grad():
                layer(x)

        def torch_with(attn):
            def run():
                for v in tp.values():
                    v.grad = None
                x.grad = None
                I.layer(tp, x, H, act, I.EPS, attn).backward(g)
            return run
        paths = {"native": native, "torch_hf_attn": torch_with(I.clip_attention), "torch_sdpa": torch_with(I.sdpa_attention),
                 "native_forward_only": native_fwd}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        times = {k: [] for k in paths}
        clk = ClockSampler(dev)
        sampled = clk.has_sysfs()
        if sampled:
            clk.start()
        for _ in range(3):   # alternated
            for k, fn in paths.items():
                times[k].append(timed(fn, args.iters))
        clocks = clk.stop() if sampled else None
        M = B * S
        rec = {"rows": M, "hidden": C, "heads": H, "inter": inter, "act": act,
               "clocks": clocks if clocks else "no amdgpu hwmon files readable: clock not sampled"}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_torch_hf_attn"] = round(min(times["native"]) / min(times["torch_hf_attn"]), 3)
        rec["native_over_torch_sdpa"] = round(min(times["native"]) / min(times["torch_sdpa"]), 3)
        rec["saved_bytes_per_layer"] = M * (5 * C + 2 * inter) * 2 + B * H * S * 4 + M * C * 2   # VllmClipLayerSaved + lse + the layer input
        # the LayerNorm backward alone, on tensors of this shape: x, grad_y, grad_res read, grad_x written
        st = _lib.current_stream(torch.device(dev))
        a, b_, c_, w = I.norm_case(M, C, device=dev)
        gx, gw, gb = torch.empty_like(a), torch.empty_like(w), torch.empty_like(w)
        wsb = L.vllm_layernorm_backward_res_workspace_bytes(M, C)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def ln():
            _lib.check(L.vllm_layernorm_backward_res_bf16(P(a), C, P(b_), C, P(w), I.EPS, M, C, P(gx), C, P(c_), C, P(gw), P(gb), P(ws), wsb, st))
        for _ in range(3):
            ln()
        us = min(timed(ln, args.iters) for _ in range(3))
        nbytes = 4 * M * C * 2
        rec["layernorm_backward_res"] = {"us": round(us, 1), "bytes": nbytes, "frac_copy_rate": round(nbytes / (us * 1e-6) / COPY_RATE, 3)}
        out[name] = rec
        del layer, params, tp, x, g
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
