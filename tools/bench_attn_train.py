"""Attention training step at the tower's two shapes (B 40: S 577 / H 16 / D 64, ViT-L/14-336; S 1025 / H 25 / D 128, InternViT-6B):
the training forward (vllm_attn_fwd_train_qkvpacked_bf16) against the inference forward, the backward call alone
(vllm_attn_bwd_qkvpacked_bf16), and forward + backward through the FlashAttention hook; next to them torch's bf16 autograd of the
reference's _naive_attn statements (modeling_intern_vit.py:136-140) on the same tensors and F.scaled_dot_product_attention forward +
backward where this torch build has a fused backend for it.  Device events around >= 0.3 s of work per timing, warm-up first, the
paths alternated in one process, minimum over three rounds, the shader clock sampled meanwhile (bench.py's ClockSampler); fractions
of the nominal bf16 MFMA peak (2.5 PFLOP/s) from each kernel's own product count (forward 2 products = 4 B H S^2 D FLOPs, backward
7 products = 14 B H S^2 D: S and dP are computed in both backward kernels).

    python tools/bench_attn_train.py [--seconds 0.3] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import ClockSampler  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd.flash_attention import FlashAttention  # noqa: E402

PEAK = 2.5e15
SHAPES = [("vit_l_336", 40, 577, 16, 64), ("internvit_6b_448", 40, 1025, 25, 128)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.3, help="device time per timing")
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    P = _lib.ptr
    res = {}
    for name, B, S, H, D in SHAPES:
        torch.manual_seed(0)
        scale = D ** -0.5
        qkv = (torch.randn(B, S, 3, H, D, device=dev) * 0.5).to(torch.bfloat16)
        dout = torch.randn(B, S, H, D, device=dev).to(torch.bfloat16)
        out = torch.empty(B, S, H, D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, H, S, dtype=torch.float32, device=dev)
        g = torch.empty_like(qkv)
        need = L.vllm_attn_bwd_workspace_bytes(B, S, H, D)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        st = _lib.current_stream(dev)
        hook = FlashAttention()
        x = qkv.clone().requires_grad_(True)

        def f_inf():
            _lib.check(L.vllm_attn_fwd_qkvpacked_bf16(P(qkv), P(out), B, S, H, D, scale, st))

        def f_train():
            _lib.check(L.vllm_attn_fwd_train_qkvpacked_bf16(P(qkv), P(out), P(lse), B, S, H, D, scale, st))

        def f_bwd():
            _lib.check(L.vllm_attn_bwd_qkvpacked_bf16(P(qkv), P(out), P(lse), P(dout), B, S, H, D, scale, P(g), P(ws), need, st))

        def f_hook():
            x.grad = None
            hook(x)[0].backward(dout)

        def f_naive():
            x.grad = None
            q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
            attn = ((q * scale) @ k.transpose(-2, -1))
            attn = attn.softmax(dim=-1)
            (attn @ v).transpose(1, 2).backward(dout)

        def f_sdpa():
            x.grad = None
            q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
            F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).backward(dout)

        paths = {"fwd_inference": f_inf, "fwd_train": f_train, "bwd": f_bwd, "hook_fwd_bwd": f_hook, "torch_naive_bf16_fwd_bwd": f_naive}
        sdpa_note = None
        try:
            from torch.nn.attention import SDPBackend, sdpa_kernel
            with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):   # fused backends only
                f_sdpa()
            torch.cuda.synchronize()

            def f_sdpa_fused():
                with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):
                    f_sdpa()
            paths["torch_sdpa_fused_fwd_bwd"] = f_sdpa_fused
        except Exception as e:   # no fused backend in this build for this shape
            sdpa_note = f"no fused scaled_dot_product_attention backend in this torch build: {type(e).__name__}: {str(e)[:160]}"
        f_train()
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        iters = {k: max(3, int(args.seconds * 1e6 / timed(fn, 3)) + 1) for k, fn in paths.items()}
        t = {k: [] for k in paths}
        clk = ClockSampler(dev)
        sampled = clk.has_sysfs()
        if sampled:
            clk.start()
        for _ in range(3):   # alternated
            for k, fn in paths.items():
                t[k].append(timed(fn, iters[k]))
        clocks = clk.stop() if sampled else None
        unit = 2.0 * B * H * S * S * D    # one S x S x D product over the batch
        flops = {"fwd_inference": 2 * unit, "fwd_train": 2 * unit, "bwd": 7 * unit, "hook_fwd_bwd": 9 * unit}
        r = {"B": B, "S": S, "H": H, "D": D}
        for k in paths:
            us = min(t[k])
            r[k] = {"us": round(us, 1), "all_us": [round(v, 1) for v in t[k]], "iters": iters[k]}
            if k in flops:
                r[k]["frac_peak"] = round(flops[k] / (us * 1e-6) / PEAK, 3)
        if sdpa_note:
            r["torch_sdpa_fused_fwd_bwd"] = sdpa_note
        r["clocks"] = clocks if clocks else "no amdgpu hwmon files readable: clock not sampled"
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
