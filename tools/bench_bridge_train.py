"""Projector training step (forward + backward) at BASELINE's two projector shapes: the native path (vllm_bridge_forward_train /
vllm_bridge_backward behind forward(x)) against torch's own bf16 autograd of the SAME module object (nn.Sequential.forward, whose
Linears run on hipBLASLt).  Device events, warm-up first, the two paths alternated in one process; per-GEMM times of the native
backward from the wgrad / GEMM entry points on the same operands; fractions of the nominal bf16 MFMA peak (2.5 PFLOP/s).

    python tools/bench_bridge_train.py [--iters 20] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd.bridge import build_vl_bridge  # noqa: E402

PEAK = 2.5e15
SHAPES = [("vit_l", "mlp2x_gelu", 1024, 4096, 40 * 576), ("internvit_6b", "internvl_mlp", 12800, 4096, 40 * 256)]


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    L = _lib.lib()
    out = {}
    for name, kind, cin, cout, rows in SHAPES:
        torch.manual_seed(0)
        br = build_vl_bridge(kind, cin, cout).to(dev).to(torch.bfloat16)
        x = torch.randn(rows, cin, device=dev).to(torch.bfloat16)
        g = (torch.randn(rows, cout, device=dev) / 64).to(torch.bfloat16)
        plain = nn.Sequential.forward

        def native():
            br.zero_grad(set_to_none=True)
            br(x).backward(g)

        def torch_ref():
            br.zero_grad(set_to_none=True)
            plain(br, x).backward(g)
        for _ in range(args.warmup):
            native()
            torch_ref()
        t_nat, t_ref = [], []
        for _ in range(3):   # alternated
            t_nat.append(timed(native, args.iters))
            t_ref.append(timed(torch_ref, args.iters))
        # FLOPs of forward + backward: forward GEMMs, weight gradients, input gradients of the Linears behind the first (and of the
        # first one for internvl_mlp, whose LayerNorm parameters need it)
        lin = [m for m in br if isinstance(m, nn.Linear)]
        f = sum(2.0 * rows * m.in_features * m.out_features for m in lin) * 2 + \
            sum(2.0 * rows * m.in_features * m.out_features for m in lin[1:]) + \
            (2.0 * rows * lin[0].in_features * lin[0].out_features if kind == "internvl_mlp" else 0.0)
        # per GEMM of the native backward, on the operands it uses
        per = {}
        for i, m in enumerate(lin):
            K, N = m.in_features, m.out_features
            A = torch.randn(rows, K, device=dev).to(torch.bfloat16)
            dw = torch.empty(N, K, device=dev, dtype=torch.bfloat16)
            db = torch.empty(N, device=dev, dtype=torch.bfloat16)
            wsb = L.vllm_gemm_wgrad_workspace_bytes(rows, N, K)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
            st = _lib.current_stream(torch.device(dev))

            def wg():
                _lib.check(L.vllm_gemm_wgrad_bf16(ctypes.c_void_p(g.data_ptr()), N, ctypes.c_void_p(A.data_ptr()), K, rows, N, K,
                                                  ctypes.c_void_p(dw.data_ptr()), K, ctypes.c_void_p(db.data_ptr()),
                                                  ctypes.c_void_p(ws.data_ptr()), wsb, st))
            for _ in range(3):
                wg()
            us = min(timed(wg, args.iters) for _ in range(3))
            per[f"wgrad_{i} {N}x{K} M={rows}"] = {"us": round(us, 1), "frac_peak": round(2.0 * rows * N * K / (us * 1e-6) / PEAK, 3)}
            if i > 0 or kind == "internvl_mlp":
                Wt = m.weight.detach().t().contiguous()
                y = torch.empty(rows, K, device=dev, dtype=torch.bfloat16)
                res = torch.randn(rows, K, device=dev).to(torch.bfloat16)
                epi = 6 if i > 0 else 0

                def dg():
                    _lib.check(L.vllm_gemm_bf16(ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(Wt.data_ptr()), None,
                                                ctypes.c_void_p(y.data_ptr()), rows, K, N, N, N, K, epi, None,
                                                ctypes.c_void_p(res.data_ptr()) if epi == 6 else None, K, 0, st))
                for _ in range(3):
                    dg()
                us = min(timed(dg, args.iters) for _ in range(3))
                per[f"dgrad_{i} {'GELU_BWD' if epi == 6 else 'plain'} {rows}x{K}x{N}"] = {
                    "us": round(us, 1), "frac_peak": round(2.0 * rows * N * K / (us * 1e-6) / PEAK, 3)}
        out[name] = {"kind": kind, "rows": rows, "native_fwd_bwd_us": round(min(t_nat), 1), "torch_bf16_autograd_us": round(min(t_ref), 1),
                     "native_frac_peak": round(f / (min(t_nat) * 1e-6) / PEAK, 3), "torch_frac_peak": round(f / (min(t_ref) * 1e-6) / PEAK, 3),
                     "all_native_us": [round(t, 1) for t in t_nat], "all_torch_us": [round(t, 1) for t in t_ref], "per_gemm": per}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
