"""The deformable-attention layer, training step (forward + backward) through Python: the native node (``native_training = True``:
vllm_msda_layer_forward_train / vllm_msda_layer_backward) against the composed bf16 path (four nn.Linear, softmax and location
arithmetic in torch, the fp32 upcast around the native operator, torch's autograd) on the same module -- the only training path before
the native node.  BASELINE cfg 4 (B = 8, d_model 256, 8 heads, 4 levels, 4 points): the encoder shape (the queries are the cells of the
maps) and a decoder shape (900 queries on the same maps).  Device events, warm-up first, the two paths alternated in one process, the
shader clock sampled meanwhile (bench.py's ClockSampler).  Also each new kernel alone, as a fraction of the 6.29 TB/s copy rate the
README uses.

    python tools/bench_msda_layer_train.py [--iters 10] [--warmup 3] [--case both|encoder|decoder]
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
from bench import ClockSampler  # noqa: E402
from msda_inputs import CFG4_SHAPES  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import ms_deform_attn as A  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README


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


def kernels_alone(dev, B, Lq, S, C, M, L, Pn, iters):
    """the three elementwise kernels on tensors of this shape -> {name: {us, bytes, frac_copy_rate}}"""
    lib = _lib.lib()
    st = _lib.current_stream(torch.device(dev))
    R, MLP = B * Lq, M * L * Pn
    N = (3 * MLP + 63) // 64 * 64
    gl, gw = torch.randn(R, MLP * 2, device=dev), torch.randn(R, MLP, device=dev)
    w = torch.softmax(torch.randn(R, M, L * Pn, device=dev), -1).reshape(R, MLP).contiguous()
    ref = torch.rand(R, L, 2, device=dev)
    ss = torch.tensor(CFG4_SHAPES, device=dev)
    dq = torch.empty(R, N, device=dev, dtype=torch.bfloat16)
    gv = torch.randn(B * S, C, device=dev)
    gv16 = torch.empty(B * S, C, device=dev, dtype=torch.bfloat16)
    mask = (torch.rand(B * S, device=dev) < 0.1).to(torch.uint8)
    wide = torch.empty(B * S, C, device=dev)
    runs = {
        "msda_prep_backward": (lambda: _lib.check(lib.vllm_msda_prep_backward_f32(P(gl), P(gw), P(w), P(ref), P(ss), R, M, L, Pn, 2, 0, P(dq), N, st)),
                               R * MLP * 16 + R * L * 8 + R * N * 2),
        "f32_to_bf16_masked": (lambda: _lib.check(lib.vllm_f32_to_bf16_masked(P(gv), P(gv16), B * S, C, P(mask), st)), B * S * C * 6 + B * S),
        "bf16_to_f32": (lambda: _lib.check(lib.vllm_bf16_to_f32(P(gv16), P(wide), B * S * C, st)), B * S * C * 6),
    }
    out = {}
    for name, (fn, nbytes) in runs.items():
        for _ in range(3):
            fn()
        us = min(timed(fn, iters) for _ in range(3))
        out[name] = {"us": round(us, 1), "bytes": nbytes, "frac_copy_rate": round(nbytes / (us * 1e-6) / COPY_RATE, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default="both", choices=["both", "encoder", "decoder"])
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    B, C, M, L, Pn = 8, 256, 8, 4, 4
    S = sum(h * w for h, w in CFG4_SHAPES)
    mod = A.MSDeformAttn(C, L, M, Pn).to(dev).to(torch.bfloat16)
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.01)
        mod.attention_weights.weight.normal_(0, 0.05)
    ss = torch.tensor(CFG4_SHAPES, device=dev)
    lsi = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    src = torch.randn(B, S, C, device=dev).to(torch.bfloat16).requires_grad_(True)
    out = {}
    for name, Lq in (("encoder", S), ("decoder", 900)):
        if args.case not in ("both", name):
            continue
        q = torch.randn(B, Lq, C, device=dev).to(torch.bfloat16).requires_grad_(True)
        g = (torch.randn(B, Lq, C, device=dev) / 16).to(torch.bfloat16)
        if Lq == S:   # encoder self-attention: a query's reference point is its own pixel centre
            pts = []
            for h, w in CFG4_SHAPES:
                ys, xs = torch.meshgrid(torch.arange(h, device=dev) + 0.5, torch.arange(w, device=dev) + 0.5, indexing="ij")
                pts.append(torch.stack([xs.reshape(-1) / w, ys.reshape(-1) / h], -1))
            ref = torch.cat(pts)[None, :, None, :].expand(B, S, L, 2).contiguous()
        else:
            ref = torch.rand(B, Lq, L, 2, device=dev)

        def step(flag):
            def run():
                mod.native_training = flag
                mod.zero_grad(set_to_none=True)
                q.grad = src.grad = None
                mod(q, ref, src, ss, lsi, None).backward(g)
            return run

        def forward_only():
            with torch.no_grad():
                mod(q, ref, src, ss, lsi, None)
        paths = {"native": step(True), "composed": step(False), "inference_forward_only": forward_only}
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
        rec = {"B": B, "Lq": Lq, "S": S, "d_model": C, "heads": M, "levels": L, "points": Pn,
               "clocks": clocks if clocks else "no amdgpu hwmon files readable: clock not sampled"}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_composed"] = round(min(times["native"]) / min(times["composed"]), 3)
        desc = _lib.VllmMsdaLayerDesc(d_model=C, n_heads=M, n_levels=L, n_points=Pn, ref_dim=2, value_proj_w=1, sampling_offsets_w=1,
                                      attention_weights_w=1, output_proj_w=1)
        rec["saved_bytes"] = _lib.lib().vllm_msda_layer_saved_bytes(ctypes.byref(desc), B, Lq, S)
        rec["backward_workspace_bytes"] = _lib.lib().vllm_msda_layer_backward_workspace_bytes(ctypes.byref(desc), B, Lq, S)
        mod.native_training = False
        mod.zero_grad(set_to_none=True)
        q.grad = src.grad = None
        torch.cuda.empty_cache()
        rec["kernels_alone"] = kernels_alone(dev, B, Lq, S, C, M, L, Pn, args.iters)
        out[name] = rec
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
