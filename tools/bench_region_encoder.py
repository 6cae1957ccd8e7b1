"""The region encoder through Python, forward and forward + backward, with ``RegionEncoder.native_branch`` on (one call of
vllm_region_encoder_forward / _backward) and off (the torch modules of the mask stem, a permute and an add per level, the native masked
mean per level, up_dim per level, torch's autograd) on the same module, tensors and sampling points: the points are drawn once and
replayed, so neither path is charged ``rand_sample``.  Two cases, 16 regions, three levels given as hidden[:, 1:] views, 2304 points:
336 x 336 with embed 1024 / out 4096 (ViT-L) and 448 x 448 with embed 3200 / out 4096 (InternViT-6B).  Device events, warm-up first, the
paths alternated in one process, three rounds, the shader clock sampled meanwhile (bench.py's ClockSampler).  Also each new kernel alone,
as a fraction of the 6.29 TB/s copy rate the README uses.

    python tools/bench_region_encoder.py [--iters 100] [--warmup 3] [--case both|vitl|ivit6b]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ClockSampler  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import region_encoder as A  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README
CASES = {"vitl": (336, 1024, 4096), "ivit6b": (448, 3200, 4096)}
N, LEVELS, HIDDEN, PATCH = 16, 3, 256, 14


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


def kernels_alone(dev, side, embed, coords, valid, levels, iters):
    """the five new kernels at this case's shapes -> {name: {us, bytes, frac_copy_rate}}"""
    lib = _lib.lib()
    st = _lib.current_stream(torch.device(dev))
    h = side // PATCH
    hw, m2 = h * h, N * h * h
    m1, kpad, c1 = 4 * m2, (PATCH * PATCH + 63) // 64 * 64, HIDDEN // 4
    bf = torch.bfloat16
    images, masks = torch.randn(N, 3, side, side, device=dev, dtype=bf), torch.ones(N, 1, side, side, device=dev, dtype=bf)
    a1 = torch.empty(m1, kpad, device=dev, dtype=bf)
    x1, x2 = torch.randn(m1, c1, device=dev, dtype=bf), torch.randn(m2, HIDDEN, device=dev, dtype=bf)
    p1, y1, p2, y2 = torch.empty_like(x1), torch.empty_like(x1), torch.empty_like(x2), torch.empty_like(x2)
    w1, w2 = torch.ones(c1, device=dev, dtype=bf), torch.ones(HIDDEN, device=dev, dtype=bf)
    wk = torch.empty(LEVELS, N, hw, device=dev)
    stem = torch.randn(N, hw, embed, device=dev, dtype=bf)
    pooled, g = torch.empty(N, embed, device=dev, dtype=bf), torch.randn(N, embed, device=dev, dtype=bf)
    gmap = torch.empty(N, hw, embed, device=dev, dtype=bf)
    ptrs = (ctypes.c_void_p * LEVELS)(*[lv.data_ptr() for lv in levels])
    rs = (ctypes.c_long * LEVELS)(*[lv.stride(1) for lv in levels])
    ims = (ctypes.c_long * LEVELS)(*[lv.stride(0) for lv in levels])
    Pn = coords.shape[2]
    runs = {
        "region_im2col": (lambda: _lib.check(lib.vllm_region_im2col_bf16(P(images), P(masks), 0, P(a1), N, side, side, PATCH, kpad, st)),
                          N * 4 * side * side * 2 + m1 * kpad * 2),
        "layernorm_gelu_C64": (lambda: _lib.check(lib.vllm_layernorm_gelu_bf16(P(x1), c1, P(w1), P(w1), P(p1), P(y1), m1, c1, 1e-6, st)), m1 * c1 * 6),
        "layernorm_gelu_C256": (lambda: _lib.check(lib.vllm_layernorm_gelu_bf16(P(x2), HIDDEN, P(w2), P(w2), P(p2), P(y2), m2, HIDDEN, 1e-6, st)),
                                m2 * HIDDEN * 6),
        "region_pool_weights": (lambda: _lib.check(lib.vllm_region_pool_weights_f32(P(coords), P(valid), P(wk), N, LEVELS, h, h, Pn, st)),
                                LEVELS * N * (Pn * 9 + hw * 4)),
        "region_pool": (lambda: _lib.check(lib.vllm_region_pool_bf16(P(wk), P(stem), ptrs, rs, ims, N, LEVELS, hw, embed, P(pooled), st)),
                        (LEVELS + 1) * m2 * embed * 2 + (LEVELS + 1) * m2 * 4 + N * embed * 2),
        "region_outer": (lambda: _lib.check(lib.vllm_region_outer_bf16(P(wk), P(g), P(gmap), N, hw, embed, st)), m2 * embed * 2 + m2 * 4 + N * embed * 2),
    }
    out = {}
    for name, (fn, nbytes) in runs.items():
        for _ in range(3):
            fn()
        us = min(timed(fn, 20 * iters) for _ in range(3))   # (microsecond kernels: a longer window than the module paths get)
        out[name] = {"us": round(us, 1), "bytes": nbytes, "frac_copy_rate": round(nbytes / (us * 1e-6) / COPY_RATE, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--case", default="both", choices=["both"] + list(CASES))
    args = ap.parse_args()
    dev = "cuda:0"
    out = {}
    for name, (side, embed, out_dim) in CASES.items():
        if args.case not in ("both", name):
            continue
        torch.manual_seed(0)
        enc = A.RegionEncoder(hidden_dim=HIDDEN, embed_dim=embed, out_dim=out_dim, patch_size=PATCH, mask_pool_type="grid_sample")
        enc = enc.to(dev).to(torch.bfloat16).train()
        hw = (side // PATCH) ** 2
        images = torch.randn(N, 3, side, side, device=dev, dtype=torch.bfloat16)
        masks = torch.zeros(N, 1, side, side, device=dev, dtype=torch.bfloat16)
        for i in range(N):   # boxes of growing size, every one with more than 2304 pixels
            masks[i, 0, 10 + 5 * i:110 + 12 * i, 20:120 + 10 * i] = 1
        hidden = [torch.randn(N, 1 + hw, embed, device=dev, dtype=torch.bfloat16).requires_grad_(True) for _ in range(LEVELS)]
        levels = [t[:, 1:] for t in hidden]
        g = (torch.randn(N, out_dim, device=dev) / 16).to(torch.bfloat16)
        real = A.rand_sample
        divisor = torch.tensor([1, side, side], device=dev)[None,]
        drawn = [real(m, divisor, enc.num_points) for _ in range(LEVELS) for m in masks]
        state = {"i": 0}

        def replay(x, divisor, max_len):
            state["i"] = (state["i"] + 1) % len(drawn)
            return drawn[state["i"] - 1]

        A.rand_sample = replay

        def step(flag):
            def run():
                enc.native_branch = flag
                state["i"] = 0
                enc.zero_grad(set_to_none=True)
                for t in hidden:
                    t.grad = None
                enc(images, masks, levels).backward(g)
            return run

        def forward(flag):
            def run():
                enc.native_branch = flag
                state["i"] = 0
                with torch.no_grad():
                    enc(images, masks, levels)
            return run

        paths = {"native_fwd_bwd": step(True), "composed_fwd_bwd": step(False), "native_fwd": forward(True), "composed_fwd": forward(False)}
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
        A.rand_sample = real
        rec = {"regions": N, "side": side, "embed": embed, "out_dim": out_dim, "levels": LEVELS, "points": enc.num_points,
               "clocks": clocks if clocks else "no amdgpu hwmon files readable: clock not sampled"}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_composed_fwd_bwd"] = round(min(times["native_fwd_bwd"]) / min(times["composed_fwd_bwd"]), 3)
        rec["native_over_composed_fwd"] = round(min(times["native_fwd"]) / min(times["composed_fwd"]), 3)
        m2 = N * hw
        kpad, c1 = (PATCH * PATCH + 63) // 64 * 64, HIDDEN // 4
        rec["saved_bytes"] = 2 * (4 * m2 * (kpad + 3 * c1) + m2 * (3 * HIDDEN + embed) + N * embed)
        d = _lib.VllmRegionEncoder(hidden=HIDDEN, embed=embed, out_dim=out_dim, patch=PATCH, n=N, H=side, W=side, levels=LEVELS, points=enc.num_points,
                                   pixel_is_f32=0, eps=1e-6)
        rec["workspace_bytes"] = _lib.lib().vllm_region_encoder_workspace_bytes(ctypes.byref(d))
        enc.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
        coords = torch.stack([torch.stack([p[:, -2:].flip(-1) for p in drawn[l * N:(l + 1) * N]]) for l in range(LEVELS)]).float().contiguous()
        valid = torch.ones(coords.shape[:3], dtype=torch.uint8, device=dev)
        rec["kernels_alone"] = kernels_alone(dev, side, embed, coords, valid, [lv.detach() for lv in levels], args.iters)
        out[name] = rec
        del enc, hidden, levels
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
