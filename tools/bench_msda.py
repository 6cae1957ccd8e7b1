#!/usr/bin/env python3
"""MSDA forward micro-benchmark at BASELINE cfg 4 (run on the GPU box).  Routes: fp32 automatic (generation 9 on nested maps, else 4),
fp32 with the general-geometry hint (generation 4 on any maps), fp32 gather kernel, bf16 automatic (generation 6 on exact pyramids),
bf16 gather kernel; + the backward."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from msda_inputs import CFG4_SHAPES, make_inputs  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import ms_deform_attn as A  # noqa: E402


def set_tiled(value):
    """vllm_set_option("msda_tiled", value) -> the previous value; stops on a refused value (carrying on would time the previous
    mode under the new label)."""
    old = _lib.set_option("msda_tiled", value)
    if old < 0:
        sys.exit(f"msda_tiled = {value} refused: {_lib.lib().vllm_last_error().decode()}")
    return old


def forward_general(t):
    """fp32 forward with the VLLM_GEO_GENERAL hint: at the encoder shape, generation 4 on any level maps."""
    v, loc = t["value"], t["loc"]
    B, S, M, D = v.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    out = torch.empty((B, Lq, M * D), dtype=torch.float32, device=v.device)
    _lib.check(_lib.lib().vllm_msda_forward_f32_geo(_lib.ptr(v), _lib.ptr(t["shapes"]), _lib.ptr(t["lsi"]), _lib.ptr(loc),
                                                    _lib.ptr(t["attw"]), B, S, M, D, L, Lq, P, A.GEO_GENERAL, _lib.ptr(out),
                                                    _lib.current_stream(v.device)), "vllm_msda_forward_f32_geo")
    return out


# route -> (value dtype, msda_tiled, general-geometry hint)
ROUTES = {"f32_auto": ("f32", 1, False), "f32_general": ("f32", 1, True), "f32_gather": ("f32", 0, False),
          "bf16_auto": ("bf16", 1, False), "bf16_gather": ("bf16", 0, False)}


def algorithmic_bytes(B, S, M, D, L, Lq, P, vbytes=4):
    # value + loc + attw + out
    return B * S * M * D * vbytes + B * Lq * M * L * P * 2 * 4 + B * Lq * M * L * P * 4 + B * Lq * M * D * vbytes


def timeit(fn, iters, warmup=3, rounds=3):
    """min over `rounds` event-timed loops (the first loop after an idle gap / on freshly allocated operands reads 5-12 % slow:
    clocks ramp, first-touch TLB fills -- a single loop made the first variant of a list look slower than the same kernel later)."""
    best = 1e9
    for _ in range(rounds):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / iters * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--modes", default="encoder_like,stress")
    a = ap.parse_args()
    dev = "cuda:0"
    res = []
    for mode in a.modes.split(","):
        for lq in (None, 900):
            g1 = make_inputs(1, 8, 32, CFG4_SHAPES, 4, Lq=lq if (lq or mode != "stress") else 37485, mode=mode, seed=0)
            t = {k: torch.from_numpy(v).to(dev) for k, v in g1.items()}
            for k in ("value", "loc", "attw"):  # replicate batch on device (same distribution, distinct memory)
                t[k] = t[k].repeat(a.B, *([1] * (t[k].dim() - 1))).contiguous()
                if k == "value":
                    t[k] = t[k] + 0.01 * torch.randn_like(t[k])
            B, S, M, D = t["value"].shape
            Lq, L, P = t["loc"].shape[1], t["loc"].shape[3], t["loc"].shape[4]
            for dt, (vt, tiled, general) in ROUTES.items():
                tv = dict(t, value=t["value"] if vt == "f32" else t["value"].bfloat16())
                set_tiled(tiled)
                if general:
                    fn = lambda: forward_general(tv)
                else:
                    fn = lambda: A.ms_deform_attn_forward(tv["value"], tv["shapes"], tv["lsi"], tv["loc"], tv["attw"], 64)
                sec = timeit(fn, a.iters)
                ab = algorithmic_bytes(B, S, M, D, L, Lq, P, 2 if dt.startswith("bf16") else 4)
                gathered = B * Lq * M * L * P * 4 * D * (2 if dt.startswith("bf16") else 4)
                r = dict(mode=mode, dtype=dt, B=B, Lq=Lq, us=sec * 1e6, algo_GBs=ab / sec / 1e9,
                         frac_of_8TBs=ab / sec / 8e12, gathered_TBs=gathered / sec / 1e12)
                res.append(r)
                print(json.dumps(r))
    # backward (training of the det heads): encoder shape, fp32
    g1 = make_inputs(1, 8, 32, CFG4_SHAPES, 4, mode="encoder_like", seed=0)
    t = {k: torch.from_numpy(v).to(dev) for k, v in g1.items()}
    for k in ("value", "loc", "attw"):
        t[k] = t[k].repeat(a.B, *([1] * (t[k].dim() - 1))).contiguous()
    go = torch.randn(a.B, t["loc"].shape[1], 256, device=dev)
    for name, mode in (("f32_backward_tiled", 1), ("f32_backward_plain_atomics", 0)):
        old = set_tiled(mode)
        sec = timeit(lambda: A.ms_deform_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["attw"], go, 64), 5)
        set_tiled(old)
        print(json.dumps(dict(mode="encoder_like", dtype=name, B=a.B, Lq=int(t["loc"].shape[1]), us=sec * 1e6)))
    return res


if __name__ == "__main__":
    main()
