"""The DCNv3 layer at inference through Python: the native call (``DCNv3.native_layer = True``: vllm_dcnv3_layer_forward, five launches)
against the composed bf16 path of the same module (permutes, nn.Conv2d, LayerNorm, GELU, three linears, softmax, the fp32 upcasts around
the native operator, the centre-feature blend) -- the only path before the native layer.  InternImage-H stages (dw_kernel_size 5, centre
feature scale on), N = 1: 168^2 x 640 / 20 groups, 84^2 x 1280 / 40 groups and, if memory allows, 336^2 x 320 / 10 groups.  Device events,
warm-up first, the two paths alternated in one process, the shader clock sampled meanwhile (bench.py's ClockSampler).  Also each new kernel
alone: its time, the bytes it has to move (input read once, output written once, the fp32 rows it reads) and that as a fraction of the
6.29 TB/s copy rate the README uses.

    python tools/bench_dcnv3_layer.py [--iters 20] [--warmup 5] [--shapes 168,84,336]
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
from visionllm_amd.dcnv3 import DCNv3  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README
STAGES = {336: (320, 10), 168: (640, 20), 84: (1280, 40), 42: (2560, 80)}   # map side -> (channels, groups) of build_internimage_h


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def kernels_alone(mod, x, iters):
    """the two new kernels on tensors of this shape -> {name: {us, bytes, frac_copy_rate}}"""
    lib = _lib.lib()
    st = _lib.current_stream(x.device)
    N, H, W, C = x.shape
    R, G = N * H * W, mod.group
    conv, ln = mod.dw_conv[0], mod.dw_conv[1][-1]
    pw, _ = mod.packed_projection()
    n_proj = pw.shape[0]
    om = torch.randn(R, n_proj, device=x.device) * 1.6
    out = torch.empty_like(x)
    k2 = conv.weight.shape[-1] ** 2
    runs = {
        "dwconv_ln_gelu": (lambda: _lib.check(lib.vllm_dwconv_ln_gelu_bf16(P(x), P(conv.weight), P(conv.bias), P(ln.weight), P(ln.bias), N, H, W,
                                                                          C, conv.weight.shape[-1], float(ln.eps), P(out), st)),
                           R * C * 4 + C * (k2 + 3) * 2),
        "dcnv3_sample_fused": (lambda: _lib.check(lib.vllm_dcnv3_sample_fused_bf16(P(x), P(om), n_proj, N, H, W, G, C // G, mod.dilation,
                                                                                  float(mod.offset_scale), 1, P(out), st)),
                               R * C * 4 + R * 28 * G * 4),
    }
    res = {}
    for name, (fn, nbytes) in runs.items():
        for _ in range(3):
            fn()
        us = min(timed(fn, iters) for _ in range(3))
        res[name] = {"us": round(us, 1), "bytes": nbytes, "frac_copy_rate": round(nbytes / (us * 1e-6) / COPY_RATE, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="168,84,336", help="map sides, out of " + ",".join(str(s) for s in STAGES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcnv3_layer: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    out = {}
    for side in [int(s) for s in args.shapes.split(",")]:
        C, G = STAGES[side]
        torch.manual_seed(side)
        mod = DCNv3(channels=C, group=G, dw_kernel_size=5, center_feature_scale=True).eval()
        with torch.no_grad():
            std = 1.5 / (0.43 * C) ** 0.5    # offsets of about 1.5 px, as the tests use
            for p in (mod.offset.weight, mod.mask.weight, mod.center_feature_scale_proj_weight):
                p.normal_(0, std)
        try:
            mod = mod.to(dev).to(torch.bfloat16)
            x = torch.randn(1, side, side, C, device=dev).to(torch.bfloat16)

            def run(flag):
                def fn():
                    mod.native_layer = flag
                    with torch.no_grad():
                        return mod(x)
                return fn
            paths = {"native": run(True), "composed": run(False)}
            for _ in range(args.warmup):
                for fn in paths.values():
                    fn()
        except torch.cuda.OutOfMemoryError:
            out[str(side)] = "out of memory: not measured"
            torch.cuda.empty_cache()
            continue
        calls = _lib.lib().vllm_dcnv3_layer_calls()
        a, b = paths["native"]().float(), paths["composed"]().float()
        assert _lib.lib().vllm_dcnv3_layer_calls() == calls + 1, "the native path did not run"
        rel = ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
        times = {k: [] for k in paths}
        clk = ClockSampler(dev)
        sampled = clk.has_sysfs()
        if sampled:
            clk.start()
        for _ in range(3):   # alternated
            for k, fn in paths.items():
                times[k].append(timed(fn, args.iters))
        clocks = clk.stop() if sampled else None
        rec = {"N": 1, "H": side, "W": side, "channels": C, "group": G, "dw_kernel_size": 5, "center_feature_scale": True,
               "clocks": clocks if clocks else "no amdgpu hwmon files readable: clock not sampled",
               "native_vs_composed_rel_rms": round(rel, 5)}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_composed"] = round(min(times["native"]) / min(times["composed"]), 3)
        rec["aim_native_le_composed"] = "met" if rec["native_over_composed"] <= 1.0 else "not met"
        mod.native_layer = False
        rec["kernels_alone"] = kernels_alone(mod, x, args.iters)
        out[str(side)] = rec
        del mod, x, paths
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
