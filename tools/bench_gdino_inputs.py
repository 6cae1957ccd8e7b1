"""The inputs of the Grounding-DINO encoder at inference through Python, BASELINE cfg 4's levels (168^2 / 84^2 / 42^2 from the backbone + one
extra level 21^2, 37 485 cells per image), B = 8, d_model 256, bf16, with the channels of InternImage-H (640, 1280, 2560) and of Swin-T
(192, 384, 768), each with contiguous NCHW maps and with channels-last maps: the same GroundingDinoEncoderInputs module with
``native_inputs = True`` (ONE vllm_gdino_inputs_forward) against the switch off (the reference's statements in torch) on the same tensors.
Device events, warm-up first, the two paths alternated in one process over five rounds, medians reported, the shader clock sampled
meanwhile (bench.py's ClockSampler).  Then the five new kernels alone at the InternImage-H shapes, with the bytes each has to move as a
fraction of the 6.29 TB/s copy rate, and the workspace size.  Recorded, not gated.

    python tools/bench_gdino_inputs.py [--iters 5] [--warmup 2] [--batch 8] [--kernel-iters 50] [--only internimage_h]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import ClockSampler  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import gdino_inputs as G  # noqa: E402

C, N_LEVELS, ROUNDS = 256, 4, 5
MAPS = ((168, 168), (84, 84), (42, 42))
LEVELS = MAPS + ((21, 21),)
PIXELS = (1344, 1344)
BACKBONES = {"internimage_h": (640, 1280, 2560), "swin_t": (192, 384, 768)}
COPY_RATE = 6.29e12   # bytes / s, read + write counted


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def PT(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def clocked(fns, iters, dev, rounds=ROUNDS):
    """`rounds` alternated rounds of `iters` calls of every function -> ({name: [us]}, clocks)"""
    times = {k: [] for k in fns}
    clk = ClockSampler(dev)
    sampled = clk.has_sysfs()
    if sampled:
        clk.start()
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    clocks = clk.stop() if sampled else None
    return times, (clocks if clocks else "no amdgpu hwmon files readable: clock not sampled")


def make_module(in_channels, dev):
    cfg = types.SimpleNamespace(d_model=C, num_feature_levels=N_LEVELS, positional_embedding_temperature=20, position_embedding_type="sine")
    m = G.GroundingDinoEncoderInputs(cfg, in_channels).to(dev).to(torch.bfloat16).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def pixel_mask(B, dev):
    """image b keeps 100 % - 4 b % of its height and 100 % - 3 b % of its width"""
    m = torch.zeros((B,) + PIXELS, dtype=torch.int64, device=dev)
    for b in range(B):
        m[b, :int(PIXELS[0] * (1 - 0.04 * b)), :int(PIXELS[1] * (1 - 0.03 * b))] = 1
    return m


def module_case(name, fmt, B, dev, args):
    lib = _lib.lib()
    mod = make_module(BACKBONES[name], dev)
    maps = [torch.randn(B, c, h, w, device=dev).to(torch.bfloat16) for c, (h, w) in zip(BACKBONES[name], MAPS)]
    if fmt == "channels_last":
        maps = [m.contiguous(memory_format=torch.channels_last) for m in maps]
    pm = pixel_mask(B, dev)
    assert mod.native_inputs_reasons(maps, pm) == [], mod.native_inputs_reasons(maps, pm)

    def run(flag):
        def fn():
            mod.native_inputs = flag
            with torch.no_grad():
                return mod(maps, pm)
        return fn
    paths = {"native": run(True), "composed": run(False)}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    n0 = lib.vllm_gdino_inputs_calls()
    a = paths["native"]()
    assert lib.vllm_gdino_inputs_calls() == n0 + 1, "the native path did not run"
    b = paths["composed"]()
    assert lib.vllm_gdino_inputs_calls() == n0 + 1
    rel = lambda x, y: round(((x.float() - y.float()).pow(2).mean().sqrt() / y.float().pow(2).mean().sqrt()).item(), 5)
    agree = {"source_rel_rms": rel(a.source_flatten, b.source_flatten), "pos_rel_rms": rel(a.lvl_pos_embed_flatten, b.lvl_pos_embed_flatten),
             "mask_equal": torch.equal(a.mask_flatten, b.mask_flatten), "valid_ratios_equal": torch.equal(a.valid_ratios, b.valid_ratios)}
    del a, b
    times, clocks = clocked(paths, args.iters, dev)
    d = mod._native_state(dev)["desc"]
    ws = lib.vllm_gdino_inputs_workspace_bytes(ctypes.byref(d), B, ints(*(h for h, _ in MAPS)), ints(*(w for _, w in MAPS)),
                                               ints(*([1 if fmt == "channels_last" else 0] * len(MAPS))))
    med = {k: statistics.median(v) for k, v in times.items()}
    rec = {"clocks": clocks, "native_vs_composed": agree, "workspace_bytes": ws,
           "map_bytes": sum(m.numel() * 2 for m in maps), "output_bytes": 2 * B * sum(h * w for h, w in LEVELS) * C * 2}
    for k, v in times.items():
        rec[k + "_median_us"] = round(med[k], 1)
        rec[k + "_all_us"] = [round(t, 1) for t in v]
    rec["native_over_composed"] = round(med["native"] / med["composed"], 3)
    rec["aim_native_le_composed"] = "met" if med["native"] <= med["composed"] else "not met"
    return rec


def kernels_alone(B, dev, iters):
    """the five kernels at InternImage-H's cfg-4 shapes; `bytes`: what the kernel has to read and write once"""
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    ck = _lib.check
    bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    S = sum(h * w for h, w in LEVELS)
    hw0, cin0 = MAPS[0][0] * MAPS[0][1], BACKBONES["internimage_h"][0]
    x0, rows0 = bf(B, cin0, hw0), torch.empty(B * hw0, cin0, dtype=torch.bfloat16, device=dev)
    conv0, gamma, beta = bf(B * hw0, C), bf(C), bf(C)
    source = torch.empty(B, S, C, dtype=torch.bfloat16, device=dev)
    gn_ws = torch.empty(lib.vllm_groupnorm_rows_workspace_bytes(B, hw0, C) + 256, dtype=torch.uint8, device=dev)
    hi, wi, cin2 = MAPS[2][0], MAPS[2][1], BACKBONES["internimage_h"][2]
    last, col = bf(B * hi * wi, cin2), torch.empty(B * LEVELS[3][0] * LEVELS[3][1], 9 * cin2, dtype=torch.bfloat16, device=dev)
    pm = pixel_mask(B, dev)
    om = torch.empty(B, S, dtype=torch.uint8, device=dev)
    yc, xc = torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)
    vr = torch.empty(B, N_LEVELS, 2, device=dev)
    lh, lw = ints(*(h for h, _ in LEVELS)), ints(*(w for _, w in LEVELS))
    level_embed = bf(N_LEVELS, C)
    dim_t = G.GroundingDinoSinePositionEmbedding(C // 2, 20, normalize=True).dim_t(dev).contiguous()
    pos = torch.empty(B, S, C, dtype=torch.bfloat16, device=dev)
    fns = {
        "nchw_to_rows_level0": lambda: ck(lib.vllm_nchw_to_rows_bf16(PT(x0), B, cin0, hw0, PT(rows0), cin0, st)),
        "groupnorm_rows_level0": lambda: ck(lib.vllm_groupnorm_rows_bf16(PT(conv0), C, PT(gamma), PT(beta), 1e-5, B, hw0, C, PT(source), S * C, C,
                                                                         PT(gn_ws), gn_ws.numel() - 256, st)),
        "im2col3x3s2_level3": lambda: ck(lib.vllm_im2col3x3s2_bf16(PT(last), hi * wi * cin2, cin2, B, hi, wi, cin2, PT(col), st)),
        "pixel_mask_levels": lambda: ck(lib.vllm_pixel_mask_levels_u8(PT(pm), 8, B, PIXELS[0], PIXELS[1], lh, lw, N_LEVELS, PT(om), PT(yc), PT(xc),
                                                                       PT(vr), st)),
        "sine_pos_embed_rows": lambda: ck(lib.vllm_sine_pos_embed_rows_bf16(PT(yc), PT(xc), lh, lw, N_LEVELS, B, C, PT(level_embed), PT(dim_t), PT(pos), st)),
    }
    nbytes = {"nchw_to_rows_level0": 2 * x0.numel() * 2, "groupnorm_rows_level0": 3 * conv0.numel() * 2, "im2col3x3s2_level3": last.numel() * 2 + col.numel() * 2,
              "pixel_mask_levels": B * S * (2 * 8 + 1 + 8), "sine_pos_embed_rows": B * S * (C * 2 + 16)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    times, clocks = clocked(fns, iters, dev)
    rec = {"clocks": clocks}
    for name, t in times.items():
        us = statistics.median(t)
        rate = nbytes[name] / (us * 1e-6)
        rec[name] = {"median_us": round(us, 2), "all_us": [round(x, 2) for x in t], "bytes": nbytes[name], "bytes_per_s": round(rate, 0),
                     "fraction_of_copy_rate": round(rate / COPY_RATE, 3)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--only", choices=sorted(BACKBONES), help="one backbone's channels instead of both")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gdino_inputs: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.batch
    out = {"B": B, "levels": LEVELS, "d_model": C, "rounds": ROUNDS, "iters": args.iters, "statistic": "median of the rounds", "cases": {}}
    for name in ([args.only] if args.only else sorted(BACKBONES)):
        for fmt in ("nchw", "channels_last"):
            out["cases"][f"{name}_{fmt}"] = module_case(name, fmt, B, dev, args)
            torch.cuda.empty_cache()
    out["kernel_iters"] = args.kernel_iters
    out["kernels_alone"] = kernels_alone(B, dev, args.kernel_iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
