"""The deformable encoder layer at inference through Python, BASELINE cfg 4 (B = 8, 37 485 tokens per image, d_model 256, 8 heads,
4 levels, 4 points, d_ffn 2048, ReLU), both flavours: the native call (``native_layer = True``: vllm_deform_enc_layer_forward) against
the composed path of the same module -- the reference's statements on torch around the fused attention call, which is what the class
runs with the switch off.  Device events, warm-up first, the two paths alternated in one process, the shader clock sampled meanwhile
(bench.py's ClockSampler).  Then the native call at each FFN slab height (option "deform_enc_ffn_slab_rows"), and each new kernel alone:
its time, the bytes it has to move (every operand read once, every result written once) and that as a fraction of the 6.29 TB/s copy
rate the README uses.

    python tools/bench_deform_encoder_layer.py [--iters 10] [--warmup 3] [--batch 8] [--slabs 0,65536,16384]
"""
import argparse
import ctypes
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import ClockSampler  # noqa: E402
from msda_inputs import CFG4_SHAPES  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import deformable_encoder as E  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README
C, M, P, F = 256, 8, 4, 2048


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def PT(t):
    return ctypes.c_void_p(t.data_ptr())


def make_layer(flavour, dev):
    L = len(CFG4_SHAPES)
    if flavour == "unipose":
        m = E.DeformableTransformerEncoderLayer(d_model=C, d_ffn=F, activation="relu", n_levels=L, n_heads=M, n_points=P)
    else:
        cfg = types.SimpleNamespace(d_model=C, num_feature_levels=L, encoder_attention_heads=M, encoder_n_points=P, encoder_ffn_dim=F,
                                    dropout=0.1, activation_function="relu", activation_dropout=0.0, disable_custom_kernels=False)
        m = E.GroundingDinoDeformableLayer(cfg)
    with torch.no_grad():
        m.self_attn.sampling_offsets.weight.normal_(0, 0.01)
    return m.to(dev).to(torch.bfloat16).eval()


def kernels_alone(R, dev, iters):
    """the layer's kernels on cfg 4's row count -> {name: {us, bytes, frac_copy_rate}}"""
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    x, pos, y, q = bf(R, C), bf(R, C), torch.empty(R, C, dtype=torch.bfloat16, device=dev), torch.empty(R, C, dtype=torch.bfloat16, device=dev)
    w, b = bf(C), bf(C)
    w1, b1, w2, b2 = bf(F, C) / 16, bf(F), bf(C, F) / 45, bf(C)
    h = torch.empty(R, F, dtype=torch.bfloat16, device=dev)
    ck = _lib.check
    runs = {
        "add_layernorm": (lambda: ck(lib.vllm_add_layernorm_bf16(PT(x), C, None, 0, PT(w), PT(b), PT(y), C, None, 0, None, 0, R, C, 1e-5, st)),
                          2 * R * C * 2),
        "add_layernorm_with_pos_out": (lambda: ck(lib.vllm_add_layernorm_bf16(PT(x), C, None, 0, PT(w), PT(b), PT(y), C, PT(pos), C, PT(q), C, R,
                                                                              C, 1e-5, st)), 4 * R * C * 2),
        "add": (lambda: ck(lib.vllm_add_bf16(PT(x), PT(pos), PT(y), R * C, st)), 3 * R * C * 2),
        "fc1_relu": (lambda: ck(lib.vllm_gemm_bf16_relu(PT(x), PT(w1), PT(b1), PT(h), R, F, C, C, C, F, 0, st)), R * C * 2 + R * F * 2 + F * C * 2),
        "fc2_residual": (lambda: ck(lib.vllm_gemm_bf16(PT(h), PT(w2), PT(b2), PT(y), R, C, F, F, F, C, _lib.EPI_RESIDUAL, None, PT(x), C, 0, st)),
                         R * F * 2 + 2 * R * C * 2 + F * C * 2),
        # linear1's GEMM with the plain bias epilogue on the persistent schedule and with one workgroup per tile (as EPI_RELU runs): whether
        # a persistent form of the ReLU epilogue would pay
        "fc1_bias_persistent": (lambda: ck(lib.vllm_gemm_bf16(PT(x), PT(w1), PT(b1), PT(h), R, F, C, C, C, F, _lib.EPI_BIAS, None, None, 0, 0, st)),
                                R * C * 2 + R * F * 2 + F * C * 2),
        "fc1_bias_tilewise": (lambda: ck(lib.vllm_gemm_bf16(PT(x), PT(w1), PT(b1), PT(h), R, F, C, C, C, F, _lib.EPI_BIAS | 0x1000, None, None, 0,
                                                            0, st)), R * C * 2 + R * F * 2 + F * C * 2),
    }
    persistent = lib.vllm_gemm_persistent_launches()
    runs["fc1_bias_persistent"][0]()
    took_persistent = lib.vllm_gemm_persistent_launches() - persistent
    res = {}
    for name, (fn, nbytes) in runs.items():
        for _ in range(3):
            fn()
        us = min(timed(fn, iters) for _ in range(3))
        res[name] = {"us": round(us, 1), "bytes": nbytes, "frac_copy_rate": round(nbytes / (us * 1e-6) / COPY_RATE, 3)}
    res["fc1_bias_persistent"]["took_the_persistent_schedule"] = bool(took_persistent)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--slabs", default="0,65536,16384", help="FFN slab heights to time the native call at (0 = the whole tensor)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deform_encoder_layer: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    B, L = args.batch, len(CFG4_SHAPES)
    S = sum(h * w for h, w in CFG4_SHAPES)
    torch.manual_seed(0)
    ss = torch.tensor(CFG4_SHAPES, device=dev)
    lsi = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    src = torch.randn(B, S, C, device=dev).to(torch.bfloat16)
    pos = (0.5 * torch.randn(B, S, C, device=dev)).to(torch.bfloat16)
    pts = []   # a query's reference point is its own pixel centre
    for h, w in CFG4_SHAPES:
        ys, xs = torch.meshgrid(torch.arange(h, device=dev) + 0.5, torch.arange(w, device=dev) + 0.5, indexing="ij")
        pts.append(torch.stack([xs.reshape(-1) / w, ys.reshape(-1) / h], -1))
    ref = torch.cat(pts)[None, :, None, :].expand(B, S, L, 2).contiguous()
    slab_default = lib.vllm_set_option(b"deform_enc_ffn_slab_rows", 0)
    lib.vllm_set_option(b"deform_enc_ffn_slab_rows", slab_default)
    out = {"B": B, "S": S, "rows": B * S, "d_model": C, "d_ffn": F, "activation": "relu", "slab_rows_default": slab_default}
    for flavour in ("unipose", "gdino"):
        mod = make_layer(flavour, dev)

        def run(flag, mod=mod, flavour=flavour):
            def fn():
                type(mod).native_layer = flag
                with torch.no_grad():
                    if flavour == "unipose":
                        return mod(src, pos, ref, ss, lsi, None)
                    return mod(src, None, pos, ref, ss, lsi)[0]
            return fn
        paths = {"native": run(True), "composed": run(False)}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        calls = lib.vllm_deform_enc_layer_calls()
        a, b = paths["native"]().float(), paths["composed"]().float()
        assert lib.vllm_deform_enc_layer_calls() == calls + 1, "the native path did not run"
        rel = ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
        del a, b
        times = {k: [] for k in paths}
        clk = ClockSampler(dev)
        sampled = clk.has_sysfs()
        if sampled:
            clk.start()
        for _ in range(3):   # alternated
            for k, fn in paths.items():
                times[k].append(timed(fn, args.iters))
        slabs = {}
        for rows in [int(s) for s in args.slabs.split(",")]:
            lib.vllm_set_option(b"deform_enc_ffn_slab_rows", rows)
            paths["native"]()
            slabs[str(rows)] = []
        for _ in range(3):   # the heights alternated too
            for rows in slabs:
                lib.vllm_set_option(b"deform_enc_ffn_slab_rows", int(rows))
                slabs[rows].append(timed(paths["native"], args.iters))
        lib.vllm_set_option(b"deform_enc_ffn_slab_rows", slab_default)
        clocks = clk.stop() if sampled else None
        type(mod).native_layer = False
        rec = {"clocks": clocks if clocks else "no amdgpu hwmon files readable: clock not sampled", "native_vs_composed_rel_rms": round(rel, 5)}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_composed"] = round(min(times["native"]) / min(times["composed"]), 3)
        rec["aim_native_le_composed"] = "met" if rec["native_over_composed"] <= 1.0 else "not met"
        rec["native_us_by_slab_rows"] = {k: {"us": round(min(v), 1), "all_us": [round(t, 1) for t in v]} for k, v in slabs.items()}
        out[flavour] = rec
        del mod, paths
        torch.cuda.empty_cache()
    out["kernels_alone"] = kernels_alone(B * S, dev, args.iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
