"""The Grounding-DINO decoder at inference through Python, BASELINE cfg 4's decoder shape (B = 8, 900 queries -- and 1100 with a
denoising mask -- over 37 485 memory tokens per image, d_model 256, 8 heads, 4 levels, 4 points, d_ffn 2048, 256 text tokens, 6 layers,
one shared box head): the native call (``native_decoder = True``: vllm_deform_decoder_forward) against the same module with the switch
off, in two runs -- (1) every layer composed, (2) every layer with ``native_layer = True`` -- on the same tensors.  Device events, warm-up
first, the three paths alternated in one process over five rounds, medians reported, the shader clock sampled meanwhile (bench.py's
ClockSampler).  Then the two new kernels alone (vllm_refpoint_embed_bf16, vllm_box_refine_f32) with the bytes they must move over their
time as a fraction of the 6.29 TB/s copy rate: recorded, not gated.

    python tools/bench_deform_decoder.py [--iters 20] [--warmup 3] [--batch 8] [--kernel-iters 500]
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
from msda_inputs import CFG4_SHAPES  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import deformable_decoder as D  # noqa: E402

C, M, P, F, LT, LAYERS = 256, 8, 4, 2048, 256, 6
COPY_RATE = 6.29e12   # bytes / s, the device's measured copy rate
ROUNDS = 5


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


def make_decoder(dev):
    cfg = types.SimpleNamespace(d_model=C, num_feature_levels=len(CFG4_SHAPES), decoder_attention_heads=M, decoder_n_points=P,
                                decoder_ffn_dim=F, dropout=0.1, attention_dropout=0.0, activation_function="relu", activation_dropout=0.0,
                                disable_custom_kernels=False, decoder_layers=LAYERS, query_dim=4, use_return_dict=False)
    m = D.GroundingDinoDecoder(cfg)
    head = D.GroundingDinoMLPPredictionHead(C, C, 4, 3)
    with torch.no_grad():
        for layer in m.layers:
            layer.encoder_attn.sampling_offsets.weight.normal_(0, 0.01)
        head.layers[-1].weight.mul_(0.1)
    m.bbox_embed = torch.nn.ModuleList([head] * LAYERS)          # decoder_bbox_embed_share
    return m.to(dev).to(torch.bfloat16).eval()


def denoise_mask(Lq, dn, dev):
    """bool [Lq, Lq], True = may NOT attend: `dn` denoising rows in two groups in front of the matching queries"""
    m = torch.zeros(Lq, Lq, dtype=torch.bool, device=dev)
    half = dn // 2
    m[dn:, :dn] = True
    m[:half, half:dn] = True
    m[half:dn, :half] = True
    return m


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


def decoder_case(mod, Lq, masked, B, S, ss, lsi, dev, args):
    lib = _lib.lib()
    L = len(CFG4_SHAPES)
    bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    tgt, memory, text = bf(B, Lq, C), bf(B, S, C), bf(B, LT, C)
    ref = torch.cat([torch.rand(B, Lq, 2, device=dev), 0.05 + 0.3 * torch.rand(B, Lq, 2, device=dev)], -1)
    vr = 1.0 - 0.3 * torch.rand(B, L, 2, device=dev)
    sam = denoise_mask(Lq, Lq - 900, dev) if masked else None
    tmask = torch.zeros(B, LT, dtype=torch.bool, device=dev)
    for b in range(B):
        tmask[b, LT - 16 * (b + 1):] = True

    def run(decoder_flag, layer_flag):
        def fn():
            D.GroundingDinoDecoder.native_decoder = decoder_flag
            D.GroundingDinoDecoderLayer.native_layer = layer_flag
            with torch.no_grad():
                return mod(tgt, memory, None, None, text, tmask, ref, ss, lsi, vr, sam)
        return fn
    paths = {"native_decoder": run(True, False), "composed_layers_composed": run(False, False), "composed_layers_native": run(False, True)}
    try:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        calls, layer_calls = lib.vllm_deform_decoder_calls(), lib.vllm_deform_dec_layer_calls()
        a = paths["native_decoder"]()
        assert lib.vllm_deform_decoder_calls() == calls + 1 and lib.vllm_deform_dec_layer_calls() == layer_calls, "the native path did not run"
        b = paths["composed_layers_native"]()
        assert lib.vllm_deform_decoder_calls() == calls + 1 and lib.vllm_deform_dec_layer_calls() == layer_calls + LAYERS
        rel = lambda x, y: round(((x.float() - y.float()).pow(2).mean().sqrt() / y.float().pow(2).mean().sqrt()).item(), 5)
        agree = {"intermediate_rel_rms_per_layer": [rel(a[1][:, l], b[1][:, l]) for l in range(LAYERS)],
                 "reference_points_rel_rms_per_layer": [rel(a[2][:, l], b[2][:, l]) for l in range(LAYERS)]}
        del a, b
        times, clocks = clocked(paths, args.iters, dev)
    finally:
        D.GroundingDinoDecoder.native_decoder = False
        D.GroundingDinoDecoderLayer.native_layer = False
    rec = {"Lq": Lq, "denoising_mask": bool(masked), "clocks": clocks, "native_vs_composed_layers_native": agree}
    for k, v in times.items():
        rec[k + "_median_us"] = round(statistics.median(v), 1)
        rec[k + "_all_us"] = [round(t, 1) for t in v]
    med = lambda k: statistics.median(times[k])
    rec["native_over_run1_layers_composed"] = round(med("native_decoder") / med("composed_layers_composed"), 3)
    rec["native_over_run2_layers_native"] = round(med("native_decoder") / med("composed_layers_native"), 3)
    rec["loop_around_the_layers_us"] = round(med("composed_layers_native") - med("native_decoder"), 1)
    rec["aim_native_le_run2"] = "met" if med("native_decoder") <= med("composed_layers_native") else "not met"
    return rec


def kernels_alone(B, dev, iters):
    """the two row kernels at both row counts: time, the bytes they must move, and that over the time as a fraction of the copy rate"""
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    L, Pf = len(CFG4_SHAPES), C // 2
    out = {}
    dim_t = D.GroundingDinoDecoder._dim_t(Pf, dev)
    for Lq in (900, 1100):
        R = B * Lq
        ref = torch.rand(B, Lq, 4, device=dev)
        vr = 1.0 - 0.3 * torch.rand(B, L, 2, device=dev)
        rpi = torch.empty(B, Lq, L, 4, device=dev)
        sine = torch.empty(R, 4 * Pf, dtype=torch.bfloat16, device=dev)
        h = torch.randn(R, C, device=dev).relu().to(torch.bfloat16)
        W = (torch.randn(4, C, device=dev) / 16).to(torch.bfloat16)
        b = torch.zeros(4, dtype=torch.bfloat16, device=dev)
        new = torch.empty(R, 4, device=dev)
        ck = _lib.check
        fns = {
            "refpoint_embed": lambda: ck(lib.vllm_refpoint_embed_bf16(PT(ref), PT(vr), PT(dim_t), B, Lq, L, 4, Pf, PT(rpi), PT(sine), 4 * Pf, st)),
            "box_refine": lambda: ck(lib.vllm_box_refine_f32(PT(h), C, PT(W), PT(b), PT(ref.view(R, 4)), PT(new), R, C, 1e-5, st)),
        }
        nbytes = {"refpoint_embed": R * 16 + B * L * 8 + Pf * 4 + R * L * 16 + R * 4 * Pf * 2, "box_refine": R * C * 2 + 4 * C * 2 + 8 + R * 16 + R * 16}
        for fn in fns.values():
            for _ in range(3):
                fn()
        times, clocks = clocked(fns, iters, dev)
        rec = {"rows": R, "clocks": clocks}
        for k, v in times.items():
            us = statistics.median(v)
            rec[k] = {"median_us": round(us, 2), "all_us": [round(t, 2) for t in v], "bytes": nbytes[k],
                      "fraction_of_copy_rate": round(nbytes[k] / (us * 1e-6) / COPY_RATE, 4)}
        out[f"Lq_{Lq}"] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=500, help="calls per timing of the kernels alone: they take microseconds, and a "
                    "timing must last several periods of the 20 ms clock sampler for its median clock to mean something")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deform_decoder: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    B = args.batch
    S = sum(h * w for h, w in CFG4_SHAPES)
    torch.manual_seed(0)
    ss = torch.tensor(CFG4_SHAPES, device=dev)
    lsi = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    mod = make_decoder(dev)
    out = {"B": B, "S": S, "d_model": C, "heads": M, "d_ffn": F, "Lt": LT, "layers": LAYERS, "box_head": "shared", "rounds": ROUNDS,
           "iters": args.iters, "statistic": "median of the rounds"}
    out["decoder"] = [decoder_case(mod, Lq, masked, B, S, ss, lsi, dev, args) for Lq, masked in ((900, False), (1100, True))]
    out["kernel_iters"] = args.kernel_iters
    out["kernels_alone"] = kernels_alone(B, dev, args.kernel_iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
