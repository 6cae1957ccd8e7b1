"""Grounding-DINO's two-stage query selection at inference through Python, BASELINE cfg 4's shape (B = 8, 37 485 encoder rows per image over
the four maps, d_model 256, 256 text tokens, 900 queries): the native call (``native_selection = True``: vllm_query_select_forward)
against the same module with the switch off on the same tensors.  Device events, warm-up first, the two paths alternated in one process
over five rounds, medians reported, the shader clock sampled meanwhile (bench.py's ClockSampler).  Then the three new kernels alone
(vllm_rowmax_dot_bf16, vllm_topk_rows_f32, vllm_query_select_tail_f32) and the top-k kernel's share of the native call: recorded, not
gated.

    python tools/bench_query_selection.py [--iters 20] [--warmup 3] [--batch 8] [--kernel-iters 200]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import ClockSampler  # noqa: E402
from msda_inputs import CFG4_SHAPES  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import query_selection as Q  # noqa: E402

C, LT, K = 256, 256, 900
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


def real_mask(B, dev):
    """bool [B, S], True = a real cell: image b keeps the top-left (1 - b / 24) of every map (image 0 is unpadded)"""
    parts = []
    for H, W in CFG4_SHAPES:
        m = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
        for b in range(B):
            f = 1.0 - b / 24.0
            m[b, :max(1, int(H * f)), :max(1, int(W * f))] = True
        parts.append(m.flatten(1))
    return torch.cat(parts, 1)


def module_case(mod, t, args, dev):
    lib = _lib.lib()

    def run(flag):
        def fn():
            Q.GroundingDinoQuerySelection.native_selection = flag
            with torch.no_grad():
                return mod(t["memory"], t["text"], t["mask"], t["tmask"], t["shapes"], K)
        return fn
    paths = {"native": run(True), "composed": run(False)}
    try:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        calls = lib.vllm_query_select_calls()
        a = paths["native"]()
        assert lib.vllm_query_select_calls() == calls + 1, "the native path did not run"
        b = paths["composed"]()
        assert lib.vllm_query_select_calls() == calls + 1
        same = torch.stack([torch.isin(a.topk_proposals[i], b.topk_proposals[i]).float().mean() for i in range(a.topk_proposals.shape[0])])
        agree = {"fraction_of_native_indices_also_selected_by_torch_topk": round(same.mean().item(), 5)}
        del a, b
        times, clocks = clocked(paths, args.iters, dev)
    finally:
        Q.GroundingDinoQuerySelection.native_selection = False
    rec = {"clocks": clocks, "native_vs_composed": agree}
    for k, v in times.items():
        rec[k + "_median_us"] = round(statistics.median(v), 1)
        rec[k + "_all_us"] = [round(x, 1) for x in v]
    med = lambda k: statistics.median(times[k])
    rec["native_over_composed"] = round(med("native") / med("composed"), 3)
    rec["aim_native_le_composed"] = "met" if med("native") <= med("composed") else "not met"
    return rec


def kernels_alone(t, B, S, dev, iters):
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    L = len(CFG4_SHAPES)
    ck = _lib.check
    q = torch.randn(B, S, C, device=dev).to(torch.bfloat16)
    tmask = t["tmask"].to(torch.uint8)
    pmask = (~t["mask"]).to(torch.uint8)
    scores = torch.empty(B, S, device=dev)
    idx = torch.empty(B, K, dtype=torch.int64, device=dev)
    h = torch.randn(B * K, C, device=dev).relu().to(torch.bfloat16)
    W = (torch.randn(4, C, device=dev) / 16).to(torch.bfloat16)
    bias = torch.zeros(4, dtype=torch.bfloat16, device=dev)
    ext = torch.empty(B, L, 2, dtype=torch.int32, device=dev)
    coords, ref = torch.empty(B, K, 4, device=dev), torch.empty(B, K, 4, device=dev)
    hw = t["shapes"][:, 0] * t["shapes"][:, 1]
    lsi = (torch.cumsum(hw, 0) - hw).contiguous()
    fns = {
        "rowmax_dot": lambda: ck(lib.vllm_rowmax_dot_bf16(PT(q), PT(t["text"]), PT(tmask), B, S, LT, C, PT(scores), st)),
        "topk_rows": lambda: ck(lib.vllm_topk_rows_f32(PT(scores), B, S, K, PT(idx), st)),
        "tail": lambda: ck(lib.vllm_query_select_tail_f32(PT(h), C, PT(W), PT(bias), PT(idx), PT(pmask), PT(t["shapes"]), PT(lsi), B, S, L, K, C, PT(ext),
                                                          PT(coords), PT(ref), None, st)),
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    times, clocks = clocked(fns, iters, dev)
    rec = {"clocks": clocks, "rows": {"rowmax_dot": B * S, "topk_rows": f"{B} x {S} -> {K}", "tail": B * K}}
    for k, v in times.items():
        rec[k] = {"median_us": round(statistics.median(v), 2), "all_us": [round(x, 2) for x in v]}
    rec["rowmax_dot"]["tflops"] = round(2.0 * B * S * LT * C / (statistics.median(times["rowmax_dot"]) * 1e-6) / 1e12, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=200, help="calls per timing of the kernels alone: a timing must last several periods "
                    "of the 20 ms clock sampler for its median clock to mean something")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_query_selection: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    B = args.batch
    S = sum(h * w for h, w in CFG4_SHAPES)
    torch.manual_seed(0)
    mod = Q.GroundingDinoQuerySelection(C, LT)
    with torch.no_grad():
        mod.encoder_output_bbox_embed.layers[-1].weight.mul_(0.1)
    mod = mod.to(dev).to(torch.bfloat16).eval()
    tmask = torch.ones(B, LT, dtype=torch.bool, device=dev)
    for b in range(B):
        tmask[b, LT - 16 * (b + 1):] = False
    t = {"memory": torch.randn(B, S, C, device=dev).to(torch.bfloat16), "text": torch.randn(B, LT, C, device=dev).to(torch.bfloat16),
         "mask": real_mask(B, dev), "tmask": tmask, "shapes": torch.tensor(CFG4_SHAPES, device=dev)}
    out = {"B": B, "S": S, "d_model": C, "Lt": LT, "num_queries": K, "rounds": ROUNDS, "iters": args.iters, "statistic": "median of the rounds"}
    out["module"] = module_case(mod, t, args, dev)
    out["kernel_iters"] = args.kernel_iters
    out["kernels_alone"] = kernels_alone(t, B, S, dev, args.kernel_iters)
    out["topk_share_of_native_call"] = round(out["kernels_alone"]["topk_rows"]["median_us"] / out["module"]["native_median_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
