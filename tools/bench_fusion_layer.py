"""Grounding-DINO's fusion layer at inference through Python, BASELINE cfg 4's shape (B = 8, 37 485 image tokens per image, 256 text
tokens with ragged lengths, a vision padding mask, d_model 256, embed 1024 over 4 heads = head dim 256): the native call
(``native_layer = True``: vllm_fusion_layer_forward) against the same module with the switch off on the same tensors.  Device events,
warm-up first, the two paths alternated in one process over five rounds, medians reported, the shader clock sampled meanwhile (bench.py's
ClockSampler).  Then each attention direction alone (vllm_xattn_fwd_bf16) against F.scaled_dot_product_attention on the same Q / K / V,
the pieces of the native call, the workspace size, and the K / V re-reads of the long-key direction: recorded, not gated.

    python tools/bench_fusion_layer.py [--iters 10] [--warmup 2] [--batch 8] [--kernel-iters 20] [--out profiles/fusion_layer.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import ClockSampler  # noqa: E402
from msda_inputs import CFG4_SHAPES  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import fusion_layer as FL  # noqa: E402

C, LT, FFN, HEADS = 256, 256, 2048, 8          # embed = FFN / 2 = 1024, heads = HEADS / 2 = 4
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


def summary(times):
    return {k: {"median_us": round(statistics.median(v), 1), "all_us": [round(x, 1) for x in v]} for k, v in times.items()}


def vision_padding(B, dev):
    """bool [B, S], True = padded: image b keeps the top-left (1 - b / 24) of every map (image 0 is unpadded)"""
    parts = []
    for H, W in CFG4_SHAPES:
        m = torch.ones(B, H, W, dtype=torch.bool, device=dev)
        for b in range(B):
            f = 1.0 - b / 24.0
            m[b, :max(1, int(H * f)), :max(1, int(W * f))] = False
        parts.append(m.flatten(1))
    return torch.cat(parts, 1)


def module_case(mod, t, args, dev):
    lib = _lib.lib()

    def run(flag):
        def fn():
            FL.GroundingDinoFusionLayer.native_layer = flag
            with torch.no_grad():
                return mod(t["vision"], t["text"], t["vmask"], t["tmask"])
        return fn
    paths = {"native": run(True), "composed": run(False)}
    try:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        calls = lib.vllm_fusion_layer_calls()
        (nv, _), (nt, _) = paths["native"]()
        assert lib.vllm_fusion_layer_calls() == calls + 1, "the native path did not run"
        (cv, _), (ct, _) = paths["composed"]()
        assert lib.vllm_fusion_layer_calls() == calls + 1
        rel = lambda a, b: ((a.float() - b.float()).pow(2).mean().sqrt() / b.float().pow(2).mean().sqrt()).item()
        agree = {"rel_rms_native_vs_composed_vision": round(rel(nv, cv), 5), "rel_rms_native_vs_composed_text": round(rel(nt, ct), 5)}
        del nv, nt, cv, ct
        times, clocks = clocked(paths, args.iters, dev)
    finally:
        FL.GroundingDinoFusionLayer.native_layer = False
    rec = {"clocks": clocks, "native_vs_composed": agree}
    for k, v in times.items():
        rec[k + "_median_us"] = round(statistics.median(v), 1)
        rec[k + "_all_us"] = [round(x, 1) for x in v]
    med = lambda k: statistics.median(times[k])
    rec["native_over_composed"] = round(med("native") / med("composed"), 3)
    rec["aim_native_le_composed"] = "met" if med("native") <= med("composed") else "not met"
    return rec


def pieces(mod, t, B, S, dev, iters):
    """every launch of the native call through the C entries, on the tensors the call would form, and each attention direction against
    F.scaled_dot_product_attention on the same Q / K / V"""
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    ck = _lib.check
    a = mod.attn
    E, H, D = a.embed_dim, a.num_heads, a.head_dim
    bf = dict(dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        vn, tn = mod.layer_norm_vision(t["vision"]), mod.layer_norm_text(t["text"])
        qv, vv, kt, vt = a.vision_proj(vn), a.values_vision_proj(vn), a.text_proj(tn), a.values_text_proj(tn)
    av, at = torch.empty(B, S, E, **bf), torch.empty(B, LT, E, **bf)
    ov, ot = torch.empty(B, S, C, **bf), torch.empty(B, LT, C, **bf)
    y_v, y_t = torch.empty(B, S, E, **bf), torch.empty(B, LT, E, **bf)
    vm8, tm8 = t["vmask"].to(torch.uint8).contiguous(), t["tmask"].to(torch.uint8).contiguous()
    need = lib.vllm_xattn_workspace_bytes(B, LT, S, H, D)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    scale = D ** -0.5

    def ln(x, m, y, rows):
        return lambda: ck(lib.vllm_layernorm_bf16(PT(x), C, PT(m.weight), PT(m.bias), PT(y), C, rows, C, m.eps, st))

    def gemm(x, lin, y, M, N, K, epi=_lib.EPI_BIAS, scale_=None, res=None):
        return lambda: ck(lib.vllm_gemm_bf16(PT(x), PT(lin.weight), PT(lin.bias), PT(y), M, N, K, K, K, N, epi, PT(scale_), PT(res), N if res is not None else 0,
                                             0, st))

    def xattn(q, k, v, out, mask, Lq, Lk, w, wb):
        return lambda: ck(lib.vllm_xattn_fwd_bf16(PT(q), Lq * E, E, PT(k), Lk * E, E, PT(v), Lk * E, E, PT(out), Lq * E, E, PT(mask), B, Lq, Lk, H, D,
                                                  scale, PT(w), wb, st))

    heads = lambda x: x.view(B, -1, H, D).transpose(1, 2)
    tmask_add = t["tmask"][:, None, None, :].logical_not()          # SDPA's bool mask: True = attend
    vmask_add = t["vmask"][:, None, None, :].logical_not()

    def sdpa(q, k, v, m):
        def fn():
            with torch.no_grad():
                return F.scaled_dot_product_attention(heads(q), heads(k), heads(v), attn_mask=m)
        return fn
    vnd, tnd = vn.detach(), tn.detach()
    fns = {
        "layer_norm_vision": ln(t["vision"], mod.layer_norm_vision, ov, B * S),
        "layer_norm_text": ln(t["text"], mod.layer_norm_text, ot, B * LT),
        "vision_proj": gemm(vnd, a.vision_proj, y_v, B * S, E, C),
        "values_vision_proj": gemm(vnd, a.values_vision_proj, y_v, B * S, E, C),
        "text_proj": gemm(tnd, a.text_proj, y_t, B * LT, E, C),
        "values_text_proj": gemm(tnd, a.values_text_proj, y_t, B * LT, E, C),
        "xattn_text_to_image": xattn(kt, qv, vv, at, vm8, LT, S, ws, need),
        "xattn_image_to_text": xattn(qv, kt, vt, av, tm8, S, LT, None, 0),
        "out_vision_proj": gemm(av, a.out_vision_proj, ov, B * S, C, E, _lib.EPI_RESIDUAL, mod.vision_param, vnd),
        "out_text_proj": gemm(at, a.out_text_proj, ot, B * LT, C, E, _lib.EPI_RESIDUAL, mod.text_param, tnd),
        "sdpa_text_to_image": sdpa(kt, qv, vv, vmask_add),
        "sdpa_image_to_text": sdpa(qv, kt, vt, tmask_add),
    }
    refused = {}
    for k in [k for k in fns if k.startswith("sdpa")]:          # a torch build may have no kernel for head dim 256: recorded, not fatal
        try:
            fns[k]()
            torch.cuda.synchronize()
        except RuntimeError as e:
            refused[k] = str(e).splitlines()[0][:200]
            del fns[k]
    for fn in fns.values():
        for _ in range(2):
            fn()
    times, clocks = clocked(fns, iters, dev)
    rec = {"clocks": clocks, "sdpa_refused": refused}
    rec.update(summary(times))
    med = lambda k: statistics.median(times[k])
    native = [k for k in fns if not k.startswith("sdpa")]
    rec["sum_of_native_pieces_us"] = round(sum(med(k) for k in native), 1)
    for d in ("text_to_image", "image_to_text"):
        if "sdpa_" + d in times:
            rec[f"xattn_over_sdpa_{d}"] = round(med("xattn_" + d) / med("sdpa_" + d), 3)
    # the long-key direction: every query block of an (image, head, split) walks that split's K and V; Lt = 256 is four query blocks
    s, kps = ctypes.c_int(), ctypes.c_int()
    ck(lib.vllm_xattn_plan(B, LT, S, H, D, ctypes.byref(s), ctypes.byref(kps)))
    nqb = (LT + 63) // 64
    kv_once = 2 * B * H * S * D * 2
    rec["long_key_direction"] = {
        "splits": s.value, "keys_per_split": kps.value, "workgroups": B * H * nqb * s.value, "query_blocks_per_image_head": nqb,
        "kv_bytes_once": kv_once, "kv_bytes_requested": kv_once * nqb, "share_of_requested_kv_bytes_that_are_re_reads": round(1 - 1 / nqb, 3),
        "requested_kv_gb_per_s": round(kv_once * nqb / (med("xattn_text_to_image") * 1e-6) / 1e9, 1),
        "partials_workspace_bytes": need,
        "tflops": round(4.0 * B * H * LT * S * D / (med("xattn_text_to_image") * 1e-6) / 1e12, 1),
    }
    rec["short_key_direction"] = {"tflops": round(4.0 * B * H * LT * S * D / (med("xattn_image_to_text") * 1e-6) / 1e12, 1)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fusion_layer: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    B = args.batch
    S = sum(h * w for h, w in CFG4_SHAPES)
    torch.manual_seed(0)
    cfg = types.SimpleNamespace(d_model=C, encoder_ffn_dim=FFN, encoder_attention_heads=HEADS, fusion_dropout=0.0, fusion_droppath=0.0)
    mod = FL.GroundingDinoFusionLayer(cfg)
    with torch.no_grad():
        for lin in (mod.attn.vision_proj, mod.attn.text_proj):          # scores with a standard deviation near 2, as a trained layer's
            lin.weight.mul_(2.45)
        mod.vision_param.uniform_(0.5, 1.5)
        mod.text_param.uniform_(0.5, 1.5)
    mod = mod.to(dev).to(torch.bfloat16).eval()
    tmask = torch.zeros(B, LT, dtype=torch.bool, device=dev)
    for b in range(B):
        tmask[b, LT - 16 * (b + 1):] = True          # ragged text lengths: 240 .. 128 real tokens
    t = {"vision": torch.randn(B, S, C, device=dev).to(torch.bfloat16), "text": torch.randn(B, LT, C, device=dev).to(torch.bfloat16),
         "vmask": vision_padding(B, dev), "tmask": tmask}
    d = mod._fill_desc([])
    out = {"B": B, "S": S, "d_model": C, "Lt": LT, "embed_dim": FFN // 2, "heads": HEADS // 2, "rounds": ROUNDS, "iters": args.iters,
           "statistic": "median of the rounds",
           "workspace_bytes": _lib.lib().vllm_fusion_layer_workspace_bytes(ctypes.byref(d), B, S, LT)}
    out["module"] = module_case(mod, t, args, dev)
    out["kernel_iters"] = args.kernel_iters
    out["pieces"] = pieces(mod, t, B, S, dev, args.kernel_iters)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
