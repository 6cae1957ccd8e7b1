"""The Grounding-DINO encoder at inference through Python, BASELINE cfg 4's encoder shape (B = 8, 37 485 image tokens per image in 4
levels, d_model 256, 8 heads -- 4 for the enhancer and the fusion layer --, 4 points, d_ffn 2048, 256 text tokens in ragged phrases,
6 layers), three paths on the same module and tensors:
  (a) ``native_encoder = True``: ONE vllm_gdino_encoder_forward;
  (b) the switch off, ``native_layer = True`` on every fusion and deformable layer, the text enhancer composed: the best the encoder
      could do before the enhancer and the loop became native -- the baseline;
  (c) everything composed.
Device events, warm-up first, the paths alternated in one process over five rounds, medians reported, the shader clock sampled meanwhile
(bench.py's ClockSampler).  Then the text enhancer alone, native against composed, and the three new kernels alone
(vllm_mha_fwd_masks_bf16, vllm_text_pos_embed_bf16, vllm_encoder_refpoints_f32).  Recorded, not gated.

    python tools/bench_gdino_encoder.py [--iters 5] [--warmup 2] [--batch 8] [--kernel-iters 300] [--skip-composed]
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
from visionllm_amd import gdino_encoder as G  # noqa: E402
from visionllm_amd.deformable_encoder import GroundingDinoDeformableLayer  # noqa: E402
from visionllm_amd.fusion_layer import GroundingDinoFusionLayer  # noqa: E402

C, HEADS, P, F, LT, LAYERS = 256, 8, 4, 2048, 256, 6
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
    rec = {}
    for k, v in times.items():
        rec[k + "_median_us"] = round(statistics.median(v), 1)
        rec[k + "_all_us"] = [round(t, 1) for t in v]
    return rec


def make_encoder(dev):
    cfg = types.SimpleNamespace(d_model=C, encoder_ffn_dim=F, encoder_attention_heads=HEADS, fusion_dropout=0.0, fusion_droppath=0.1,
                                text_enhancer_dropout=0.0, activation_function="relu", num_feature_levels=len(CFG4_SHAPES), encoder_n_points=P,
                                dropout=0.1, activation_dropout=0.0, disable_custom_kernels=False, encoder_layers=LAYERS, use_return_dict=False)
    m = G.GroundingDinoEncoder(cfg)
    with torch.no_grad():
        for layer in m.layers:
            layer.deformable_layer.self_attn.sampling_offsets.weight.normal_(0, 0.01)
            layer.fusion_layer.vision_param.fill_(0.1)
            layer.fusion_layer.text_param.fill_(0.1)
    return m.to(dev).to(torch.bfloat16).eval()


def text_masks(B, dev):
    """phrases of 3 .. 17 tokens, different per image; the last 16 (b + 1) tokens of image b are padding, which sees itself only"""
    allowed = torch.zeros(B, LT, LT, dtype=torch.bool)
    ids = torch.zeros(B, LT, dtype=torch.int64)
    pad = torch.zeros(B, LT, dtype=torch.bool)
    for b in range(B):
        real = LT - 16 * (b + 1)
        lo, k = 0, 0
        while lo < real:
            hi = min(real, lo + 3 + (5 * b + 7 * k) % 15)
            allowed[b, lo:hi, lo:hi] = True
            ids[b, lo:hi] = torch.arange(hi - lo)
            lo, k = hi, k + 1
        pad[b, real:] = True
        idx = torch.arange(real, LT)
        allowed[b, idx, idx] = True
    return allowed.to(dev), ids.to(dev), pad.to(dev)


def set_switches(encoder, members, enhancer):
    G.GroundingDinoEncoder.native_encoder = encoder
    GroundingDinoFusionLayer.native_layer = members
    GroundingDinoDeformableLayer.native_layer = members
    G.GroundingDinoTextEnhancerLayer.native_layer = enhancer


def encoder_case(mod, B, S, ss, lsi, dev, args):
    lib = _lib.lib()
    L = len(CFG4_SHAPES)
    bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    vision, vpos, text = bf(B, S, C), bf(B, S, C), bf(B, LT, C)
    vr = 1.0 - 0.3 * torch.rand(B, L, 2, device=dev)
    vmask = torch.zeros(B, S, dtype=torch.bool, device=dev)
    for b in range(B):
        vmask[b, S - 1000 * b:] = b > 0
    allowed, ids, tpad = text_masks(B, dev)

    def run(*switches):
        def fn():
            set_switches(*switches)
            with torch.no_grad():
                return mod(vision, vmask, vpos, ss, lsi, vr, text, tpad, None, allowed, ids)
        return fn
    paths = {"a_native_encoder": run(True, False, False), "b_members_native_enhancer_composed": run(False, True, False)}
    if not args.skip_composed:
        paths["c_all_composed"] = run(False, False, False)
    try:
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        n0 = (lib.vllm_gdino_encoder_calls(), lib.vllm_fusion_layer_calls(), lib.vllm_deform_enc_layer_calls(), lib.vllm_text_enhancer_calls())
        a = paths["a_native_encoder"]()
        n1 = (lib.vllm_gdino_encoder_calls(), lib.vllm_fusion_layer_calls(), lib.vllm_deform_enc_layer_calls(), lib.vllm_text_enhancer_calls())
        assert n1 == (n0[0] + 1, n0[1], n0[2], n0[3]), "the native path did not run"
        b = paths["b_members_native_enhancer_composed"]()
        n2 = (lib.vllm_gdino_encoder_calls(), lib.vllm_fusion_layer_calls(), lib.vllm_deform_enc_layer_calls(), lib.vllm_text_enhancer_calls())
        assert n2 == (n1[0], n1[1] + LAYERS, n1[2] + LAYERS, n1[3]), "the baseline did not run the members' native calls"
        rel = lambda x, y: round(((x.float() - y.float()).pow(2).mean().sqrt() / y.float().pow(2).mean().sqrt()).item(), 5)
        agree = {"vision_rel_rms": rel(a[0], b[0]), "text_rel_rms": rel(a[1], b[1])}
        del a, b
        times, clocks = clocked(paths, args.iters, dev)
    finally:
        set_switches(False, False, False)
    rec = {"clocks": clocks, "a_vs_b": agree}
    rec.update(summary(times))
    med = lambda k: statistics.median(times[k])
    rec["a_over_b"] = round(med("a_native_encoder") / med("b_members_native_enhancer_composed"), 3)
    rec["b_minus_a_us"] = round(med("b_members_native_enhancer_composed") - med("a_native_encoder"), 1)
    rec["b_minus_a_per_layer_us"] = round(rec["b_minus_a_us"] / LAYERS, 1)
    if not args.skip_composed:
        rec["a_over_c"] = round(med("a_native_encoder") / med("c_all_composed"), 3)
    rec["aim_a_le_b"] = "met" if med("a_native_encoder") <= med("b_members_native_enhancer_composed") else "not met"
    return rec


def enhancer_case(mod, B, dev, args):
    e = mod.layers[0].text_enhancer_layer
    text = torch.randn(B, LT, C, device=dev).to(torch.bfloat16)
    pos = torch.randn(B, LT, C, device=dev).to(torch.bfloat16)
    allowed, _, _ = text_masks(B, dev)
    mask = ~allowed

    def run(flag):
        def fn():
            G.GroundingDinoTextEnhancerLayer.native_layer = flag
            with torch.no_grad():
                return e(text, mask, pos)[0]
        return fn
    paths = {"native": run(True), "composed": run(False)}
    try:
        for _ in range(3):
            for fn in paths.values():
                fn()
        times, clocks = clocked(paths, args.kernel_iters // 3 or 1, dev)
    finally:
        G.GroundingDinoTextEnhancerLayer.native_layer = False
    rec = {"rows": B * LT, "clocks": clocks}
    rec.update(summary(times))
    rec["native_over_composed"] = round(statistics.median(times["native"]) / statistics.median(times["composed"]), 3)
    return rec


def kernels_alone(B, S, ss, lsi, dev, iters):
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    ck = _lib.check
    L, H, D = len(CFG4_SHAPES), HEADS // 2, C // (HEADS // 2)
    qkv = torch.randn(B, LT, 3 * C, device=dev).to(torch.bfloat16)
    ctx = torch.empty(B, LT, C, dtype=torch.bfloat16, device=dev)
    allowed, ids, _ = text_masks(B, dev)
    am = (~allowed).to(torch.uint8).contiguous()
    dim_t = G.sine_dim_t(C, dev).contiguous()
    posf = ids.float().contiguous()
    tpe = torch.empty(B * LT, C, dtype=torch.bfloat16, device=dev)
    vr = (1.0 - 0.3 * torch.rand(B, L, 2, device=dev)).contiguous()
    ref = torch.empty(B, S, L, 2, device=dev)
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    fns = {
        "mha_fwd_masks_n_masks_B": lambda: ck(lib.vllm_mha_fwd_masks_bf16(PT(q), LT * 3 * C, 3 * C, PT(k), LT * 3 * C, 3 * C, PT(v), LT * 3 * C, 3 * C,
                                                                          PT(ctx), LT * C, C, PT(am), B, None, B, LT, LT, H, D, D ** -0.5, st)),
        "text_pos_embed": lambda: ck(lib.vllm_text_pos_embed_bf16(PT(posf), PT(dim_t), B, LT, C, PT(tpe), C, st)),
        "encoder_refpoints": lambda: ck(lib.vllm_encoder_refpoints_f32(PT(ss), PT(lsi), PT(vr), B, S, L, PT(ref), st)),
    }
    nbytes = {"mha_fwd_masks_n_masks_B": B * LT * 4 * C * 2 + B * LT * LT, "text_pos_embed": B * LT * (4 + C * 2) + C * 4,
              "encoder_refpoints": B * S * L * 8 + B * L * 8 + L * 24}
    for fn in fns.values():
        for _ in range(3):
            fn()
    times, clocks = clocked(fns, iters, dev)
    rec = {"clocks": clocks}
    for name, t in times.items():
        us = statistics.median(t)
        rec[name] = {"median_us": round(us, 2), "all_us": [round(x, 2) for x in t], "bytes": nbytes[name],
                     "bytes_per_s": round(nbytes[name] / (us * 1e-6), 0)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=300, help="calls per timing of the kernels alone: they take microseconds, and a "
                    "timing must last several periods of the 20 ms clock sampler for its median clock to mean something")
    ap.add_argument("--skip-composed", action="store_true", help="leave path (c) out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gdino_encoder: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    B = args.batch
    S = sum(h * w for h, w in CFG4_SHAPES)
    torch.manual_seed(0)
    ss = torch.tensor(CFG4_SHAPES, device=dev)
    lsi = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    mod = make_encoder(dev)
    out = {"B": B, "S": S, "d_model": C, "heads": HEADS, "d_ffn": F, "Lt": LT, "layers": LAYERS, "rounds": ROUNDS, "iters": args.iters,
           "statistic": "median of the rounds"}
    out["encoder"] = encoder_case(mod, B, S, ss, lsi, dev, args)
    out["kernel_iters"] = args.kernel_iters
    out["enhancer_alone"] = enhancer_case(mod, B, dev, args)
    out["kernels_alone"] = kernels_alone(B, S, ss, lsi, dev, args.kernel_iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
