"""The deformable decoder layer at inference through Python, BASELINE cfg 4's decoder shape (B = 8, 900 queries -- and 1100 with a
denoising mask -- over 37 485 memory tokens per image, d_model 256, 8 heads, 4 levels, 4 points, d_ffn 2048, 256 text tokens, ReLU), both
flavours: the native call (``native_layer = True``: vllm_deform_dec_layer_forward) against the composed path of the same module on the
same tensors -- the reference's statements on torch (nn.MultiheadAttention, LayerNorm, Linear) around the fused attention call, which is
what the class runs with the switch off.  Device events, warm-up first, the two paths alternated in one process, the shader clock
sampled meanwhile (bench.py's ClockSampler).  Then the pieces alone: the attention kernel (vllm_mha_fwd_bf16) against
F.scaled_dot_product_attention on the same Q / K / V, the UniPose mirror's transposes, and where the native call's time goes
(value_proj over B S rows, the whole cross-attention call, the FFN's two GEMMs).

    python tools/bench_deform_decoder_layer.py [--iters 50] [--warmup 3] [--batch 8] [--kernel-iters 200]
"""
import argparse
import ctypes
import json
import os
import sys
import types

import torch
import torch.nn.functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench import ClockSampler  # noqa: E402
from msda_inputs import CFG4_SHAPES  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import deformable_decoder as D  # noqa: E402

C, M, P, F, LT = 256, 8, 4, 2048, 256


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


def make_layer(flavour, dev):
    L = len(CFG4_SHAPES)
    if flavour == "unipose":
        m = D.DeformableTransformerDecoderLayer(d_model=C, d_ffn=F, activation="relu", n_levels=L, n_heads=M, n_points=P,
                                                use_text_cross_attention=True)
    else:
        cfg = types.SimpleNamespace(d_model=C, num_feature_levels=L, decoder_attention_heads=M, decoder_n_points=P, decoder_ffn_dim=F,
                                    dropout=0.1, attention_dropout=0.0, activation_function="relu", activation_dropout=0.0,
                                    disable_custom_kernels=False)
        m = D.GroundingDinoDecoderLayer(cfg)
    with torch.no_grad():
        (m.cross_attn if flavour == "unipose" else m.encoder_attn).sampling_offsets.weight.normal_(0, 0.01)
    return m.to(dev).to(torch.bfloat16).eval()


def denoise_mask(Lq, dn, dev):
    """bool [Lq, Lq], True = may NOT attend: `dn` denoising rows in two groups in front of the matching queries"""
    m = torch.zeros(Lq, Lq, dtype=torch.bool, device=dev)
    half = dn // 2
    m[dn:, :dn] = True
    m[:half, half:dn] = True
    m[half:dn, :half] = True
    return m


def clocked(fns, iters, dev):
    """three alternated rounds of `iters` calls of every function -> ({name: [us]}, clocks)"""
    times = {k: [] for k in fns}
    clk = ClockSampler(dev)
    sampled = clk.has_sysfs()
    if sampled:
        clk.start()
    for _ in range(3):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    clocks = clk.stop() if sampled else None
    return times, (clocks if clocks else "no amdgpu hwmon files readable: clock not sampled")


def layer_case(flavour, Lq, masked, B, S, ss, lsi, dev, args):
    lib = _lib.lib()
    mod = make_layer(flavour, dev)
    L = len(CFG4_SHAPES)
    bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    tgt, pos, memory, text = bf(B, Lq, C), bf(B, Lq, C) * 0.5, bf(B, S, C), bf(B, LT, C)
    ref = torch.cat([torch.rand(B, Lq, L, 2, device=dev), 0.05 + 0.3 * torch.rand(B, Lq, L, 2, device=dev)], -1)
    sam = denoise_mask(Lq, Lq - 900, dev) if masked else None
    tmask = torch.zeros(B, LT, dtype=torch.bool, device=dev)
    for b in range(B):
        tmask[b, LT - 16 * (b + 1):] = True
    if flavour == "unipose":   # the model's own layout: sequence-first, contiguous
        tgt_s, pos_s, ref_s, mem_s = (x.transpose(0, 1).contiguous() for x in (tgt, pos, ref, memory))

    def run(flag):
        def fn():
            type(mod).native_layer = flag
            with torch.no_grad():
                if flavour == "unipose":
                    return mod(tgt_s, pos_s, None, None, ref_s, text, tmask, mem_s, None, lsi, ss, None, sam, None)
                return mod(tgt, pos, ref, ss, lsi, memory, None, text, tmask, sam)[0]
        return fn
    paths = {"native": run(True), "composed": run(False)}
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    calls = lib.vllm_deform_dec_layer_calls()
    a, b = paths["native"]().float(), paths["composed"]().float()
    assert lib.vllm_deform_dec_layer_calls() == calls + 1, "the native path did not run"
    rel = ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    del a, b
    times, clocks = clocked(paths, args.iters, dev)
    type(mod).native_layer = False
    rec = {"Lq": Lq, "denoising_mask": bool(masked), "clocks": clocks, "native_vs_composed_rel_rms": round(rel, 5)}
    for k, v in times.items():
        rec[k + "_us"] = round(min(v), 1)
        rec[k + "_all_us"] = [round(t, 1) for t in v]
    rec["native_over_composed"] = round(min(times["native"]) / min(times["composed"]), 3)
    rec["aim_native_le_composed"] = "met" if rec["native_over_composed"] <= 1.0 else "not met"
    if flavour == "unipose":
        # what the mirror pays for the batch-first entry: tgt, pos, the reference points in, the result out -- and the memory, which the
        # composed path's attention module copies as well
        small = lambda: (tgt_s.transpose(0, 1).contiguous(), pos_s.transpose(0, 1).contiguous(),
                         ref_s.transpose(0, 1).contiguous(), tgt.transpose(0, 1).contiguous())
        times, clocks = clocked({"transposes_tgt_pos_ref_out": small, "transpose_memory": lambda: mem_s.transpose(0, 1).contiguous()},
                                args.iters, dev)
        rec["unipose_transposes"] = {"clocks": clocks, **{k + "_us": round(min(v), 1) for k, v in times.items()}}
    del mod
    torch.cuda.empty_cache()
    return rec


def mha_alone(B, dev, iters):
    """vllm_mha_fwd_bf16 on column slices of packed projection outputs against F.scaled_dot_product_attention on the same Q / K / V"""
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    Dh = C // M
    out = {}
    for name, Lq, Lk, kind in (("self_900", 900, 900, None), ("self_1100_denoising_mask", 1100, 1100, "attn"),
                               ("text_900x256_padding_mask", 900, LT, "kpm"), ("text_1100x256_padding_mask", 1100, LT, "kpm")):
        qk = torch.randn(B, Lq, 2 * C, device=dev).to(torch.bfloat16)
        kv = qk if Lk == Lq else torch.randn(B, Lk, 2 * C, device=dev).to(torch.bfloat16)
        q, k = qk[:, :, :C], kv[:, :, C:] if Lk == Lq else kv[:, :, :C]
        v = torch.randn(B, Lk, C, device=dev).to(torch.bfloat16) if Lk == Lq else kv[:, :, C:]
        am = denoise_mask(Lq, Lq - 900, dev) if kind == "attn" else None
        kp = None
        if kind == "kpm":
            kp = torch.zeros(B, Lk, dtype=torch.bool, device=dev)
            for b in range(B):
                kp[b, Lk - 16 * (b + 1):] = True
        am8, kp8 = (None if m is None else m.to(torch.uint8) for m in (am, kp))
        o = torch.empty(B, Lq, C, dtype=torch.bfloat16, device=dev)
        native = lambda: _lib.check(lib.vllm_mha_fwd_bf16(PT(q), q.stride(0), q.stride(1), PT(k), k.stride(0), k.stride(1), PT(v), v.stride(0),
                                                          v.stride(1), PT(o), o.stride(0), o.stride(1), PT(am8), PT(kp8), B, Lq, Lk, M, Dh,
                                                          Dh ** -0.5, st))
        heads = lambda x, L: x.reshape(B, L, M, Dh).transpose(1, 2)
        qh, kh, vh = heads(q, Lq), heads(k, Lk), heads(v, Lk)
        allowed = None if am is None and kp is None else ~am[None, None] if am is not None else ~kp[:, None, None, :]
        sdpa = lambda: F_.scaled_dot_product_attention(qh, kh, vh, attn_mask=allowed)
        native()
        ref = sdpa().transpose(1, 2).reshape(B, Lq, C).float()
        rel = ((o.float() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
        times, clocks = clocked({"native": native, "sdpa": sdpa}, iters, dev)
        out[name] = {"clocks": clocks, "native_us": round(min(times["native"]), 1), "sdpa_us": round(min(times["sdpa"]), 1),
                     "native_over_sdpa": round(min(times["native"]) / min(times["sdpa"]), 3), "rel_rms_vs_sdpa": round(rel, 5)}
    return out


def pieces(B, S, ss, lsi, dev, iters):
    """where the native call's time goes at Lq = 900: the cross-attention call alone (value_proj over B S rows inside it), value_proj
    alone, the FFN's GEMMs, and the shapes of the six projection GEMMs of the two attention blocks (N = 2C and N = C over the B Lq query
    rows: [q | k]; v, the text's q and the two out_proj; N = 2C over the B Lt text rows: the text's [k | v])"""
    lib = _lib.lib()
    st = _lib.current_stream(dev)
    Lq, L = 900, len(CFG4_SHAPES)
    R = B * Lq
    bf = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
    mod = make_layer("unipose", dev)
    q, memory = bf(B, Lq, C), bf(B, S, C)
    ref = torch.cat([torch.rand(B, Lq, L, 2, device=dev), 0.05 + 0.3 * torch.rand(B, Lq, L, 2, device=dev)], -1)
    x, w, bias, w1, b1, w2 = bf(R, C), bf(C, C) / 16, bf(C), bf(F, C) / 16, bf(F), bf(C, F) / 45
    w3 = bf(2 * C, C) / 16
    b3 = bf(2 * C)
    y, y2, h = (torch.empty(R, n, dtype=torch.bfloat16, device=dev) for n in (C, 2 * C, F))
    text, tkv = bf(B * LT, C), torch.empty(B * LT, 2 * C, dtype=torch.bfloat16, device=dev)
    val = torch.empty(B * S, C, dtype=torch.bfloat16, device=dev)
    ck = _lib.check
    with torch.no_grad():
        fns = {
            "cross_attn_call": lambda: mod.cross_attn(q, ref, memory, ss, lsi, None),
            "value_proj_gemm_B_S_rows": lambda: ck(lib.vllm_gemm_bf16(PT(memory), PT(w), PT(bias), PT(val), B * S, C, C, C, C, C, _lib.EPI_BIAS, None,
                                                                      None, 0, 0, st)),
            "fc1_relu": lambda: ck(lib.vllm_gemm_bf16_relu(PT(x), PT(w1), PT(b1), PT(h), R, F, C, C, C, F, 0, st)),
            "fc2_residual": lambda: ck(lib.vllm_gemm_bf16(PT(h), PT(w2), PT(bias), PT(y), R, C, F, F, F, C, _lib.EPI_RESIDUAL, None, PT(x), C, 0, st)),
            "proj_gemm_N_2C": lambda: ck(lib.vllm_gemm_bf16(PT(x), PT(w3), PT(b3), PT(y2), R, 2 * C, C, C, C, 2 * C, _lib.EPI_BIAS, None, None, 0, 0, st)),
            "text_kv_gemm_B_Lt_rows_N_2C": lambda: ck(lib.vllm_gemm_bf16(PT(text), PT(w3), PT(b3), PT(tkv), B * LT, 2 * C, C, C, C, 2 * C, _lib.EPI_BIAS, None,
                                                                        None, 0, 0, st)),
            "proj_gemm_N_C": lambda: ck(lib.vllm_gemm_bf16(PT(x), PT(w), PT(bias), PT(y), R, C, C, C, C, C, _lib.EPI_BIAS, None, None, 0, 0, st)),
            "add_layernorm_with_pos_out": lambda: ck(lib.vllm_add_layernorm_bf16(PT(x), C, None, 0, PT(bias), PT(bias), PT(y), C, PT(x), C, PT(val), C, R,
                                                                                 C, 1e-5, st)),
        }
        for fn in fns.values():
            for _ in range(3):
                fn()
        times, clocks = clocked(fns, iters, dev)
    return {"clocks": clocks, **{k + "_us": round(min(v), 1) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--kernel-iters", type=int, default=200, help="calls per timing of the kernels alone: they take 6-130 us, and a timing "
                    "must last several periods of the 20 ms clock sampler for its median clock to mean something")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deform_decoder_layer: no GPU -- nothing is measured without one")
    dev = torch.device("cuda:0")
    B = args.batch
    S = sum(h * w for h, w in CFG4_SHAPES)
    torch.manual_seed(0)
    ss = torch.tensor(CFG4_SHAPES, device=dev)
    lsi = torch.cat([ss.new_zeros(1), (ss[:, 0] * ss[:, 1]).cumsum(0)[:-1]])
    out = {"B": B, "S": S, "d_model": C, "heads": M, "d_ffn": F, "Lt": LT, "activation": "relu", "ref_dim": 4}
    for flavour in ("unipose", "gdino"):
        out[flavour] = [layer_case(flavour, Lq, masked, B, S, ss, lsi, dev, args) for Lq, masked in ((900, False), (1100, True))]
    out["kernel_iters"] = args.kernel_iters
    out["mha_alone"] = mha_alone(B, dev, args.kernel_iters)
    out["pieces_alone_Lq_900"] = pieces(B, S, ss, lsi, dev, args.kernel_iters)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
