"""The embeddings of the vision tower, training step (forward + backward): the native path (vllm_vit_embed_forward /
vllm_vit_embed_backward behind InternVisionEmbeddings.forward) against torch's own bf16 autograd of the reference's statements
(tests/embed_train_inputs.py: ``embeddings`` -- F.conv2d, cat, + pos) on the same tensors.  Device events, warm-up first, the two paths
alternated in one process, the shader clock sampled meanwhile (bench.py's ClockSampler).  Also the tile-sum kernel alone (fraction of
the 6.29 TB/s copy rate the README uses), the weight-gradient launch alone (fraction of the 2.5 PFLOP/s bf16 MFMA peak) and the
backward's two halves through the C entry.

    python tools/bench_embed_train.py [--iters 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import embed_train_inputs as E  # noqa: E402
from bench import ClockSampler  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd.intern_vit import InternVisionConfig, InternVisionEmbeddings  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s (read + write), README
MFMA_PEAK = 2.5e15    # bf16 FLOP / s, README
# (name, tiles, image, patch, hidden)
SHAPES = [("internvit_6b", 40, 448, 14, 3200), ("vit_l_336", 40, 336, 14, 1024)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    L = _lib.lib()
    st = _lib.current_stream(torch.device(dev))
    out = {"device": torch.cuda.get_device_name(0)}
    for name, n, image, patch, C in SHAPES:
        c = E.make_case(n, image, patch, C, True, torch.bfloat16, device=dev)
        cfg = InternVisionConfig(hidden_size=C, num_attention_heads=C // 128, intermediate_size=4 * C, num_hidden_layers=1, image_size=image,
                                 patch_size=patch)
        emb = InternVisionEmbeddings(cfg).to(dev).to(torch.bfloat16)
        with torch.no_grad():
            emb.patch_embedding.weight.copy_(c["w"])
            emb.patch_embedding.bias.copy_(c["b"])
            emb.class_embedding.copy_(c["cls"])
            emb.position_embedding.copy_(c["pos"])
        pix, g = c["pix"], c["gout"]
        tp = {k: c[k].clone().requires_grad_(True) for k in ("w", "b", "cls", "pos")}

        def native():
            emb.zero_grad(set_to_none=True)
            emb(pix).backward(g)

        def native_fwd():
            with torch.no_grad():
                emb(pix)

        def torch_bf16():
            for v in tp.values():
                v.grad = None
            E.embeddings(pix, tp["w"], tp["b"], tp["cls"], tp["pos"], patch).backward(g)
        paths = {"native": native, "torch_bf16": torch_bf16, "native_forward_only": native_fwd}
        for _ in range(args.warmup):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in paths}
        clk = ClockSampler(dev)   # the shader clock while the timed paths run (bench.py's sampler)
        sampled = clk.has_sysfs()
        if sampled:
            clk.start()
        for _ in range(3):   # alternated
            for k, fn in paths.items():
                times[k].append(timed(fn, args.iters))
        clocks = clk.stop() if sampled else None
        S, kpad, K = (image // patch) ** 2 + 1, E.kpad_for(patch), 3 * patch * patch
        M = n * S
        rec = {"tiles": n, "rows": M, "hidden": C, "image": image, "kpad": kpad}
        for k, v in times.items():
            rec[k + "_us"] = round(min(v), 1)
            rec[k + "_all_us"] = [round(t, 1) for t in v]
        rec["native_over_torch"] = round(min(times["native"]) / min(times["torch_bf16"]), 3)
        # the pieces of the backward through the C entry, on the same tensors
        d = _lib.VllmVitEmbed(hidden=C, patch=patch, image=image, pixel_is_f32=0, patch_w=c["w"].data_ptr(), patch_b=c["b"].data_ptr(),
                              cls=c["cls"].data_ptr(), pos=c["pos"].data_ptr())
        wsb = L.vllm_vit_embed_workspace_bytes(ctypes.byref(d), n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        gw, gb, gc, gp = (torch.empty_like(c[k]) for k in ("w", "b", "cls", "pos"))

        def bwd(*ptrs):
            return lambda: _lib.check(L.vllm_vit_embed_backward(ctypes.byref(d), P(pix), n, P(g), *ptrs, P(ws), wsb, st), "vllm_vit_embed_backward")
        col = torch.randn(M, kpad, device=dev).to(torch.bfloat16)
        dw = torch.empty(C, kpad, device=dev, dtype=torch.bfloat16)
        wgb = max(L.vllm_gemm_wgrad_workspace_bytes(M, C, kpad), 16)
        wgws = torch.empty(wgb, dtype=torch.uint8, device=dev)

        def wgrad():
            _lib.check(L.vllm_gemm_wgrad_bf16(P(g), C, P(col), kpad, M, C, kpad, P(dw), kpad, None, P(wgws), wgb, st), "vllm_gemm_wgrad_bf16")
        sum_bytes = M * C * 2 + S * C * 2 + C * 2
        flops = 2.0 * M * C * kpad
        pieces = (("tile_sum_kernel_alone", bwd(None, None, P(gc), P(gp)), sum_bytes, None),          # one launch: grad_pos + grad_cls
                  ("tile_sum_with_bias_reduce", bwd(None, P(gb), P(gc), P(gp)), sum_bytes + C * 2, None),
                  ("weight_gradient_launch_alone", wgrad, None, flops),                               # gemm_wgrad (+ its fixed-order reduce)
                  ("grad_patch_w_only", bwd(P(gw), None, None, None), None, flops),                   # im2col + gemm_wgrad + unpad
                  ("backward_all_four", bwd(P(gw), P(gb), P(gc), P(gp)), None, None))
        for nm, fn, nbytes, fl in pieces:
            for _ in range(3):
                fn()
            us = min(timed(fn, args.iters) for _ in range(3))
            r = {"us": round(us, 1)}
            if nbytes:
                r.update(bytes=nbytes, frac_copy_rate=round(nbytes / (us * 1e-6) / COPY_RATE, 3))
            if fl:
                r.update(flop=fl, frac_mfma_peak=round(fl / (us * 1e-6) / MFMA_PEAK, 3))
            rec[nm] = r
        rec["im2col_bytes_rebuilt"] = M * kpad * 2
        rec["clocks"] = clocks if clocks else "no amdgpu hwmon files readable: clock not sampled"
        out[name] = rec
        del emb, c, tp, col, ws
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
