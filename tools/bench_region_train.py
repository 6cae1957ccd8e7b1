"""Region-encoder pooling under training (forward + backward of the masked mean of 2304 bilinear samples per region) at
16 regions x 3072 channels x 24 x 24 (README's shape) and 16 x 1024 (what ViT-L gives the model):
  (a) native: visionllm_amd.region_encoder.point_sample_masked_mean under autograd, fp32 and bf16 maps;
  (b) torch's autograd of the composed reference expression (grid_sample -> mask -> sum -> div) on the same tensors -- what the
      reference runs, independent of the code under test;
  (c) the native backward alone through the C ABI, as a share of the HBM store roof: bytes from shapes
      (N C H W sizeof(out) written + N C 4 read) over the time, against the measured float4-copy rate of 6.29 TB/s.
Device events around >= --seconds of work per timing after warm-up, the paths alternated in one process, three rounds; the minimum
and all rounds are printed.  VLLM_HIP_LIB selects another build of the library (chunk-size sweeps); --backward-only skips (a), (b).

    python tools/bench_region_train.py [--seconds 0.5] [--backward-only]
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import region_encoder as R  # noqa: E402

HBM = 6.29e12          # measured float4 copy rate of the MI355X, bytes / s
SHAPES = [("readme_3072", 16, 3072, 24, 24, 2304), ("vit_l_1024", 16, 1024, 24, 24, 2304)]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


def composed(x, c, v):
    s = F.grid_sample(x, 2.0 * c.unsqueeze(2) - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False).squeeze(3)
    feats = s.permute(0, 2, 1) * v.unsqueeze(-1)
    return (feats.sum(1) / v.sum(1).unsqueeze(-1)).nan_to_num()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--backward-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    out = {"lib": _lib.lib_path(), "hbm_roof_bytes_per_s": HBM}
    for name, N, C, H, W, P in SHAPES:
        torch.manual_seed(0)
        c = torch.rand(N, P, 2, device=dev)
        v = torch.rand(N, P, device=dev) > 0.1
        v8 = v.to(torch.uint8)
        g32 = torch.randn(N, C, device=dev)
        paths = {}
        for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            x = torch.randn(N, C, H, W, device=dev).to(dt).requires_grad_(True)
            g = g32.to(dt)
            grad_in = torch.empty(N, C, H, W, device=dev, dtype=dt)
            fn = getattr(L, "vllm_point_sample_mean_backward_" + tag)
            st = _lib.current_stream(dev)
            wsb = L.vllm_point_sample_backward_workspace_bytes(N, C, H, W, P)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)

            def bwd_only(fn=fn, grad_in=grad_in, ws=ws):
                _lib.check(fn(_lib.ptr(c), _lib.ptr(v8), _lib.ptr(g32), N, C, H, W, P, _lib.ptr(grad_in), _lib.ptr(ws), wsb, st))

            def native(x=x, g=g):
                x.grad = None
                R.point_sample_masked_mean(x, c, v).backward(g)

            def torch_ref(x=x, g=g, cc=c.to(dt)):
                x.grad = None
                composed(x, cc, v).backward(g)
            paths["native_backward_only_" + tag] = bwd_only
            if not args.backward_only:
                paths["native_fwd_bwd_" + tag] = native
                paths["torch_autograd_fwd_bwd_" + tag] = torch_ref
        iters = {}
        for k, f in list(paths.items()):    # warm-up, and the iteration count that fills --seconds
            try:
                for _ in range(3):
                    f()
            except RuntimeError as e:       # (a dtype torch's grid_sample does not take: reported, not timed)
                out.setdefault("skipped", {})[f"{name}/{k}"] = str(e)[:200]
                del paths[k]
                continue
            iters[k] = max(10, math.ceil(args.seconds * 1e6 / timed(f, 5)))
        rounds = {k: [] for k in paths}
        for _ in range(3):                  # alternated
            for k, f in paths.items():
                rounds[k].append(timed(f, iters[k]))
        res = {"shape": [N, C, H, W, P]}
        for k, t in rounds.items():
            res[k] = {"us": round(min(t), 1), "all_us": [round(u, 1) for u in t], "iters": iters[k]}
            if k.startswith("native_backward_only"):
                nbytes = N * C * H * W * (4 if k.endswith("f32") else 2) + N * C * 4
                res[k]["bytes"] = nbytes
                res[k]["share_of_hbm_store_roof"] = round(nbytes / (min(t) * 1e-6) / HBM, 3)
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
