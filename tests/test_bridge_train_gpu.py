"""GPU: training the projector (vl_bridge) through forward(x) -- the call modeling_visionllmv2.py:579 makes with grad on a frozen
input.  Native backward (gemm_wgrad.hip, the EPI_GELU_BWD epilogue, the LayerNorm backward) against torch fp64 autograd of the SAME
module on the same bf16 parameters, input and grad_output, judged by DESIGN section 5's assembled-bf16 rule against torch's own bf16
autograd (nn.Sequential.forward / nn.Linear.forward): relative rms <= 1.25x torch's, worst element <= 2x torch's.  The building
blocks against fp64 with the GEMM tests' per-element bound."""
import copy
import ctypes
import math

import pytest
import torch
from torch import nn

from bounds import P, assert_bound, stream
from visionllm_amd import _lib
from visionllm_amd.bridge import build_vl_bridge

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ["linear", "mlp2x_gelu", "mlp3x_gelu", "internvl_mlp"]


def make_bridge(kind, cin, cout, bias=True, seed=0):
    torch.manual_seed(seed)
    br = build_vl_bridge(kind, cin, cout)
    with torch.no_grad():
        for m in br.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.normal_(1.0, 0.1)
                m.bias.normal_(0.0, 0.1)
            elif isinstance(m, nn.Linear):
                m.bias.normal_(0.0, 0.1)
                if not bias:
                    m.bias = None
    return br.to(DEV).to(torch.bfloat16)


def torch_grads(br, x, gout, dtype, need_x):
    """gradients of the same module by torch's own autograd in `dtype` (nn.Linear / nn.Sequential forward, not ours)"""
    m = copy.deepcopy(br).to(dtype)
    xx = x.detach().to(dtype).requires_grad_(need_x)
    fwd = nn.Linear.forward if isinstance(m, nn.Linear) else nn.Sequential.forward
    y = fwd(m, xx)
    y.backward(gout.to(dtype))
    return y, {n: p.grad for n, p in m.named_parameters()}, xx.grad


def native_grads(br, x, gout, need_x):
    for p in br.parameters():
        p.grad = None
    xx = x.detach().requires_grad_(need_x)   # (same storage and offset as x)
    y = br(xx)
    y.backward(gout)
    return y, {n: p.grad.clone() for n, p in br.named_parameters()}, xx.grad


def assert_rule(nat, t16, t64, what):
    t64 = t64.double()
    en, et = nat.double() - t64, t16.double() - t64
    scale = t64.pow(2).mean().sqrt().item() + 1e-300
    rn, rt = en.pow(2).mean().sqrt().item() / scale, et.pow(2).mean().sqrt().item() / scale
    wn, wt = en.abs().max().item(), et.abs().max().item()
    assert rn <= 1.25 * rt, f"{what}: relative rms {rn:.3g} > 1.25 x torch bf16's {rt:.3g}"
    assert wn <= 2.0 * wt, f"{what}: worst element {wn:.3g} > 2 x torch bf16's {wt:.3g}"


def check_module(kind, cin, cout, n, T, bias=True, need_x=False, seed=0):
    br = make_bridge(kind, cin, cout, bias, seed)
    torch.manual_seed(seed + 1)
    x = torch.randn(n, T, cin, device=DEV).to(torch.bfloat16)
    gout = (torch.randn(n, T, cout, device=DEV) / math.sqrt(cout)).to(torch.bfloat16)
    y, g, gx = native_grads(br, x, gout, need_x)
    _, g16, gx16 = torch_grads(br, x, gout, torch.bfloat16, need_x)
    _, g64, gx64 = torch_grads(br, x, gout, torch.float64, need_x)
    assert set(g) == set(g64)
    for name in g:
        assert g[name].dtype == torch.bfloat16 and g[name].shape == g64[name].shape
        assert_rule(g[name], g16[name], g64[name], f"{kind} {cin}->{cout} rows {n}x{T}: grad {name}")
    if need_x:
        assert gx is not None and gx.shape == x.shape
        assert_rule(gx, gx16, gx64, f"{kind} {cin}->{cout}: x.grad")
    else:
        assert gx is None
    return br, x, gout, y, g


# ---- 1 / 3: gradients per kind, small and ragged row counts, with and without x.requires_grad --------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cin", [128, 512])
@pytest.mark.parametrize("n,T", [(3, 64), (2, 37)])
@pytest.mark.parametrize("need_x", [False, True])
def test_gradients_per_kind(kind, cin, n, T, need_x):
    check_module(kind, cin, 256, n, T, need_x=need_x, seed=cin + T)


@pytest.mark.parametrize("kind", ["linear", "mlp2x_gelu", "internvl_mlp"])
def test_gradients_without_biases(kind):
    br = make_bridge(kind, 128, 256, bias=False)
    assert all(m.bias is None for m in br.modules() if isinstance(m, nn.Linear))
    check_module(kind, 128, 256, 3, 64, bias=False, need_x=True)


# ---- 2: BASELINE's projector widths, 8 tiles: the split and the unsplit wgrad route ------------------------------------------------
@pytest.mark.parametrize("kind,cin,cout,T,splits", [("mlp2x_gelu", 1024, 4096, 576, 1),      # W_0 [4096, 1024]: 256 tiles -> split
                                                    ("internvl_mlp", 12800, 4096, 256, 0)])  # 3200 / 1024 tiles: unsplit
def test_baseline_widths(kind, cin, cout, T, splits):
    L = _lib.lib()
    before = L.vllm_gemm_wgrad_split_launches()
    check_module(kind, cin, cout, 8, T, need_x=kind == "internvl_mlp", seed=7)
    assert L.vllm_gemm_wgrad_split_launches() - before == splits


# ---- 4: the training forward computes the inference forward's bits -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,T,cin,cout", [(3, 64, 128, 256), (2, 37, 512, 256), (8, 576, 1024, 4096)])
def test_training_forward_equals_inference_forward(kind, n, T, cin, cout):
    br = make_bridge(kind, cin, cout, seed=3)
    x = torch.randn(n, T, cin, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        ref = br(x)
    y = br(x)
    assert y.grad_fn is not None
    assert torch.equal(y, ref)
    y2 = br(x.clone().requires_grad_(True))
    assert torch.equal(y2, ref)


# ---- 5: determinism and accumulation -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mlp2x_gelu", "internvl_mlp"])
def test_deterministic_and_accumulating(kind):
    br = make_bridge(kind, 512, 256, seed=5)
    x = torch.randn(4, 300, 512, device=DEV).to(torch.bfloat16)
    gout = torch.randn(4, 300, 256, device=DEV).to(torch.bfloat16)
    _, g1, _ = native_grads(br, x, gout, False)
    _, g2, _ = native_grads(br, x, gout, False)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for p in br.parameters():
        p.grad = None
    br(x).backward(gout)
    br(x).backward(gout)
    for k, p in br.named_parameters():
        assert torch.equal(p.grad, g1[k] + g1[k]), k


def test_in_place_update_between_forward_and_backward_is_caught():
    br = make_bridge("mlp2x_gelu", 128, 256)
    y = br(torch.randn(2, 64, 128, device=DEV).to(torch.bfloat16))
    with torch.no_grad():
        br[0].weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.sum().backward()


def test_project_hidden_state_still_refuses_under_grad():
    br = make_bridge("mlp2x_gelu", 128, 256)
    with pytest.raises(RuntimeError, match="forward\\(x\\)"):
        br.project_hidden_state(torch.randn(2, 65, 128, device=DEV).to(torch.bfloat16))


# ---- 6: building blocks against fp64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,pad", [(1000, 256, 128, 0), (77, 64, 640, 8), (4096, 1024, 256, 16), (2304, 512, 512, 24), (0, 128, 64, 0)])
@pytest.mark.parametrize("with_db", [False, True])
def test_wgrad_against_fp64(M, N, K, pad, with_db):
    """dW = dY^T A (and db = colsum dY): row strides wider than the width, ragged M, the split route (small N x K, many rows).
    Bound: fp32 accumulation of bf16 products in M / 32 MFMA steps (and at most 32 fixed-order partial sums): <= 2^-17 sum|terms| for
    the M here, + 1 ulp for the final rounding."""
    torch.manual_seed(M + N + K)
    L = _lib.lib()
    dy_full = torch.randn(max(M, 1), N + pad, device=DEV).to(torch.bfloat16)
    a_full = torch.randn(max(M, 1), K + pad, device=DEV).to(torch.bfloat16)
    dy, a = dy_full[:M, :N], a_full[:M, :K]
    dw_full = torch.full((N, K + pad), float("nan"), device=DEV).to(torch.bfloat16)
    db = torch.full((N,), float("nan"), device=DEV).to(torch.bfloat16) if with_db else None
    wsb = L.vllm_gemm_wgrad_workspace_bytes(M, N, K)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    before = L.vllm_gemm_wgrad_split_launches()
    _lib.check(L.vllm_gemm_wgrad_bf16(P(dy_full), N + pad, P(a_full), K + pad, M, N, K, P(dw_full), K + pad, P(db), P(ws), wsb, stream()),
               "vllm_gemm_wgrad_bf16")
    torch.cuda.synchronize()
    assert (L.vllm_gemm_wgrad_split_launches() - before == 1) == (wsb > 0)
    ref = dy.double().T @ a.double()
    mag = dy.double().abs().T @ a.double().abs()
    assert_bound(dw_full[:, :K], ref, mag, f"wgrad {M}x{N}x{K}")
    if pad:
        assert torch.isnan(dw_full[:, K:].float()).all()   # nothing written past the width
    if with_db:
        assert_bound(db, dy.double().sum(0), dy.double().abs().sum(0), f"db {M}x{N}")
    # run-to-run identical
    dw2 = torch.empty_like(dw_full)
    _lib.check(L.vllm_gemm_wgrad_bf16(P(dy_full), N + pad, P(a_full), K + pad, M, N, K, P(dw2), K + pad, None, P(ws), wsb, stream()))
    assert torch.equal(dw2[:, :K], dw_full[:, :K])


def gelu_grad64(h):
    h = h.double()
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


@pytest.mark.parametrize("force", [0, 0x100, 0x200, 0x300, 0x800, 0x1000])
@pytest.mark.parametrize("M,N,K", [(1000, 1024, 512), (300, 256, 128), (2048, 4096, 1024)])
def test_gelu_bwd_epilogue_against_fp64(force, M, N, K):
    """VLLM_EPI_GELU_BWD: y = (x W^T) * gelu'(res) under every schedule; bound 1 ulp + 2^-17 sum|x w| (gelu' <= 1.13; its own error
    ~1e-7 relative)."""
    torch.manual_seed(M + N + K + force)
    L = _lib.lib()
    pad = 8
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    res_full = (2 * torch.randn(M, N + pad, device=DEV)).to(torch.bfloat16)
    y_full = torch.full((M, N + pad), float("nan"), device=DEV).to(torch.bfloat16)
    _lib.check(L.vllm_gemm_bf16(P(x), P(w), None, P(y_full), M, N, K, K, K, N + pad, 6 | force, None, P(res_full), N + pad, 0, stream()),
               "vllm_gemm_bf16 GELU_BWD")
    torch.cuda.synchronize()
    res = res_full[:, :N]
    acc = x.double() @ w.double().T
    ref = acc * gelu_grad64(res)
    mag = (x.double().abs() @ w.double().abs().T) * 1.2
    assert_bound(y_full[:, :N], ref, mag, f"GELU_BWD force {force:#x} {M}x{N}x{K}")
    assert torch.isnan(y_full[:, N:].float()).all()
    # a bias is refused (the epilogue has none)
    b = torch.zeros(N, device=DEV, dtype=torch.bfloat16)
    assert L.vllm_gemm_bf16(P(x), P(w), P(b), P(y_full), M, N, K, K, K, N + pad, 6 | force, None, P(res_full), N + pad, 0, stream()) == -1


@pytest.mark.parametrize("rows,C", [(300, 128), (77, 1024), (64, 12800)])
@pytest.mark.parametrize("with_dx", [False, True])
def test_layernorm_backward_against_fp64(rows, C, with_dx):
    """grad_x / grad_w / grad_b of nn.LayerNorm from fp32 grad_y (bf16 x, gamma): against fp64 autograd of F.layer_norm.  Bound: 1 ulp
    + 2^-17 of the natural magnitude (sum|terms| for the column sums; r (|g| + mean|g| + |xhat| mean|g xhat|) for grad_x)."""
    torch.manual_seed(rows + C)
    L = _lib.lib()
    x = (torch.randn(rows, C, device=DEV) * 2 + 0.5).to(torch.bfloat16)
    gam = (1 + 0.1 * torch.randn(C, device=DEV)).to(torch.bfloat16)
    bet = (0.1 * torch.randn(C, device=DEV)).to(torch.bfloat16)
    gy = torch.randn(rows, C, device=DEV)
    eps = 1e-5
    gx = torch.full((rows, C), float("nan"), device=DEV).to(torch.bfloat16) if with_dx else None
    gw = torch.empty(C, device=DEV, dtype=torch.bfloat16)
    gb = torch.empty(C, device=DEV, dtype=torch.bfloat16)
    wsb = L.vllm_layernorm_backward_workspace_bytes(rows, C)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=DEV)
    _lib.check(L.vllm_layernorm_backward_bf16(P(x), C, P(gy), C, P(gam), eps, rows, C, P(gx), C, P(gw), P(gb), P(ws), wsb, stream()),
               "vllm_layernorm_backward_bf16")
    torch.cuda.synchronize()
    xd = x.double().requires_grad_(True)
    gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (C,), gd, bd, eps).backward(gy.double())
    mean = x.double().mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(((x.double() - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x.double() - mean) * r
    assert_bound(gw, gd.grad, (gy.double() * xh).abs().sum(0), "LayerNorm grad_w")
    assert_bound(gb, bd.grad, gy.double().abs().sum(0), "LayerNorm grad_b")
    if with_dx:
        g = gy.double() * gam.double()
        mag = r * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)) * 4
        assert_bound(gx, xd.grad, mag, "LayerNorm grad_x")


# ---- 7: placement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mlp2x_gelu", "internvl_mlp"])
def test_misaligned_input_and_side_stream(kind):
    br = make_bridge(kind, 512, 256, seed=11)
    n, T, C = 3, 100, 512
    base = torch.randn(n * T * C + 1, device=DEV).to(torch.bfloat16)
    gout = torch.randn(n, T, 256, device=DEV).to(torch.bfloat16)
    x_al = base[:-1].view(n, T, C).clone()
    y0, g0, gx0 = native_grads(br, x_al, gout, True)
    # x at an odd storage offset
    x_off = base[1:].view(n, T, C)
    x_off.copy_(x_al)
    assert x_off.data_ptr() % 16 != 0
    y1, g1, gx1 = native_grads(br, x_off, gout, True)
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    # forward + backward on a side stream, behind the work that produced x and grad_output
    s = torch.cuda.Stream()
    xs = (x_al.float() * 1.0).to(torch.bfloat16)
    gs = (gout.float() * 1.0).to(torch.bfloat16)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for p in br.parameters():
            p.grad = None
        xx = xs.detach().requires_grad_(True)
        y2 = br(xx)
        y2.backward(gs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(y2, y0) and torch.equal(xx.grad, gx0)
    for k, p in br.named_parameters():
        assert torch.equal(p.grad, g0[k]), k


def _desc(br, kind, ps=0, skip=0):
    from visionllm_amd.bridge import _BridgeTrain, _modules
    lin, ln = _modules(br, kind)
    params = [t for m in lin for t in (m.weight, m.bias)] + ([ln.weight, ln.bias] if ln is not None else [])
    keep = []
    d = _BridgeTrain._desc(kind, len(lin), ln.eps if ln is not None else 0.0, params, keep)
    d.pixel_shuffle, d.skip_cls = ps, skip
    return d, keep


@pytest.mark.parametrize("kind", ["mlp2x_gelu", "internvl_mlp"])
def test_invalid_calls_write_nothing(kind):
    L = _lib.lib()
    br = make_bridge(kind, 128, 256)
    rows, Cin, Cout = 2048, 128, 256
    x = torch.randn(rows, Cin, device=DEV).to(torch.bfloat16)
    out = torch.full((rows, Cout), 7.0, device=DEV).to(torch.bfloat16)
    pre = [torch.full((rows, Cout), 7.0, device=DEV).to(torch.bfloat16)]
    act = [torch.full((rows, Cout), 7.0, device=DEV).to(torch.bfloat16)]
    lnb = torch.full((rows, Cin), 7.0, device=DEV).to(torch.bfloat16)
    arr = lambda ts: (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - len(ts))))
    d, keep = _desc(br, kind)
    wsb = L.vllm_bridge_backward_workspace_bytes(ctypes.byref(d), rows, 1)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    for ps, skip in [(1, 0), (0, 1)]:
        dd, k2 = _desc(br, kind, ps, skip)
        assert L.vllm_bridge_forward_train(ctypes.byref(dd), P(x), rows, P(out), arr(pre), arr(act), P(lnb), P(ws), wsb, stream()) == -1
        assert b"forward(x)" in L.vllm_last_error()
        assert L.vllm_bridge_backward_workspace_bytes(ctypes.byref(dd), rows, 1) == -1
        gw = [torch.full(p.shape, 7.0, device=DEV).to(torch.bfloat16) for p in (br[0].weight, br[-1].weight)] if kind != "internvl_mlp" else \
             [torch.full(p.shape, 7.0, device=DEV).to(torch.bfloat16) for p in (br[1].weight, br[3].weight)]
        assert L.vllm_bridge_backward(ctypes.byref(dd), P(x), rows, P(out), arr(pre), arr(act), P(lnb), None, arr(gw), None, None, None,
                                      P(ws), wsb, stream()) == -1
    # a workspace that is too small
    assert L.vllm_bridge_forward_train(ctypes.byref(d), P(x), rows, P(out), arr(pre), arr(act), P(lnb), P(ws), 1024, stream()) == -1
    gw = [torch.full((Cout, Cin), 7.0, device=DEV).to(torch.bfloat16), torch.full((Cout, Cout), 7.0, device=DEV).to(torch.bfloat16)]
    assert L.vllm_bridge_backward(ctypes.byref(d), P(x), rows, P(out), arr(pre), arr(act), P(lnb), P(x), arr(gw), None, None, None,
                                  P(ws), wsb - 256, stream()) == -1
    torch.cuda.synchronize()
    for t in [out, pre[0], act[0], lnb] + gw:
        assert (t == 7.0).all()
    assert (ws == 0).all()
