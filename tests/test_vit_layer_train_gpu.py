"""GPU: training one InternViT encoder layer (layer_train.cpp) and its new row-wise kernels (norm.hip) and GEMM epilogue.

Yardstick: torch fp64 autograd of the reference's statements restated in vit_layer_train_inputs.py, on the same bf16 parameters, input
and grad_out.  The kernels alone are judged per element (1 bf16 ulp + 2^-17 of the natural magnitude, the LayerNorm backward test's
form); the assembled layer by DESIGN section 5's rule: relative rms against fp64 <= 1.25 x that of torch's own bf16 autograd of the same
statements, for the output, x.grad and every parameter gradient (both numbers are printed)."""
import ctypes
import functools
import math

import pytest
import torch

import vit_layer_train_inputs as I
from bounds import P, stream
from visionllm_amd import _lib
from visionllm_amd.intern_vit import (InternRMSNorm, InternVisionConfig, InternVisionEncoder, InternVisionEncoderLayer, InternVisionModel)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def nan_like(rows, cols):
    return torch.full((rows, cols), NAN, device=DEV).to(torch.bfloat16)


def padded(t, pad):
    """a copy of the 2-D tensor inside rows `pad` elements wider, the padding NaN"""
    full = nan_like(t.shape[0], t.shape[1] + pad)
    full[:, :t.shape[1]] = t
    return full


# ---- 1: RMSNorm backward against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
@pytest.mark.parametrize("with_dx,with_res", [(False, False), (True, False), (True, True)])   # (grad_res is added into grad_x)
def test_rmsnorm_backward_against_fp64(rows, C, with_dx, with_res):
    L = _lib.lib()
    x, gy, gres, w = I.norm_case(rows, C, device=DEV)
    pad = 8
    xf, gyf, grf = padded(x, pad), padded(gy, 2 * pad), padded(gres, 3 * pad)
    gx = nan_like(rows, C + pad) if with_dx else None
    gw = torch.full((C,), NAN, device=DEV).to(torch.bfloat16)
    wsb = L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    call = lambda gx_, gw_: _lib.check(L.vllm_rmsnorm_backward_bf16(
        P(xf), C + pad, P(gyf), C + 2 * pad, P(w), None, 1, I.EPS, rows, C, P(gx_), C + pad, P(grf) if with_res else None, C + 3 * pad,
        P(gw_), None, P(ws), wsb, stream()), "vllm_rmsnorm_backward_bf16")
    call(gx, gw)
    torch.cuda.synchronize()
    rx, rw, mx, mw = I.rms_bwd_ref(x, gy, w, gres if with_res else None)
    ew = I.excess_ulp(gw, rw, mw)
    print(f"rmsnorm bwd {rows}x{C}: grad_w {ew:.3f} of the bound")
    assert ew <= 1.0
    if with_dx:
        ex = I.excess_ulp(gx[:, :C], rx, mx)
        print(f"rmsnorm bwd {rows}x{C} res={with_res}: grad_x {ex:.3f} of the bound")
        assert ex <= 1.0
        assert torch.isnan(gx[:, C:].float()).all(), "wrote into the padding"
    # run-to-run identical; grad_w alone (no grad_x) and grad_x alone give the same bits
    gx2 = nan_like(rows, C + pad) if with_dx else None
    gw2 = torch.empty_like(gw)
    call(gx2, gw2)
    assert torch.equal(gw2, gw)
    if with_dx:
        assert torch.equal(gx2[:, :C], gx[:, :C])
        gx3 = nan_like(rows, C + pad)
        call(gx3, None)
        assert torch.equal(gx3[:, :C], gx[:, :C])


@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
def test_qk_norm_backward_in_place_on_a_qkv_slab(rows, C):
    """G = 2: the q and k blocks of a [rows, 3C] gradient are rewritten in place in ONE launch, the v block is not touched."""
    L = _lib.lib()
    xq, gq, _, wq = I.norm_case(rows, C, seed=1, device=DEV)
    xk, gk, xv, wk = I.norm_case(rows, C, seed=2, device=DEV)
    _, gv, _, _ = I.norm_case(rows, C, seed=3, device=DEV)
    qkv = torch.cat([xq, xk, xv], 1).contiguous()
    g = torch.cat([gq, gk, gv], 1).contiguous()
    g0 = g.clone()
    gwq = torch.empty(C, device=DEV, dtype=torch.bfloat16)
    gwk = torch.empty(C, device=DEV, dtype=torch.bfloat16)
    wsb = L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 2)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    _lib.check(L.vllm_rmsnorm_backward_bf16(P(qkv), 3 * C, P(g), 3 * C, P(wq), P(wk), 2, I.EPS, rows, C, P(g), 3 * C, None, 0, P(gwq), P(gwk),
                                            P(ws), wsb, stream()), "vllm_rmsnorm_backward_bf16 G=2")
    torch.cuda.synchronize()
    assert torch.equal(g[:, 2 * C:], g0[:, 2 * C:]), "the v block changed"
    for name, x_, g_, w_, out, gw in (("q", xq, gq, wq, g[:, :C], gwq), ("k", xk, gk, wk, g[:, C:2 * C], gwk)):
        rx, rw, mx, mw = I.rms_bwd_ref(x_, g_, w_)
        assert I.excess_ulp(out, rx, mx) <= 1.0, name
        assert I.excess_ulp(gw, rw, mw) <= 1.0, name
    # the same bits as two G = 1 launches out of place
    for x_, g_, w_, out, gw in ((xq, gq, wq, g[:, :C], gwq), (xk, gk, wk, g[:, C:2 * C], gwk)):
        o1, w1 = torch.empty_like(x_), torch.empty_like(gw)
        _lib.check(L.vllm_rmsnorm_backward_bf16(P(x_), C, P(g_), C, P(w_), None, 1, I.EPS, rows, C, P(o1), C, None, 0, P(w1), None, P(ws), wsb,
                                                stream()))
        assert torch.equal(o1, out) and torch.equal(w1, gw)


# ---- 2: LayerScale backward against fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
def test_layerscale_backward_against_fp64(rows, C):
    L = _lib.lib()
    go, y, _, w = I.norm_case(rows, C, seed=1, device=DEV)
    ls = (0.1 * w.float()).to(torch.bfloat16)
    pad = 8
    gof, yf = padded(go, pad), padded(y, 2 * pad)
    gy = nan_like(rows, C + 3 * pad)
    gls = torch.full((C,), NAN, device=DEV).to(torch.bfloat16)
    wsb = L.vllm_layerscale_backward_workspace_bytes(rows, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    call = lambda gy_, gls_: _lib.check(L.vllm_layerscale_backward_bf16(P(gof), C + pad, P(yf), C + 2 * pad, P(ls), rows, C, P(gy_), C + 3 * pad,
                                                                        P(gls_), P(ws), wsb, stream()), "vllm_layerscale_backward_bf16")
    call(gy, gls)
    torch.cuda.synchronize()
    ry, rls, mls = I.ls_bwd_ref(go, y, ls)
    assert I.excess_ulp(gy[:, :C], ry, torch.zeros_like(ry)) <= 1.0
    e = I.excess_ulp(gls, rls, mls)
    print(f"layerscale bwd {rows}x{C}: grad_ls {e:.3f} of the bound")
    assert e <= 1.0
    assert torch.isnan(gy[:, C:].float()).all(), "wrote into the padding"
    gy2, gls2 = nan_like(rows, C + 3 * pad), torch.empty_like(gls)
    call(gy2, None)
    call(None, gls2)
    assert torch.equal(gy2[:, :C], gy[:, :C]) and torch.equal(gls2, gls)


# ---- 3: the residual epilogue that also keeps the pre-LayerScale output ----------------------------------------------------------------
@pytest.mark.parametrize("force", [0, 0x100, 0x200, 0x300, 0x800])
@pytest.mark.parametrize("M,N,K,pad,scaled", [(300, 256, 128, 0, True), (1100, 1024, 512, 0, True), (1100, 1024, 512, 4, True),
                                              (1100, 1024, 512, 0, False), (16500, 2048, 256, 0, True)])
def test_residual_save_epilogue(force, M, N, K, pad, scaled):
    """EPI_RESIDUAL_SAVE under every schedule it is built for (128 x 128; 8-phase with 256- / 192-row tiles and on the 32x32x16
    instruction, through LDS and -- odd row strides -- straight from the accumulators, the residual as the accumulators' initial value
    or read in the epilogue; the last shape is one the persistent schedule takes for EPI_RESIDUAL): Y equals EPI_RESIDUAL on one
    workgroup per tile, pre is bf16(x W^T + b) to the GEMM tests' bound."""
    torch.manual_seed(M + N + K + force + pad)
    L = _lib.lib()
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(M, K, device=DEV))
    w = bf(torch.randn(N, K, device=DEV) / math.sqrt(K))
    b = bf(0.1 * torch.randn(N, device=DEV))
    ls = bf(0.1 * (1 + 0.1 * torch.randn(N, device=DEV))) if scaled else None
    res = bf(torch.randn(M, N + pad, device=DEV))
    ld = N + pad
    y0, y1, pre = nan_like(M, ld), nan_like(M, ld), nan_like(M, ld)
    _lib.check(L.vllm_gemm_bf16(P(x), P(w), P(b), P(y0), M, N, K, K, K, ld, 3 | force | 0x1000, P(ls), P(res), ld, 0, stream()), "EPI_RESIDUAL")
    _lib.check(L.vllm_gemm_bf16_residual_save(P(x), P(w), P(b), P(y1), P(pre), M, N, K, K, K, ld, 3 | force, P(ls), P(res), ld, stream()),
               "vllm_gemm_bf16_residual_save")
    torch.cuda.synchronize()
    assert torch.equal(y1[:, :N], y0[:, :N]), "Y differs from EPI_RESIDUAL"
    if pad:
        assert torch.isnan(y1[:, N:].float()).all() and torch.isnan(pre[:, N:].float()).all()
    rows = torch.cat([torch.arange(0, min(M, 300)), torch.arange(max(M - 300, 0), M)]).unique().to(DEV)
    ref = x[rows].double() @ w.double().T + b.double()
    mag = x[rows].double().abs() @ w.double().abs().T + b.double().abs()
    e = I.excess_ulp(pre[rows, :N], ref, mag)
    print(f"residual-save force {force:#x} {M}x{N}x{K} pad {pad} scaled {scaled}: pre {e:.3f} of the bound")
    assert e <= 1.0
    assert not torch.isnan(pre[:, :N].float()).any()


# ---- shared layer runs -------------------------------------------------------------------------------------------------------------
def build_layer(cfg_tuple, seed=0):
    hidden, heads, inter, B, S, qkn, qkvb = cfg_tuple
    cfg = InternVisionConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter, num_hidden_layers=1,
                             qk_normalization=qkn, qkv_bias=qkvb, layer_norm_eps=I.EPS)
    layer = InternVisionEncoderLayer(cfg)
    params = I.make_params(hidden, inter, qkn, qkvb, seed=seed, device=DEV)
    layer = layer.to(DEV).to(torch.bfloat16)
    missing = layer.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return layer, params


def native_run(layer, x, gout, need_x=True):
    for p in layer.parameters():
        p.grad = None
    xx = x.detach().requires_grad_(need_x)
    y = layer(xx)
    y.backward(gout)
    return y.detach(), {n: (p.grad.clone() if p.grad is not None else None) for n, p in layer.named_parameters()}, xx.grad


@functools.lru_cache(maxsize=None)
def layer_case(idx):
    """-> everything the tests of configuration `idx` share (computed once, never modified)"""
    cfg = I.LAYER_CONFIGS[idx]
    hidden, heads, inter, B, S, qkn, qkvb = cfg
    layer, params = build_layer(cfg, seed=idx)
    x, gout = I.make_io(B, S, hidden, seed=idx, device=DEV)
    nat = native_run(layer, x, gout)
    t64 = I.autograd_layer(params, x, gout, heads, torch.float64)
    t16 = I.autograd_layer(params, x, gout, heads, torch.bfloat16)
    return dict(cfg=cfg, layer=layer, params=params, x=x, gout=gout, nat=nat, t64=t64, t16=t16)


# ---- 4: the training forward is the inference encoder's layer where that one launches its norms ----------------------------------------
def test_layer_forward_equals_the_inference_encoder():
    torch.manual_seed(4)
    cfg = InternVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, image_size=70, patch_size=14,
                             layer_norm_eps=I.EPS)
    model = InternVisionModel(cfg)
    with torch.no_grad():
        for i, lyr in enumerate(model.encoder.layers):
            lyr.load_state_dict({k: v.float() for k, v in I.make_params(128, 256, seed=40 + i).items()})
    model = model.to(DEV).to(torch.bfloat16)
    pix = torch.randn(3, 3, 70, 70, device=DEV).to(torch.bfloat16)
    hs = model(pix, output_hidden_states=True).hidden_states
    assert len(hs) == 3 and hs[0].shape == (3, 26, 128)
    for i, lyr in enumerate(model.encoder.layers):
        with torch.no_grad():
            y0 = lyr(hs[i])
        assert y0.grad_fn is None and not y0.requires_grad
        assert torch.equal(y0, hs[i + 1]), f"layer {i}: no-grad forward differs from the inference encoder"
        y1 = lyr(hs[i])
        assert y1.grad_fn is not None
        assert torch.equal(y1, hs[i + 1]), f"layer {i}: training forward differs from the inference encoder"
        y2 = lyr(hs[i].clone().requires_grad_(True))
        assert torch.equal(y2, hs[i + 1])


# ---- 5: gradients by the assembled-bf16 rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(I.LAYER_CONFIGS)))
def test_layer_gradients(idx):
    L = _lib.lib()
    c = layer_case(idx)
    hidden, heads, inter, B, S, qkn, qkvb = c["cfg"]
    (y, g, gx), (y64, g64, gx64), (y16, g16, gx16) = c["nat"], c["t64"], c["t16"]
    assert set(g) == set(g64), set(g) ^ set(g64)
    rows = [("out", y, y16, y64), ("x.grad", gx, gx16, gx64)] + [(n, g[n], g16[n], g64[n]) for n in sorted(g)]
    bad = []
    for name, a, b, ref in rows:
        assert a is not None and a.dtype == torch.bfloat16 and a.shape == ref.shape, name
        rn, rt = I.rel_rms(a, ref), I.rel_rms(b, ref)
        print(f"layer {hidden}/{heads}/{inter} {B}x{S}  {name:22s} native {rn:.4g}  torch bf16 {rt:.4g}  ratio {rn / rt:.3f}")
        if not rn <= 1.25 * rt:
            bad.append(f"{name}: {rn:.4g} > 1.25 x {rt:.4g}")
    assert not bad, bad
    if idx == 2:   # this configuration is the one meant to cover the split weight-gradient route (proj: 64 output tiles) and the 8-phase GEMM
        assert L.vllm_gemm_wgrad_workspace_bytes(B * S, hidden, hidden) > 0 and B * S >= 1024


# ---- 6: frozen subsets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 1])
def test_frozen_subsets(idx):
    c = layer_case(idx)
    layer, _ = build_layer(c["cfg"], seed=idx)
    trainable = {"ls1", "ls2", "norm1.weight", "norm2.weight", "attn.q_norm.weight", "attn.k_norm.weight"}
    for n, p in layer.named_parameters():
        p.requires_grad_(n in trainable)
    y, g, gx = native_run(layer, c["x"], c["gout"], need_x=False)
    assert gx is None and torch.equal(y, c["nat"][0])
    for n in g:
        if n in trainable:
            assert torch.equal(g[n], c["nat"][1][n]), n
        else:
            assert g[n] is None, n
    # a bias alone: its gradient still comes (with the weight's launch), the weight's is not reported
    for n, p in layer.named_parameters():
        p.requires_grad_(n == "mlp.fc2.bias")
    _, g, _ = native_run(layer, c["x"], c["gout"], need_x=False)
    assert torch.equal(g["mlp.fc2.bias"], c["nat"][1]["mlp.fc2.bias"]) and g["mlp.fc2.weight"] is None


# ---- 7: the encoder, with and without checkpointing --------------------------------------------------------------------------------
def test_encoder_checkpointing_changes_nothing():
    cfg = InternVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, layer_norm_eps=I.EPS)
    enc = InternVisionEncoder(cfg)
    for i, lyr in enumerate(enc.layers):
        lyr.load_state_dict({k: v.float() for k, v in I.make_params(128, 256, seed=70 + i).items()})
    enc = enc.to(DEV).to(torch.bfloat16).train()
    x, gout = I.make_io(2, 37, 128, seed=7, device=DEV)
    runs = []
    for ckpt in (True, False):
        enc.gradient_checkpointing = ckpt
        for p in enc.parameters():
            p.grad = None
        xx = x.detach().requires_grad_(True)
        out = enc(xx, output_hidden_states=True)
        assert len(out.hidden_states) == 3 and out.hidden_states[0] is xx
        out.last_hidden_state.backward(gout)
        runs.append((out.last_hidden_state.detach(), xx.grad, {n: p.grad.clone() for n, p in enc.named_parameters()}))
    (y0, gx0, g0), (y1, gx1, g1) = runs
    assert torch.equal(y0, y1) and torch.equal(gx0, gx1)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    # frozen input, trainable layers, checkpointing on: the parameters still get their gradients
    enc.gradient_checkpointing = True
    for p in enc.parameters():
        p.grad = None
    enc(x).last_hidden_state.backward(gout)
    for n, p in enc.named_parameters():
        assert torch.equal(p.grad, g0[n]), n
    assert enc(x, return_dict=False)[0].shape == x.shape


# ---- 8: determinism and hygiene ----------------------------------------------------------------------------------------------------
def test_deterministic_and_accumulating():
    c = layer_case(0)
    layer, x, gout = c["layer"], c["x"], c["gout"]
    y2, g2, gx2 = native_run(layer, x, gout)
    assert torch.equal(y2, c["nat"][0]) and torch.equal(gx2, c["nat"][2])
    for n in g2:
        assert torch.equal(g2[n], c["nat"][1][n]), n
    for p in layer.parameters():
        p.grad = None
    layer(x).backward(gout)
    layer(x).backward(gout)
    for n, p in layer.named_parameters():
        assert torch.equal(p.grad, g2[n] + g2[n]), n
    for p in layer.parameters():
        p.grad = None


def test_in_place_update_between_forward_and_backward_is_caught():
    layer, _ = build_layer(I.LAYER_CONFIGS[0], seed=8)
    x, gout = I.make_io(2, 37, 128, seed=8, device=DEV)
    y = layer(x)
    with torch.no_grad():
        layer.mlp.fc1.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(gout)


def test_misaligned_input_and_side_stream():
    c = layer_case(0)
    layer, gout = c["layer"], c["gout"]
    B, S, C = c["x"].shape
    base = torch.zeros(B * S * C + 1, device=DEV, dtype=torch.bfloat16)
    x_off = base[1:].view(B, S, C)
    x_off.copy_(c["x"])
    assert x_off.data_ptr() % 16 != 0
    y1, g1, gx1 = native_run(layer, x_off, gout)
    assert torch.equal(y1, c["nat"][0]) and torch.equal(gx1, c["nat"][2])
    for n in g1:
        assert torch.equal(g1[n], c["nat"][1][n]), n
    s = torch.cuda.Stream()
    xs, gs = (c["x"].float() * 1.0).to(torch.bfloat16), (gout.float() * 1.0).to(torch.bfloat16)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y2, g2, gx2 = native_run(layer, xs, gs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(y2, c["nat"][0]) and torch.equal(gx2, c["nat"][2])
    for n in g2:
        assert torch.equal(g2[n], c["nat"][1][n]), n
    for p in layer.parameters():
        p.grad = None


def test_invalid_calls_write_nothing():
    from visionllm_amd.intern_vit import _LAYER_PARAMS, _SAVED, _layer_desc
    L = _lib.lib()
    layer, _ = build_layer(I.LAYER_CONFIGS[0], seed=9)
    B, S, C, inter, heads = 2, 37, 128, 256, 2
    M = B * S
    x, gout = I.make_io(B, S, C, seed=9, device=DEV)
    seven = lambda *s: torch.full(s, 7.0, device=DEV).to(torch.bfloat16)
    out = seven(B, S, C)
    saved = [seven(M, 3 * C), seven(M, C), torch.full((B, heads, S), 7.0, device=DEV), seven(M, C), seven(M, C), seven(M, inter), seven(M, inter),
             seven(M, C)]
    sv = _lib.VllmVitLayerSaved(**{n: t.data_ptr() for n, t in zip(_SAVED, saved)})
    keep = []
    d = _layer_desc((heads, inter, I.EPS), layer._params(), keep)
    wsb = L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), B, S)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    grads = [seven(*p.shape) if p is not None else None for p in layer._params()]
    gs = _lib.VllmVitLayerGrads(**{n: (t.data_ptr() if t is not None else None) for n, t in zip(_LAYER_PARAMS, grads)})
    gx = seven(B, S, C)
    fwd = lambda dd, nbytes: L.vllm_vit_layer_forward_train(ctypes.byref(dd), P(x), B, S, P(out), ctypes.byref(sv), P(ws), nbytes, stream())
    bwd = lambda dd, nbytes: L.vllm_vit_layer_backward(ctypes.byref(dd), P(x), B, S, P(gout), ctypes.byref(sv), P(gx), ctypes.byref(gs), P(ws),
                                                       nbytes, stream())
    bad = _layer_desc((4, inter, I.EPS), layer._params(), keep)      # head_dim 32
    assert fwd(bad, wsb) == -1 and b"head_dim" in L.vllm_last_error()
    assert bwd(bad, wsb) == -1
    assert L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(bad), B, S) == -1
    assert fwd(d, 1024) == -1 and b"workspace" in L.vllm_last_error()    # short workspace
    assert bwd(d, wsb - 256) == -1 and b"workspace" in L.vllm_last_error()
    torch.cuda.synchronize()
    for t in [out, gx] + saved + [g for g in grads if g is not None]:
        assert (t == 7.0).all()
    assert (ws == 0).all()
    assert fwd(d, wsb) == 0 and bwd(d, wsb) == 0                           # and the valid call goes through
    torch.cuda.synchronize()
    assert not (out == 7.0).all() and not (gx == 7.0).all()


# ---- 9: the InternRMSNorm hook under autograd --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [128, 3200])
def test_rmsnorm_hook_under_autograd(C):
    rows = 150
    x, gy, _, w = I.norm_case(rows, C, seed=9, device=DEV)
    x3, gy3 = x.view(3, 50, C), gy.view(3, 50, C)
    norm = InternRMSNorm(C, eps=I.EPS).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(w)
        y0 = norm(x3)
    assert y0.grad_fn is None
    # the call as it was before this path existed (weight detached, no node): the same bits
    y_old = torch.empty_like(x)
    _lib.check(_lib.lib().vllm_rmsnorm_bf16(P(x), C, P(w), P(y_old), C, rows, C, I.EPS, stream()))
    assert torch.equal(y0.view(rows, C), y_old)
    xx = x3.detach().requires_grad_(True)
    y = norm(xx)
    assert y.grad_fn is not None and torch.equal(y, y0)
    y.backward(gy3)
    _, gx64, gw64 = I.autograd_rms_norm(x3, w, gy3, torch.float64)
    _, gx16, gw16 = I.autograd_rms_norm(x3, w, gy3, torch.bfloat16)
    for name, a, b, ref in (("x.grad", xx.grad, gx16, gx64), ("weight.grad", norm.weight.grad, gw16, gw64)):
        rn, rt = I.rel_rms(a, ref), I.rel_rms(b, ref)
        print(f"InternRMSNorm C={C} {name}: native {rn:.4g}  torch bf16 {rt:.4g}")
        assert rn <= 1.25 * rt, name
    # frozen weight: only x.grad
    norm.weight.requires_grad_(False)
    norm.weight.grad = None
    xx2 = x3.detach().requires_grad_(True)
    norm(xx2).backward(gy3)
    assert norm.weight.grad is None and torch.equal(xx2.grad, xx.grad)
