"""GPU: training one CLIP encoder layer (layer_train.cpp), its new row-wise kernel (norm.hip), the two quick-GELU training epilogues and
the tower from pixels (clip_vit.py).

Yardstick: torch fp64 autograd of HF 4.34's statements restated in clip_layer_train_inputs.py, on the same bf16 parameters, input and
grad_out.  The kernels alone are judged per element (1 bf16 ulp + 2^-17 of the natural magnitude, the LayerNorm backward test's form);
the assembled layer and tower by DESIGN section 5's rule: relative rms against fp64 <= 1.25 x that of torch's own bf16 autograd of the
same statements, for the output, x.grad and every parameter gradient (both numbers are printed)."""
import ctypes
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import clip_layer_train_inputs as I
import test_workspace_contract_gpu as WC
from bounds import P, assert_bound, stream
from visionllm_amd import _lib
from visionllm_amd.clip_vit import CLIPVisionModel, _CLIPEncoder, _CLIPEncoderLayer, _CLIPLayerNorm

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


def clip_config(hidden, heads, inter, layers=1, act="quick_gelu", image=70, patch=14):
    return SimpleNamespace(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter, num_hidden_layers=layers, image_size=image,
                           patch_size=patch, layer_norm_eps=I.EPS, hidden_act=act, output_hidden_states=False, use_return_dict=True)


# ---- 1: the new LayerNorm backward against fp64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
@pytest.mark.parametrize("with_dx", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_backward_res_against_fp64(rows, C, with_dx, with_res):
    """(grad_res is added into grad_x: without grad_x it has nowhere to go and the entry refuses it -- that case asserts the refusal and
    goes on without it)"""
    L = _lib.lib()
    x, gy, gres, w = I.norm_case(rows, C, device=DEV)
    pad = 8
    xf, gyf, grf = padded(x, pad), padded(gy, 2 * pad), padded(gres, 3 * pad)
    gx = nan_like(rows, C + 2 * pad) if with_dx else None
    gw, gb = nan_like(1, C)[0], nan_like(1, C)[0]
    wsb = L.vllm_layernorm_backward_res_workspace_bytes(rows, C)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    raw = lambda gy_, gx_, gres_, gw_, gb_: L.vllm_layernorm_backward_res_bf16(
        P(xf), C + pad, P(gy_), C + 2 * pad, P(w), I.EPS, rows, C, P(gx_), C + 2 * pad, P(gres_), C + 3 * pad, P(gw_), P(gb_), P(ws), wsb, stream())
    if with_res and not with_dx:
        assert raw(gyf, None, grf, gw, gb) == -1 and b"grad_res needs grad_x" in L.vllm_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(gw.float()).all() and torch.isnan(gb.float()).all(), "a refused call wrote"
        with_res = False
    res = grf if with_res else None
    call = lambda gy_, gx_, gw_, gb_: _lib.check(raw(gy_, gx_, res if gx_ is not None else None, gw_, gb_), "vllm_layernorm_backward_res_bf16")
    call(gyf, gx, gw, gb)
    torch.cuda.synchronize()
    rx, rw, rb, mx, mw, mb = I.ln_bwd_ref(x, gy, w, gres if with_res else None)
    ew, eb = I.excess_ulp(gw, rw, mw), I.excess_ulp(gb, rb, mb)
    print(f"layernorm bwd {rows}x{C}: grad_w {ew:.3f} grad_b {eb:.3f} of the bound")
    assert ew <= 1.0 and eb <= 1.0
    if with_dx:
        ex = I.excess_ulp(gx[:, :C], rx, mx)
        print(f"layernorm bwd {rows}x{C} res={with_res}: grad_x {ex:.3f} of the bound")
        assert ex <= 1.0
        assert torch.isnan(gx[:, C:].float()).all(), "wrote into the padding"
    # a second run gives identical bits; each output alone gives the same bits
    gx2 = nan_like(rows, C + 2 * pad) if with_dx else None
    gw2, gb2 = torch.empty_like(gw), torch.empty_like(gb)
    call(gyf, gx2, gw2, gb2)
    assert torch.equal(gw2, gw) and torch.equal(gb2, gb)
    gw3, gb3 = torch.empty_like(gw), torch.empty_like(gb)
    call(gyf, None, gw3, None)
    call(gyf, None, None, gb3)
    assert torch.equal(gw3, gw) and torch.equal(gb3, gb)
    if with_dx:
        assert torch.equal(gx2[:, :C], gx[:, :C])
        gx3 = nan_like(rows, C + 2 * pad)
        call(gyf, gx3, None, None)
        assert torch.equal(gx3[:, :C], gx[:, :C])
        # in place: grad_x aliasing grad_y (the same row stride) equals out of place bit for bit, and leaves the padding alone
        g_in = gyf.clone()
        gw4, gb4 = torch.empty_like(gw), torch.empty_like(gb)
        call(g_in, g_in, gw4, gb4)
        assert torch.equal(g_in[:, :C], gx[:, :C]) and torch.equal(gw4, gw) and torch.equal(gb4, gb)
        assert torch.isnan(g_in[:, C:].float()).all()


def test_layernorm_backward_res_without_rows_zero_fills_the_sums():
    L = _lib.lib()
    C = 128
    gw, gb = nan_like(1, C)[0], nan_like(1, C)[0]
    one = torch.zeros(16, device=DEV, dtype=torch.bfloat16)
    _lib.check(L.vllm_layernorm_backward_res_bf16(P(one), C, P(one), C, P(one), I.EPS, 0, C, None, C, None, 0, P(gw), P(gb), None, 0, stream()))
    torch.cuda.synchronize()
    assert (gw == 0).all() and (gb == 0).all()


# ---- 2 / 3: the two quick-GELU training epilogues ------------------------------------------------------------------------------------
FORCES = [0, 0x100, 0x200, 0x300, 0x800, 0x1000]                       # test_gelu_bwd_epilogue_against_fp64's
EPI_SHAPES = [(1000, 1024, 512), (300, 256, 128), (2048, 4096, 1024)]   # the last: one the persistent schedule takes for EPI_QUICK_GELU


@pytest.mark.parametrize("force", FORCES)
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_quick_gelu_save_epilogue(force, M, N, K):
    """Y equals VLLM_EPI_QUICK_GELU on one workgroup per tile bit for bit; pre is bf16(x W^T + b) to the GEMM tests' bound."""
    torch.manual_seed(M + N + K + force)
    L = _lib.lib()
    bf = lambda t: t.to(torch.bfloat16)
    pad = 8
    x = bf(torch.randn(M, K, device=DEV))
    w = bf(torch.randn(N, K, device=DEV) / math.sqrt(K))
    b = bf(0.1 * torch.randn(N, device=DEV))
    ld = N + pad
    y0, y1, pre = nan_like(M, ld), nan_like(M, ld), nan_like(M, ld)
    p0 = L.vllm_gemm_persistent_launches()
    _lib.check(L.vllm_gemm_bf16(P(x), P(w), P(b), P(y0), M, N, K, K, K, ld, 2 | force | 0x1000, None, None, 0, 0, stream()), "EPI_QUICK_GELU")
    _lib.check(L.vllm_gemm_bf16_quick_gelu_save(P(x), P(w), P(b), P(y1), P(pre), M, N, K, K, K, ld, force, stream()),
               "vllm_gemm_bf16_quick_gelu_save")
    torch.cuda.synchronize()
    assert L.vllm_gemm_persistent_launches() == p0
    assert torch.equal(y1[:, :N], y0[:, :N]), "Y differs from EPI_QUICK_GELU"
    assert torch.isnan(y1[:, N:].float()).all() and torch.isnan(pre[:, N:].float()).all()
    rows = torch.cat([torch.arange(0, min(M, 300)), torch.arange(max(M - 300, 0), M)]).unique().to(DEV)
    ref = x[rows].double() @ w.double().T + b.double()
    mag = x[rows].double().abs() @ w.double().abs().T + b.double().abs()
    e = I.excess_ulp(pre[rows, :N], ref, mag)
    print(f"quick-gelu-save force {force:#x} {M}x{N}x{K}: pre {e:.3f} of the bound")
    assert e <= 1.0
    assert not torch.isnan(pre[:, :N].float()).any()


def test_quick_gelu_save_keeps_the_persistent_schedules_bits():
    """Where the persistent schedule takes EPI_QUICK_GELU (the inference fc1), the training form's Y is still that call's Y."""
    torch.manual_seed(5)
    L = _lib.lib()
    M, N, K = 2048, 4096, 1024
    bf = lambda t: t.to(torch.bfloat16)
    x, w, b = bf(torch.randn(M, K, device=DEV)), bf(torch.randn(N, K, device=DEV) / math.sqrt(K)), bf(0.1 * torch.randn(N, device=DEV))
    y0, y1, pre = nan_like(M, N), nan_like(M, N), nan_like(M, N)
    p0 = L.vllm_gemm_persistent_launches()
    _lib.check(L.vllm_gemm_bf16(P(x), P(w), P(b), P(y0), M, N, K, K, K, N, 2, None, None, 0, 0, stream()), "EPI_QUICK_GELU")
    taken = L.vllm_gemm_persistent_launches() - p0
    _lib.check(L.vllm_gemm_bf16_quick_gelu_save(P(x), P(w), P(b), P(y1), P(pre), M, N, K, K, K, N, 0, stream()))
    torch.cuda.synchronize()
    print(f"persistent schedule taken by the inference call: {taken}")
    assert L.vllm_gemm_persistent_launches() - p0 == taken
    assert torch.equal(y1, y0)


@pytest.mark.parametrize("force", FORCES)
@pytest.mark.parametrize("M,N,K", EPI_SHAPES)
def test_quick_gelu_bwd_epilogue_against_fp64(force, M, N, K):
    """y = (x W^T) * q'(res) under every schedule; bound 1 ulp + 2^-17 * 1.2 sum|x w| (|q'| <= 1.0999; its own error ~1e-6 relative)."""
    torch.manual_seed(M + N + K + force)
    L = _lib.lib()
    pad = 8
    x = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV) / math.sqrt(K)).to(torch.bfloat16)
    res_full = (2 * torch.randn(M, N + pad, device=DEV)).to(torch.bfloat16)
    y_full = nan_like(M, N + pad)
    _lib.check(L.vllm_gemm_bf16_quick_gelu_bwd(P(x), P(w), None, P(y_full), M, N, K, K, K, N + pad, force, P(res_full), N + pad, stream()),
               "vllm_gemm_bf16_quick_gelu_bwd")
    torch.cuda.synchronize()
    acc = x.double() @ w.double().T
    ref = acc * I.quick_gelu_grad_ref(res_full[:, :N])
    mag = (x.double().abs() @ w.double().abs().T) * 1.2
    assert_bound(y_full[:, :N], ref, mag, f"QUICK_GELU_BWD force {force:#x} {M}x{N}x{K}")
    assert torch.isnan(y_full[:, N:].float()).all()
    # a bias is refused (the epilogue has none), and the refused call writes nothing
    b = torch.zeros(N, device=DEV, dtype=torch.bfloat16)
    y7 = torch.full((M, N + pad), 7.0, device=DEV).to(torch.bfloat16)
    assert L.vllm_gemm_bf16_quick_gelu_bwd(P(x), P(w), P(b), P(y7), M, N, K, K, K, N + pad, force, P(res_full), N + pad, stream()) == -1
    torch.cuda.synchronize()
    assert (y7 == 7.0).all()


# ---- shared layer runs -------------------------------------------------------------------------------------------------------------
def build_layer(cfg_tuple, seed=0):
    hidden, heads, inter, B, S, act = cfg_tuple
    layer = _CLIPEncoderLayer(clip_config(hidden, heads, inter, act=act))
    params = I.make_params(hidden, inter, seed=seed, device=DEV)
    layer = layer.to(DEV).to(torch.bfloat16)
    missing = layer.load_state_dict(params, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return layer, params


def native_run(layer, x, gout, need_x=True):
    for p in layer.parameters():
        p.grad = None
    xx = x.detach().requires_grad_(need_x)
    (y,) = layer(xx)
    y.backward(gout)
    return y.detach(), {n: (p.grad.clone() if p.grad is not None else None) for n, p in layer.named_parameters()}, xx.grad


@functools.lru_cache(maxsize=None)
def layer_case(idx):
    """-> everything the tests of configuration `idx` share (computed once, never modified)"""
    cfg = I.LAYER_CONFIGS[idx]
    hidden, heads, inter, B, S, act = cfg
    layer, params = build_layer(cfg, seed=idx)
    x, gout = I.make_io(B, S, hidden, seed=idx, device=DEV)
    nat = native_run(layer, x, gout)
    t64 = I.autograd_layer(params, x, gout, heads, act, torch.float64)
    t16 = I.autograd_layer(params, x, gout, heads, act, torch.bfloat16)
    return dict(cfg=cfg, layer=layer, params=params, x=x, gout=gout, nat=nat, t64=t64, t16=t16)


def same_run(got, want, tag=""):
    (y, g, gx), (y0, g0, gx0) = got, want
    assert torch.equal(y, y0), tag
    assert (gx is None and gx0 is None) or torch.equal(gx, gx0), tag
    assert set(g) == set(g0)
    for n in g0:
        assert torch.equal(g[n], g0[n]), (tag, n)


def small_model(seed, layers=2):
    """a CLIP tower of hidden 128 for 70 x 70 tiles (S = 26), every parameter bf16-valued and non-degenerate"""
    torch.manual_seed(seed)
    model = CLIPVisionModel(clip_config(128, 2, 256, layers=layers))
    with torch.no_grad():
        for i, lyr in enumerate(model.vision_model.encoder.layers):
            lyr.load_state_dict({k: v.float() for k, v in I.make_params(128, 256, seed=seed + i).items()})
        for ln in (model.vision_model.pre_layrnorm, model.vision_model.post_layernorm):
            ln.weight.copy_(1 + 0.1 * torch.randn(128))
            ln.bias.copy_(0.1 * torch.randn(128))
    return model.to(DEV).to(torch.bfloat16)


# ---- 4: the training forward is the inference encoder's layer where that one launches its norms ----------------------------------------
def test_layer_forward_equals_the_inference_encoder():
    model = small_model(40)
    pix = torch.randn(3, 3, 70, 70, device=DEV).to(torch.bfloat16)
    hs = model(pix, output_hidden_states=True).hidden_states
    assert len(hs) == 3 and hs[0].shape == (3, 26, 128)
    for i, lyr in enumerate(model.vision_model.encoder.layers):
        with torch.no_grad():
            (y0,) = lyr(hs[i])
        assert y0.grad_fn is None and not y0.requires_grad
        assert torch.equal(y0, hs[i + 1]), f"layer {i}: no-grad forward differs from the inference encoder"
        (y1,) = lyr(hs[i])
        assert y1.grad_fn is not None
        assert torch.equal(y1, hs[i + 1]), f"layer {i}: training forward differs from the inference encoder"
        (y2,) = lyr(hs[i].clone().requires_grad_(True))
        assert torch.equal(y2, hs[i + 1])


# ---- 5: gradients by the assembled-bf16 rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(I.LAYER_CONFIGS)))
def test_layer_gradients(idx):
    L = _lib.lib()
    c = layer_case(idx)
    hidden, heads, inter, B, S, act = c["cfg"]
    (y, g, gx), (y64, g64, gx64), (y16, g16, gx16) = c["nat"], c["t64"], c["t16"]
    assert set(g) == set(g64), set(g) ^ set(g64)
    assert {f"self_attn.{n}_proj.{k}" for n in "qkv" for k in ("weight", "bias")} <= set(g)      # q, k and v are judged apart
    rows = [("out", y, y16, y64), ("x.grad", gx, gx16, gx64)] + [(n, g[n], g16[n], g64[n]) for n in sorted(g)]
    bad = []
    for name, a, b, ref in rows:
        assert a is not None and a.dtype == torch.bfloat16 and a.shape == ref.shape, name
        rn, rt = I.rel_rms(a, ref), I.rel_rms(b, ref)
        print(f"clip layer {hidden}/{heads}/{inter} {act} {B}x{S}  {name:28s} native {rn:.4g}  torch bf16 {rt:.4g}  ratio {rn / rt:.3f}")
        if not rn <= 1.25 * rt:
            bad.append(f"{name}: {rn:.4g} > 1.25 x {rt:.4g}")
    assert not bad, bad
    # the k projection's bias shifts every score of a query row alike, which softmax does not see: its gradient is identically zero (the fp64
    # autograd leaves 1e-16 of rounding there), and the native backward writes that value instead of the column sum of the computed dK --
    # which measured 1.3-1.8 x the noise torch's bf16 autograd leaves in that tensor, against a reference of nothing
    assert g64["self_attn.k_proj.bias"].abs().max().item() < 1e-12 and not g["self_attn.k_proj.bias"].any()
    if idx == 2:   # this configuration is the one meant to cover the split weight-gradient route (proj: 64 output tiles) and the 8-phase GEMM
        assert L.vllm_gemm_wgrad_workspace_bytes(B * S, hidden, hidden) > 0 and B * S >= 1024


# ---- 6: behaviour that must give identical bits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 1])
def test_frozen_subsets(idx):
    c = layer_case(idx)
    layer, _ = build_layer(c["cfg"], seed=idx)
    subsets = [{"layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"},
               {"self_attn.k_proj.weight", "self_attn.v_proj.bias", "mlp.fc1.weight"},
               {"self_attn.out_proj.weight", "self_attn.out_proj.bias"},
               {"layer_norm2.bias"}]
    for trainable in subsets:
        for n, p in layer.named_parameters():
            p.requires_grad_(n in trainable)
        y, g, gx = native_run(layer, c["x"], c["gout"], need_x=False)
        assert gx is None and torch.equal(y, c["nat"][0])
        for n in g:
            if n in trainable:
                assert torch.equal(g[n], c["nat"][1][n]), n
            else:
                assert g[n] is None, n
    # a bias alone: its gradient still comes (with the weight's launch), the weight's is not reported -- for a q / k / v slice too
    for bias, weight in (("mlp.fc2.bias", "mlp.fc2.weight"), ("self_attn.q_proj.bias", "self_attn.q_proj.weight")):
        for n, p in layer.named_parameters():
            p.requires_grad_(n == bias)
        _, g, _ = native_run(layer, c["x"], c["gout"], need_x=False)
        assert torch.equal(g[bias], c["nat"][1][bias]) and g[weight] is None
        assert sum(v is not None for v in g.values()) == 1
    # everything frozen, only x.grad
    for p in layer.parameters():
        p.requires_grad_(False)
    y, g, gx = native_run(layer, c["x"], c["gout"], need_x=True)
    assert torch.equal(gx, c["nat"][2]) and all(v is None for v in g.values())


def test_encoder_checkpointing_changes_nothing():
    enc = _CLIPEncoder(clip_config(128, 2, 256, layers=2))
    assert enc.gradient_checkpointing is False
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
    # checkpointing only acts in training mode (HF's rule)
    enc.eval()
    with torch.no_grad():
        assert torch.equal(enc(x).last_hidden_state, y0)


def test_deterministic_and_accumulating():
    c = layer_case(0)
    layer, x, gout = c["layer"], c["x"], c["gout"]
    same_run(native_run(layer, x, gout), c["nat"], "second pass")
    g2 = c["nat"][1]
    for p in layer.parameters():
        p.grad = None
    layer(x)[0].backward(gout)
    layer(x)[0].backward(gout)
    for n, p in layer.named_parameters():
        assert torch.equal(p.grad, g2[n] + g2[n]), n
    for p in layer.parameters():
        p.grad = None


def test_misaligned_input_and_side_stream():
    c = layer_case(0)
    layer, gout = c["layer"], c["gout"]
    B, S, C = c["x"].shape
    base = torch.zeros(B * S * C + 1, device=DEV, dtype=torch.bfloat16)
    x_off = base[1:].view(B, S, C)
    x_off.copy_(c["x"])
    assert x_off.data_ptr() % 16 != 0
    same_run(native_run(layer, x_off, gout), c["nat"], "offset view")
    s = torch.cuda.Stream()
    xs, gs = (c["x"].float() * 1.0).to(torch.bfloat16), (gout.float() * 1.0).to(torch.bfloat16)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = native_run(layer, xs, gs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    same_run(got, c["nat"], "side stream")
    for p in layer.parameters():
        p.grad = None


# ---- 7: failure handling -----------------------------------------------------------------------------------------------------------
def test_in_place_update_between_forward_and_backward_is_caught():
    layer, _ = build_layer(I.LAYER_CONFIGS[0], seed=8)
    x, gout = I.make_io(2, 37, 128, seed=8, device=DEV)
    (y,) = layer(x)
    with torch.no_grad():
        layer.self_attn.k_proj.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(gout)


def test_invalid_calls_write_nothing():
    from visionllm_amd.clip_vit import _LAYER_PARAMS, _SAVED, _fused_params, _layer_desc
    L = _lib.lib()
    layer, _ = build_layer(I.LAYER_CONFIGS[0], seed=9)
    B, S, C, inter, heads = 2, 37, 128, 256, 2
    M = B * S
    x, gout = I.make_io(B, S, C, seed=9, device=DEV)
    seven = lambda *s: torch.full(s, 7.0, device=DEV).to(torch.bfloat16)
    out = seven(B, S, C)
    saved = [seven(M, 3 * C), seven(M, C), torch.full((B, heads, S), 7.0, device=DEV), seven(M, C), seven(M, inter), seven(M, inter)]
    sv = _lib.VllmClipLayerSaved(**{n: t.data_ptr() for n, t in zip(_SAVED, saved)})
    keep = []
    fused = _fused_params(layer._params())
    d = _layer_desc((heads, inter, _lib.EPI_QUICK_GELU, I.EPS), fused, keep)
    wsb = L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(d), B, S)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    grads = [seven(*p.shape) for p in fused]
    gs = _lib.VllmClipLayerGrads(**{n: t.data_ptr() for n, t in zip(_LAYER_PARAMS, grads)})
    gx = seven(B, S, C)
    fwd = lambda dd, nbytes: L.vllm_clip_layer_forward_train(ctypes.byref(dd), P(x), B, S, P(out), ctypes.byref(sv), P(ws), nbytes, stream())
    bwd = lambda dd, nbytes, gg=gs: L.vllm_clip_layer_backward(ctypes.byref(dd), P(x), B, S, P(gout), ctypes.byref(sv), P(gx), ctypes.byref(gg), P(ws),
                                                               nbytes, stream())
    bad = _layer_desc((4, inter, _lib.EPI_QUICK_GELU, I.EPS), fused, keep)      # head_dim 32
    assert fwd(bad, wsb) == -1 and b"head_dim" in L.vllm_last_error()
    assert bwd(bad, wsb) == -1
    assert L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(bad), B, S) == -1
    bad_act = _layer_desc((heads, inter, _lib.EPI_RESIDUAL, I.EPS), fused, keep)
    assert fwd(bad_act, wsb) == -1 and b"act" in L.vllm_last_error()
    assert bwd(bad_act, wsb) == -1
    assert fwd(d, 1024) == -1 and b"workspace" in L.vllm_last_error()    # short workspace
    assert bwd(d, wsb - 256) == -1 and b"workspace" in L.vllm_last_error()
    lone = _lib.VllmClipLayerGrads(**{n: (t.data_ptr() if n != "fc1_w" else None) for n, t in zip(_LAYER_PARAMS, grads)})
    assert bwd(d, wsb, lone) == -1 and b"bias gradient" in L.vllm_last_error()
    torch.cuda.synchronize()
    for t in [out, gx] + saved + grads:
        assert (t == 7.0).all()
    assert (ws == 0).all()
    assert fwd(d, wsb) == 0 and bwd(d, wsb) == 0                           # and the valid call goes through
    torch.cuda.synchronize()
    assert not (out == 7.0).all() and not (gx == 7.0).all()
    # no rows: the forward has nothing to do, the backward zero-fills every gradient it was asked for
    assert L.vllm_clip_layer_forward_train(ctypes.byref(d), P(x), 0, S, P(out), ctypes.byref(sv), None, 0, stream()) == 0
    assert L.vllm_clip_layer_backward(ctypes.byref(d), P(x), 0, S, P(gout), ctypes.byref(sv), P(gx), ctypes.byref(gs), None, 0, stream()) == 0
    torch.cuda.synchronize()
    for t in grads:
        assert (t == 0).all()


# ---- 8: the caller-workspace contract of the three new workspace-taking entries ----------------------------------------------------
@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
def test_layernorm_backward_res_partials(rows, C):
    L = _lib.lib()
    need = L.vllm_layernorm_backward_res_workspace_bytes(rows, C)
    assert need > 0
    x, gy, gres, w = I.norm_case(rows, C, device=DEV)

    def run(W):
        ws, n = W.take(need)
        gx, gw, gb = WC.nan_bf16(rows, C), WC.nan_bf16(C), WC.nan_bf16(C)
        _lib.check(L.vllm_layernorm_backward_res_bf16(P(x), C, P(gy), C, P(w), I.EPS, rows, C, P(gx), C, P(gres), C, P(gw), P(gb), P(ws), n,
                                                      stream()), "vllm_layernorm_backward_res_bf16")
        return dict(gx=gx, gw=gw, gb=gb)

    base = WC.three_runs(run, widest_row_bytes=C * 4)[0][0]
    rx, rw, rb, mx, mw, mb = I.ln_bwd_ref(x, gy, w, gres)
    assert I.excess_ulp(base["gx"], rx, mx) <= 1.0 and I.excess_ulp(base["gw"], rw, mw) <= 1.0 and I.excess_ulp(base["gb"], rb, mb) <= 1.0


WS_LAYER_CASES = [I.LAYER_CONFIGS[0], I.LAYER_CONFIGS[1], (128, 2, 256, 4, 256, "quick_gelu"),   # B S = 1024: the stream-K scratch is carved
                  I.LAYER_CONFIGS[2]]                                                            # hidden 1024, 1154 rows: the 8-phase GEMM
WS_FROZEN = {"all": None, "norms": {"layer_norm1.weight", "layer_norm1.bias", "layer_norm2.weight", "layer_norm2.bias"},
             "fc2_bias_alone": {"mlp.fc2.bias"}}
WS_LAYER_RUNS = [(0, "all"), (1, "all"), (2, "all"), (3, "all"), (0, "norms"), (0, "fc2_bias_alone")]


@pytest.mark.parametrize("idx,frozen", WS_LAYER_RUNS)
def test_clip_layer_train_workspace(idx, frozen, monkeypatch):
    """The forward's [sk][xn] and everything the backward carves behind them; every request of the module is a fresh hostile buffer of
    exactly the bytes the query answers, at the least alignment, between guard bytes: the same bits as a clean run."""
    cfg = WS_LAYER_CASES[idx]
    hidden, heads, inter, B, S, act = cfg
    trainable = WS_FROZEN[frozen]
    layer, params = build_layer(cfg, seed=idx)
    x, gout = I.make_io(B, S, hidden, seed=idx, device=DEV)
    need_x = trainable is None
    for n, p in layer.named_parameters():
        p.requires_grad_(trainable is None or n in trainable)
    L = _lib.lib()

    def run(W):
        y, g, gx = native_run(layer, x, gout, need_x)
        return dict(y=y, gx=gx, **g)

    outs, spaces = WC.three_runs(run, widest_row_bytes=max(3 * hidden, inter) * 4, patch=monkeypatch)
    base = outs[0]
    assert len(spaces[0].sizes) == 2, spaces[0].sizes                      # the forward's request and the backward's
    if B * S >= 1024:
        assert min(spaces[0].sizes) >= L.vllm_gemm_scratch_bytes()         # the stream-K scratch is carved
    for p in layer.parameters():
        p.requires_grad_(True)
    y64, g64, gx64 = I.autograd_layer(params, x, gout, heads, act, torch.float64)
    y16, g16, gx16 = I.autograd_layer(params, x, gout, heads, act, torch.bfloat16)
    rows = [("y", y16, y64)] + ([("gx", gx16, gx64)] if need_x else []) + [(n, g16[n], g64[n]) for n in g64 if trainable is None or n in trainable]
    for name, t16, t64 in rows:       # DESIGN section 5's rule, as test_layer_gradients
        rn, rt = I.rel_rms(base[name], t64), I.rel_rms(t16, t64)
        assert rn <= 1.25 * rt, f"{name}: {rn:.4g} > 1.25 x {rt:.4g}"
    for n in g64:
        if trainable is not None and n not in trainable:
            assert base[n] is None, n


@pytest.mark.parametrize("idx", [0, 2])
def test_clip_layer_forward_train_takes_the_head_of_the_workspace(idx):
    """The training forward is served by [sk][xn] alone (layer_train.cpp's layout comment, qkn without bytes; the number is derived here, as in
    test_clip_layer_train_cpu.py): straight through the C ABI with exactly those bytes, hostile and guarded."""
    from visionllm_amd.clip_vit import _SAVED, _fused_params, _layer_desc
    L = _lib.lib()
    cfg = WS_LAYER_CASES[idx]
    hidden, heads, inter, B, S, act = cfg
    layer, _ = build_layer(cfg, seed=idx)
    x, _ = I.make_io(B, S, hidden, seed=idx, device=DEV)
    M = B * S
    a256 = lambda v: (v + 255) & ~255  # noqa: E731
    fwd = (a256(L.vllm_gemm_scratch_bytes()) if M >= 1024 else 0) + a256(M * hidden * 2)
    keep = []
    d = _layer_desc(layer._meta, _fused_params(layer._params()), keep)
    assert 0 < fwd < L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(d), B, S)

    def run(W):
        ws, n = W.take(fwd)
        out = WC.nan_bf16(B, S, hidden)
        saved = [WC.nan_bf16(M, 3 * hidden), WC.nan_bf16(M, hidden), torch.full((B, heads, S), NAN, device=DEV), WC.nan_bf16(M, hidden),
                 WC.nan_bf16(M, inter), WC.nan_bf16(M, inter)]
        sv = _lib.VllmClipLayerSaved(**{k: t.data_ptr() for k, t in zip(_SAVED, saved)})
        _lib.check(L.vllm_clip_layer_forward_train(ctypes.byref(d), P(x), B, S, P(out), ctypes.byref(sv), P(ws), n, stream()),
                   "vllm_clip_layer_forward_train")
        return dict(out=out, **dict(zip(_SAVED, saved)))

    base = WC.three_runs(run, widest_row_bytes=3 * hidden * 2)[0][0]
    with torch.no_grad():
        assert torch.equal(base["out"], layer(x)[0])
    for k, t in base.items():
        assert bool(torch.isfinite(t.float()).all()), k


# ---- 9: the tower from pixels ------------------------------------------------------------------------------------------------------
def test_layernorm_module_under_autograd():
    rows, C = 150, 128
    x, gy, _, w = I.norm_case(rows, C, seed=9, device=DEV)
    b = (0.1 * torch.randn(C, device=DEV)).to(torch.bfloat16)
    x3, gy3 = x.view(3, 50, C), gy.view(3, 50, C)
    norm = _CLIPLayerNorm(C, eps=I.EPS).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(w)
        norm.bias.copy_(b)
        y0 = norm(x3)
    assert y0.grad_fn is None
    y_old = torch.empty_like(x)
    _lib.check(_lib.lib().vllm_layernorm_bf16(P(x), C, P(w), P(b), P(y_old), C, rows, C, I.EPS, stream()))
    assert torch.equal(y0.view(rows, C), y_old)
    xx = x3.detach().requires_grad_(True)
    y = norm(xx)
    assert y.grad_fn is not None and torch.equal(y, y0)
    y.backward(gy3)
    _, gx64, gw64, gb64 = I.autograd_layer_norm(x3, w, b, gy3, torch.float64)
    _, gx16, gw16, gb16 = I.autograd_layer_norm(x3, w, b, gy3, torch.bfloat16)
    for name, a, b_, ref in (("x.grad", xx.grad, gx16, gx64), ("weight.grad", norm.weight.grad, gw16, gw64), ("bias.grad", norm.bias.grad, gb16, gb64)):
        rn, rt = I.rel_rms(a, ref), I.rel_rms(b_, ref)
        print(f"_CLIPLayerNorm C={C} {name}: native {rn:.4g}  torch bf16 {rt:.4g}")
        assert rn <= 1.25 * rt, name
    # a strided input (the pooler's last[:, 0]) and a frozen module: only x.grad, the same bits
    norm.requires_grad_(False)
    norm.weight.grad = norm.bias.grad = None
    wide = torch.zeros(3, 50, 2 * C, device=DEV, dtype=torch.bfloat16)
    wide[..., :C] = x3
    xs = wide.requires_grad_(True)
    norm(xs[..., :C]).backward(gy3)
    assert norm.weight.grad is None and torch.equal(xs.grad[..., :C], xx.grad)


def test_tower_trains_from_pixels():
    model = small_model(90)
    vm = model.vision_model
    torch.manual_seed(91)
    pix = torch.randn(3, 3, 70, 70).to(torch.bfloat16)
    gout = (torch.randn(3, 26, 128) / math.sqrt(128)).to(torch.bfloat16)
    gpool = (torch.randn(3, 128) / math.sqrt(128)).to(torch.bfloat16)
    pd = pix.to(DEV)
    # native_training off (the default): today's output, whatever the grad mode
    with torch.no_grad():
        ref_out = model(pd, output_hidden_states=True)
    out0 = model(pd, output_hidden_states=True)
    assert out0.last_hidden_state.grad_fn is None
    assert all(torch.equal(a, b) for a, b in zip(out0.hidden_states, ref_out.hidden_states)) and torch.equal(out0.pooler_output, ref_out.pooler_output)
    model.native_training = True
    with torch.no_grad():
        out1 = model(pd, output_hidden_states=True)          # grad disabled: the fused encoder still
    assert all(torch.equal(a, b) for a, b in zip(out1.hidden_states, ref_out.hidden_states)) and torch.equal(out1.pooler_output, ref_out.pooler_output)
    out = model(pd, output_hidden_states=True)
    assert len(out.hidden_states) == 3 and all(h.grad_fn is not None for h in out.hidden_states) and out.pooler_output.grad_fn is not None
    assert out.last_hidden_state is out.hidden_states[-1]
    for a, b in zip(out.hidden_states, ref_out.hidden_states):   # the same kernels in the same order at this size: the inference bits
        assert torch.equal(a, b)
    assert torch.equal(out.pooler_output, ref_out.pooler_output)

    # the yardstick: fp64 / bf16 autograd of the restated tower on the CPU (tiny shapes), on the same bf16 values
    sd = {k[len("vision_model."):]: v.detach().cpu() for k, v in model.state_dict().items()}

    def torch_run(dtype):
        p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
        hs, pooled = I.tower(p, pix.to(dtype), 2, 2, 14, "quick_gelu", I.EPS)
        (g2,) = torch.autograd.grad((hs[-2] * gout.to(dtype)).sum(), [hs[-2]], retain_graph=True)      # (checks the loss is what it says)
        assert torch.equal(g2, gout.to(dtype))
        ga = torch.autograd.grad(hs[-2], list(p.values()), gout.to(dtype), retain_graph=True, allow_unused=True)
        gb = torch.autograd.grad(pooled, list(p.values()), gpool.to(dtype), allow_unused=True)
        return hs[-2].detach(), pooled.detach(), dict(zip(p, ga)), dict(zip(p, gb))

    h64, p64, ga64, gb64 = torch_run(torch.float64)
    h16, p16, ga16, gb16 = torch_run(torch.bfloat16)

    def rule(name, nat, t16, t64):
        rn, rt = I.rel_rms(nat.cpu(), t64), I.rel_rms(t16, t64)
        print(f"clip tower  {name:52s} native {rn:.4g}  torch bf16 {rt:.4g}  ratio {rn / rt:.3f}")
        assert rn <= 1.25 * rt, f"{name}: {rn:.4g} > 1.25 x {rt:.4g}"

    rule("hidden_states[-2]", out.hidden_states[-2].detach(), h16, h64)
    rule("pooler_output", out.pooler_output.detach(), p16, p64)
    # loss on hidden_states[-2]: gradients reach the embeddings and pre_layrnorm; the last layer and post_layernorm get none
    out.hidden_states[-2].backward(gout.to(DEV), retain_graph=True)
    named = dict(model.named_parameters())
    reached = {k for k, v in named.items() if v.grad is not None}
    for k in ("embeddings.patch_embedding.weight", "embeddings.class_embedding", "embeddings.position_embedding.weight", "pre_layrnorm.weight",
              "pre_layrnorm.bias"):
        assert "vision_model." + k in reached, k
    for k, v in named.items():
        short = k[len("vision_model."):]
        if short.startswith("encoder.layers.1.") or short.startswith("post_layernorm."):
            assert v.grad is None and ga64[short] is None, k
        else:
            rule(short + ".grad", v.grad.reshape(ga64[short].shape), ga16[short], ga64[short])
    # loss on the pooler: every parameter is reached, post_layernorm included
    for v in named.values():
        v.grad = None
    out.pooler_output.backward(gpool.to(DEV))
    for k in ("post_layernorm.weight", "post_layernorm.bias", "encoder.layers.1.mlp.fc2.weight", "embeddings.patch_embedding.weight"):
        rule(k + ".grad (pooler)", named["vision_model." + k].grad.reshape(gb64[k].shape), gb16[k], gb64[k])
    assert all(v.grad is not None for v in named.values())
    # frozen tower: native_training has nothing to train, the fused encoder runs
    model.requires_grad_(False)
    assert model(pd).last_hidden_state.grad_fn is None
    assert vm.encoder.gradient_checkpointing is False
