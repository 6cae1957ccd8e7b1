"""CPU: the host side of the CLIP layer's training path (no GPU): the restated statements reproduce the HF-made golden hidden states, an
fp32 emulation of the new row-wise kernel and of q' stays inside the GPU tests' bounds at the GPU tests' shapes (so a faithful
implementation can meet them), header / mirrors / exports agree, and every new entry refuses what it cannot serve before any HIP call
(fake non-null pointers: the gates look at values, they dereference nothing)."""
import ast
import ctypes

import numpy as np
import pytest
import torch

import clip_layer_train_inputs as I
from conftest import golden_sd, load_golden
from visionllm_amd import _lib
from visionllm_amd.clip_vit import CLIPVisionModel, _CLIPEncoder, _CLIPEncoderLayer, _CLIPLayerNorm

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def _fill(cls, ints, skip=()):
    d = cls()
    for name, ctype in cls._fields_:
        if name in ints:
            setattr(d, name, ints[name])
        elif ctype is ctypes.c_void_p and name not in skip:
            setattr(d, name, PTR)
    return d


def align256(x):
    return (x + 255) & ~255


# ---- the yardstick is the reference's function ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clip_tiny.npz", "clip_small_d64.npz"])
def test_restated_layer_reproduces_the_golden_hidden_states(name):
    g = load_golden(name)
    cfg = ast.literal_eval(str(g["cfg"]))
    sd = golden_sd(g)
    prefix = "vision_model." if any(k.startswith("vision_model.") for k in sd) else ""
    ref = g["hidden_states"]
    assert ref.shape[0] == cfg["num_hidden_layers"] + 1
    h = torch.from_numpy(ref[0])
    for i in range(cfg["num_hidden_layers"]):
        pre = f"{prefix}encoder.layers.{i}."
        p = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        assert set(p) == set(I.make_params(64, 128)), "the restatement's parameter names are HF's"
        h = I.layer(p, h, cfg["num_attention_heads"], cfg["hidden_act"], cfg["layer_norm_eps"])
        np.testing.assert_allclose(h.numpy(), ref[i + 1], rtol=2e-5, atol=2e-5)
    # ... and so is the whole tower from pixels (a post_layernorm the fixture does not hold is made up: only the hidden states are compared)
    C = cfg["hidden_size"]
    sd2 = dict(sd)
    sd2.setdefault(prefix + "post_layernorm.weight", torch.ones(C))
    sd2.setdefault(prefix + "post_layernorm.bias", torch.zeros(C))
    hs, pooled = I.tower(sd2, torch.from_numpy(g["pixel_values"]), cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["patch_size"],
                         cfg["hidden_act"], cfg["layer_norm_eps"], prefix)
    assert len(hs) == ref.shape[0] and pooled.shape == (ref.shape[1], C)
    for i, t in enumerate(hs):
        np.testing.assert_allclose(t.numpy(), ref[i], rtol=2e-5, atol=2e-5)


# ---- the bounds are ones a faithful implementation meets ------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
@pytest.mark.parametrize("with_res", [False, True])
def test_layernorm_backward_emulation_meets_the_bounds(rows, C, with_res):
    x, gy, gres, w = I.norm_case(rows, C)
    gres = gres if with_res else None
    gx, gw, gb = I.emulate_ln_bwd(x, gy, w, gres)
    rx, rw, rb, mx, mw, mb = I.ln_bwd_ref(x, gy, w, gres)
    ex, ew, eb = I.excess_ulp(gx, rx, mx), I.excess_ulp(gw, rw, mw), I.excess_ulp(gb, rb, mb)
    print(f"layernorm bwd emulation {rows}x{C} res={with_res}: grad_x {ex:.3f} grad_w {ew:.3f} grad_b {eb:.3f} of the bound")
    assert ex <= 1.0 and ew <= 1.0 and eb <= 1.0
    # the restated norm's own fp64 autograd is the same function
    if gres is None:
        _, ax, aw, ab = I.autograd_layer_norm(x, w, torch.zeros_like(w), gy, torch.float64)
        assert torch.allclose(ax, rx, rtol=1e-9, atol=1e-12) and torch.allclose(aw, rw, rtol=1e-9, atol=1e-12)
        assert torch.allclose(ab, rb, rtol=1e-9, atol=1e-12)


def test_quick_gelu_grad_is_bounded_and_its_emulation_is_exact_enough():
    h = torch.linspace(-30.0, 30.0, 2_000_001, dtype=torch.float64)
    q = I.quick_gelu_grad_ref(h)
    assert q.abs().max().item() <= I.QUICK_GELU_GRAD_MAX
    assert q.abs().max().item() > 1.09                                  # (the constant is tight: the GPU test's 1.2 has room)
    # autograd of the restated activation is the same function
    hh = h[::1000].clone().requires_grad_(True)
    I.quick_gelu(hh).sum().backward()
    assert torch.allclose(hh.grad, I.quick_gelu_grad_ref(hh.detach()), rtol=1e-12, atol=1e-14)
    # the epilogue's fp32 walk against fp64: the exponent's argument reaches 1.702 log2(e) 30 = 74 on this grid and carries half an fp32 ulp
    # of it, 2^-18 at most, so 2^x -- and with it s and q', both at most 1.1 -- is off by 2^-18 ln 2 relative plus a few fp32 roundings:
    # inside 2^-17, far below bf16 resolution (2^-9)
    e = (I.emulate_quick_gelu_grad(h.float()).double() - I.quick_gelu_grad_ref(h.float())).abs().max().item()
    assert e < 2.0 ** -17, e


# ---- header, mirrors, exports ---------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("vllm_layernorm_backward_res_workspace_bytes", "vllm_layernorm_backward_res_bf16", "vllm_gemm_bf16_quick_gelu_save",
               "vllm_gemm_bf16_quick_gelu_bwd", "vllm_clip_layer_train_sizeof", "vllm_clip_layer_saved_sizeof", "vllm_clip_layer_grads_sizeof",
               "vllm_clip_layer_backward_workspace_bytes", "vllm_clip_layer_forward_train", "vllm_clip_layer_backward")


def test_header_mirrors_and_exports_agree():
    L = _lib.lib()
    protos = _lib.parse_header()
    for n in NEW_ENTRIES:
        assert n in protos and hasattr(L, n), n
    _lib.check_struct_layouts()
    assert L.vllm_clip_layer_train_sizeof() == ctypes.sizeof(_lib.VllmClipLayerTrain) == 24 + 12 * 8
    assert L.vllm_clip_layer_saved_sizeof() == ctypes.sizeof(_lib.VllmClipLayerSaved) == 6 * 8
    assert L.vllm_clip_layer_grads_sizeof() == ctypes.sizeof(_lib.VllmClipLayerGrads) == 12 * 8
    assert [n for n, _ in _lib.VllmClipLayerTrain._fields_[5:]] == [n for n, _ in _lib.VllmClipLayerGrads._fields_]      # parameter order
    assert L.vllm_abi_version() == _lib.header_abi_version() == 2
    assert len(protos["vllm_layernorm_backward_res_bf16"][1]) == 17
    assert len(protos["vllm_gemm_bf16_quick_gelu_save"][1]) == 13 and len(protos["vllm_gemm_bf16_quick_gelu_bwd"][1]) == 14


def test_workspace_queries_need_no_gpu():
    L = _lib.lib()
    for rows, C in I.NORM_SHAPES:
        b = L.vllm_layernorm_backward_res_workspace_bytes(rows, C)
        assert b > 0 and b % (2 * 4 * C) == 0 and b // (2 * 4 * C) <= rows                # two sums per row range, never more ranges than rows
        assert b == 2 * L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 1)               # the same walk
    assert L.vllm_layernorm_backward_res_workspace_bytes(10, 200, ) == -1                 # C % 64
    assert L.vllm_layernorm_backward_res_workspace_bytes(10, 8256) == -1                  # C > 8192
    assert L.vllm_layernorm_backward_res_workspace_bytes(-1, 128) == -1
    assert L.vllm_layernorm_backward_res_workspace_bytes(0, 128) >= 0
    d = _fill(_lib.VllmClipLayerTrain, dict(hidden=128, heads=2, inter=256, act=_lib.EPI_QUICK_GELU, eps=1e-5))
    small = L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(d), 2, 37)
    big = L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(d), 8, 577)
    assert 0 < small < big
    assert L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(d), 0, 37) >= 0


# ---- refusals before any HIP call ----------------------------------------------------------------------------------------------------
def _ws_entries():
    L = _lib.lib()
    p = vp(PTR)
    E = []

    def add(name, need, call):
        E.append(pytest.param(need, call, id=name))

    for rows, C in ((300, 128), (64, 1280)):
        add(f"layernorm_backward_res_{rows}x{C}", L.vllm_layernorm_backward_res_workspace_bytes(rows, C),
            lambda w, n, rows=rows, C=C: L.vllm_layernorm_backward_res_bf16(p, C, p, C, p, 1e-5, rows, C, p, C, p, C, p, p, vp(w), n, None))
    sv = _fill(_lib.VllmClipLayerSaved, {})
    gr = _fill(_lib.VllmClipLayerGrads, {})
    for act, B, S in ((_lib.EPI_QUICK_GELU, 2, 37), (_lib.EPI_GELU, 3, 65), (_lib.EPI_QUICK_GELU, 4, 256)):
        ld = _fill(_lib.VllmClipLayerTrain, dict(hidden=128, heads=2, inter=256, act=act, eps=1e-5))
        tag = f"act{act}_{B}x{S}"
        add(f"clip_layer_backward_{tag}", L.vllm_clip_layer_backward_workspace_bytes(ctypes.byref(ld), B, S),
            lambda w, n, ld=ld, B=B, S=S: L.vllm_clip_layer_backward(ctypes.byref(ld), p, B, S, p, ctypes.byref(sv), p, ctypes.byref(gr), vp(w), n,
                                                                     None))
        # forward: [sk][xn] (layer_train.cpp, "forward: [sk][xn][qkn]", qkn without bytes): the stream-K scratch from 1024 rows on, LN1(x) / LN2(x1) [M, C] bf16; every
        # piece rounded up to 256 bytes
        M, C = B * S, 128
        fwd = (align256(L.vllm_gemm_scratch_bytes()) if M >= 1024 else 0) + align256(M * C * 2)
        add(f"clip_layer_forward_train_{tag}", fwd,
            lambda w, n, ld=ld, B=B, S=S: L.vllm_clip_layer_forward_train(ctypes.byref(ld), p, B, S, p, ctypes.byref(sv), vp(w), n, None))
    return E


try:
    WS_ENTRIES, _NOT_BUILT = _ws_entries(), None
except (RuntimeError, OSError, AttributeError) as e:      # (the library is not built: the file still collects, the test below says why)
    WS_ENTRIES, _NOT_BUILT = [], e


def test_every_workspace_entry_has_its_case():
    assert _NOT_BUILT is None, _NOT_BUILT
    assert len(WS_ENTRIES) == 8
    by_id = {e.id: e.values[0] for e in WS_ENTRIES}
    for tag in ("act2_2x37", "act1_3x65", "act2_4x256"):
        assert 0 < by_id[f"clip_layer_forward_train_{tag}"] < by_id[f"clip_layer_backward_{tag}"], tag
    assert by_id["clip_layer_forward_train_act2_2x37"] == 74 * 128 * 2
    assert by_id["clip_layer_forward_train_act2_4x256"] == 4096 + 320 * 262144 + 1024 * 128 * 2


def refused(rc, word):
    msg = _lib.lib().vllm_last_error().decode()
    assert rc == EINVAL and word in msg, (rc, msg)


@pytest.mark.parametrize("need,call", WS_ENTRIES)
def test_short_misaligned_and_null_workspaces_are_refused(need, call):
    assert need > 0, "the case is meant to need a workspace"
    refused(call(PTR, need - 1), "workspace")
    refused(call(PTR + 8, need), "workspace")
    refused(call(PTR + 8, need + 4096), "workspace")      # room to spare does not excuse the pointer
    refused(call(0, need), "workspace")


def test_layernorm_backward_res_refuses_bad_arguments():
    L = _lib.lib()
    p, off = vp(PTR), vp(PTR + 8)
    big = 1 << 30

    def call(x=p, ldx=128, gy=p, ldg=128, w=p, rows=300, C=128, gx=p, ldgx=128, gres=p, ldgr=128, gw=p, gb=p):
        return L.vllm_layernorm_backward_res_bf16(x, ldx, gy, ldg, w, 1e-5, rows, C, gx, ldgx, gres, ldgr, gw, gb, p, big, None)

    refused(call(C=200, ldx=200, ldg=200, ldgx=200, ldgr=200), "multiple of 64")
    refused(call(C=8256, ldx=8256, ldg=8256, ldgx=8256, ldgr=8256), "8192")
    refused(call(rows=-1), "layernorm_backward_res")
    refused(call(x=None), "aligned")
    refused(call(x=off), "aligned")
    refused(call(gy=off), "aligned")
    refused(call(w=off), "aligned")
    refused(call(gx=off), "aligned")
    refused(call(gres=off), "aligned")
    refused(call(gx=None), "grad_res needs grad_x")
    refused(call(ldx=120), "row strides")
    refused(call(ldg=132), "row strides")
    refused(call(ldgx=64), "row strides")
    refused(call(ldgr=100), "row strides")
    refused(call(gw=vp(PTR + 1)), "misaligned")
    refused(call(gb=vp(PTR + 1)), "misaligned")


def test_quick_gelu_entries_refuse_bad_arguments():
    L = _lib.lib()
    p, off8, off4 = vp(PTR), vp(PTR + 8), vp(PTR + 4)
    M, N, K = 300, 256, 128

    def save(X=p, W=p, b=p, Y=p, pre=p, M=M, N=N, K=K, ldx=K, ldw=K, ldy=N, force=0):
        return L.vllm_gemm_bf16_quick_gelu_save(X, W, b, Y, pre, M, N, K, ldx, ldw, ldy, force, None)

    def bwd(X=p, W=p, b=None, Y=p, M=M, N=N, K=K, ldx=K, ldw=K, ldy=N, force=0, res=p, ldr=N):
        return L.vllm_gemm_bf16_quick_gelu_bwd(X, W, b, Y, M, N, K, ldx, ldw, ldy, force, res, ldr, None)

    for fn in (save, bwd):
        refused(fn(K=100, ldx=104, ldw=104), "K=100")
        refused(fn(N=254), "N=254")
        refused(fn(M=-1), "bad dims")
        refused(fn(X=off8), "aligned")
        refused(fn(W=off8), "aligned")
        refused(fn(Y=off4), "aligned")
        refused(fn(ldx=K + 4), "aligned")
        refused(fn(X=None), "null pointer")
        refused(fn(force=2), "force_bits")                  # an epilogue number is not a force bit
        refused(fn(force=0x400), "4-wave")                  # the schedule that is not built
    refused(save(pre=None), "null pointer")
    refused(save(pre=off4), "pre-activation")
    refused(save(b=off4), "bias")
    refused(bwd(b=p), "no bias")
    refused(bwd(res=None), "no bias")                       # (the same gate: the saved pre-activation is required)
    refused(bwd(res=off4), "no bias")
    refused(bwd(ldr=N + 2), "no bias")
    # the public epilogue numbers stay what they were: 7 is still nobody's (the two new epilogues are internal numbers)
    assert L.vllm_gemm_bf16(p, p, None, p, M, N, K, K, K, N, 7, None, p, N, 0, None) == EINVAL
    assert b"unknown epilogue 7" in L.vllm_last_error()


def test_clip_layer_entries_refuse_bad_arguments():
    L = _lib.lib()
    p, off = vp(PTR), vp(PTR + 8)
    big = 1 << 40
    sv = _fill(_lib.VllmClipLayerSaved, {})
    gr = _fill(_lib.VllmClipLayerGrads, {})
    base = dict(hidden=128, heads=2, inter=256, act=_lib.EPI_QUICK_GELU, eps=1e-5)

    def both(d, word, B=2, S=37, x=p, saved=sv, grads=gr, gx=p):
        dd = ctypes.byref(d) if d is not None else None
        refused(L.vllm_clip_layer_forward_train(dd, x, B, S, p, ctypes.byref(saved), p, big, None), word)
        refused(L.vllm_clip_layer_backward(dd, x, B, S, p, ctypes.byref(saved), gx, ctypes.byref(grads), p, big, None), word)
        if d is not None and word not in ("aligned", "saved"):
            assert L.vllm_clip_layer_backward_workspace_bytes(dd, B, S) == -1

    both(None, "null descriptor")
    both(_fill(_lib.VllmClipLayerTrain, dict(base, heads=4)), "head_dim")
    both(_fill(_lib.VllmClipLayerTrain, dict(base, heads=3)), "heads")
    both(_fill(_lib.VllmClipLayerTrain, dict(base, inter=250)), "multiples of 64")
    both(_fill(_lib.VllmClipLayerTrain, dict(base, hidden=8320, heads=65)), "8192")
    both(_fill(_lib.VllmClipLayerTrain, dict(base, act=_lib.EPI_BIAS)), "act")
    both(_fill(_lib.VllmClipLayerTrain, dict(base, act=7)), "act")
    both(_fill(_lib.VllmClipLayerTrain, base, skip=("norm2_b",)), "missing")
    both(_fill(_lib.VllmClipLayerTrain, base), "B=", B=-1)
    both(_fill(_lib.VllmClipLayerTrain, base), "B=", S=0)
    mis = _fill(_lib.VllmClipLayerTrain, base)
    mis.fc1_b = PTR + 8
    both(mis, "aligned")
    ok = _fill(_lib.VllmClipLayerTrain, base)
    both(ok, "aligned", x=off)
    both(ok, "saved", saved=_fill(_lib.VllmClipLayerSaved, {}, skip=("lse",)))
    bad_sv = _fill(_lib.VllmClipLayerSaved, {})
    bad_sv.h1 = PTR + 8
    both(ok, "aligned", saved=bad_sv)
    # the backward's own gates: a bias gradient without its weight's, a misaligned gradient, a null table
    lone = _fill(_lib.VllmClipLayerGrads, {}, skip=("fc2_w",))
    refused(L.vllm_clip_layer_backward(ctypes.byref(ok), p, 2, 37, p, ctypes.byref(sv), p, ctypes.byref(lone), p, big, None), "bias gradient")
    mg = _fill(_lib.VllmClipLayerGrads, {})
    mg.norm1_b = PTR + 8
    refused(L.vllm_clip_layer_backward(ctypes.byref(ok), p, 2, 37, p, ctypes.byref(sv), p, ctypes.byref(mg), p, big, None), "aligned")
    refused(L.vllm_clip_layer_backward(ctypes.byref(ok), p, 2, 37, p, ctypes.byref(sv), off, ctypes.byref(gr), p, big, None), "aligned")
    refused(L.vllm_clip_layer_backward(ctypes.byref(ok), p, 2, 37, p, ctypes.byref(sv), p, None, p, big, None), "gradient table")


# ---- the modules ---------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from types import SimpleNamespace
    base = dict(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, image_size=28, patch_size=14,
                layer_norm_eps=1e-5, hidden_act="quick_gelu", output_hidden_states=False, use_return_dict=True)
    base.update(kw)
    return SimpleNamespace(**base)


def test_cpu_inputs_masks_and_attention_maps_raise():
    layer = _CLIPEncoderLayer(_cfg())
    x = torch.zeros(1, 5, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="CUDA"):
        layer(x)
    with pytest.raises(RuntimeError, match="CUDA"):
        _CLIPEncoder(_cfg())(x)
    with pytest.raises(RuntimeError, match="CUDA"):
        _CLIPLayerNorm(128)(x)
    with pytest.raises(NotImplementedError, match="mask"):
        layer(x, attention_mask=torch.zeros(1, 1, 5, 5))
    with pytest.raises(NotImplementedError, match="mask"):
        layer(x, None, torch.zeros(1, 1, 5, 5))
    with pytest.raises(NotImplementedError, match="attention maps"):
        layer(x, output_attentions=True)
    drop = _CLIPEncoderLayer(_cfg(attention_dropout=0.1)).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        drop(x)


def test_defaults_follow_hf_and_keep_todays_behaviour():
    model = CLIPVisionModel(_cfg())
    assert model.native_training is False
    assert model.vision_model.encoder.gradient_checkpointing is False
    assert isinstance(model.vision_model.pre_layrnorm, torch.nn.LayerNorm) and isinstance(model.vision_model.post_layernorm, torch.nn.LayerNorm)
    names = {n for n, _ in model.named_parameters()}
    assert "vision_model.encoder.layers.1.self_attn.q_proj.bias" in names and "vision_model.post_layernorm.weight" in names
    assert len(names) == 3 + 2 + 2 * 16 + 2                             # embeddings, pre-LN, 16 per layer, post-LN: nothing added
