"""CPU: the host side of the InternViT layer's training path (no GPU): an fp32 emulation of the two new row-wise kernels stays inside
the GPU tests' per-element bounds at the GPU tests' shapes (so a faithful implementation can meet them), the workspace / sizeof queries
answer without a device, and CPU tensors and the dropout / drop-path cases raise."""
import ctypes

import pytest
import torch

import vit_layer_train_inputs as I
from visionllm_amd import _lib
from visionllm_amd.intern_vit import InternRMSNorm, InternVisionConfig, InternVisionEncoder, InternVisionEncoderLayer


@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
@pytest.mark.parametrize("with_res", [False, True])
def test_rmsnorm_backward_emulation_meets_the_bounds(rows, C, with_res):
    x, gy, gres, w = I.norm_case(rows, C)
    gres = gres if with_res else None
    gx, gw = I.emulate_rms_bwd(x, gy, w, gres)
    rx, rw, mx, mw = I.rms_bwd_ref(x, gy, w, gres)
    assert I.excess_ulp(gx, rx, mx) <= 1.0
    assert I.excess_ulp(gw, rw, mw) <= 1.0
    # the restated norm's own fp64 autograd is the same function
    _, ax, aw = I.autograd_rms_norm(x, w, gy, torch.float64)
    if gres is None:
        assert torch.allclose(ax, rx, rtol=1e-9, atol=1e-12) and torch.allclose(aw, rw, rtol=1e-9, atol=1e-12)


def test_rounded_xhat_in_grad_w_would_miss_the_bound():
    """Why grad_w sums grad_y * xhat with the UNROUNDED fp32 xhat: the forward's bf16(x r) in its place is outside the bound."""
    x, gy, _, w = I.norm_case(300, 128)
    _, rw, _, mw = I.rms_bwd_ref(x, gy, w)
    r = torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + I.EPS)
    xh16 = (x.float() * r).to(torch.bfloat16).float()
    assert I.excess_ulp((gy.float() * xh16).sum(0).to(torch.bfloat16), rw, mw) > 1.0


@pytest.mark.parametrize("rows,C", I.NORM_SHAPES)
def test_layerscale_backward_emulation_meets_the_bounds(rows, C):
    go, y, _, w = I.norm_case(rows, C, seed=1)
    ls = (0.1 * w.float()).to(torch.bfloat16)
    gy, gls = I.emulate_ls_bwd(go, y, ls)
    ry, rls, mls = I.ls_bwd_ref(go, y, ls)
    assert I.excess_ulp(gy, ry, torch.zeros_like(ry)) <= 1.0
    assert I.excess_ulp(gls, rls, mls) <= 1.0


def test_workspace_and_sizeof_queries_need_no_gpu():
    L = _lib.lib()
    _lib.check_struct_layouts()
    assert L.vllm_vit_layer_train_sizeof() == ctypes.sizeof(_lib.VllmVitLayerTrain) == 16 + 14 * 8
    assert L.vllm_vit_layer_saved_sizeof() == ctypes.sizeof(_lib.VllmVitLayerSaved) == 8 * 8
    assert L.vllm_vit_layer_grads_sizeof() == ctypes.sizeof(_lib.VllmVitLayerGrads) == 14 * 8
    for rows, C in I.NORM_SHAPES:
        b1, b2 = L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 1), L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 2)
        assert b1 > 0 and b1 % (4 * C) == 0 and b2 == 2 * b1
        assert b1 // (4 * C) <= rows                      # never more blocks than rows
        assert L.vllm_layerscale_backward_workspace_bytes(rows, C) == b1
    assert L.vllm_rmsnorm_backward_workspace_bytes(10, 100, 1) == -1      # C % 8
    assert L.vllm_rmsnorm_backward_workspace_bytes(10, 128, 3) == -1      # G
    assert L.vllm_rmsnorm_backward_workspace_bytes(0, 128, 1) >= 0
    one = ctypes.c_void_p(1 << 20)
    ptrs = {n: one for n, _ in _lib.VllmVitLayerTrain._fields_[4:]}
    d = _lib.VllmVitLayerTrain(hidden=128, heads=2, inter=256, eps=1e-6, **ptrs)
    small = L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), 2, 37)
    big = L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), 8, 577)
    assert 0 < small < big
    d.heads = 4                                            # head_dim 32
    assert L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), 2, 37) == -1
    assert b"head_dim" in L.vllm_last_error()
    d.heads, d.inter = 2, 250
    assert L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), 2, 37) == -1


def _cfg(**kw):
    return InternVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2, **kw)


def test_cpu_and_non_bf16_inputs_raise():
    layer = InternVisionEncoderLayer(_cfg())
    with pytest.raises(RuntimeError, match="CUDA"):
        layer(torch.zeros(1, 5, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="CUDA"):
        InternVisionEncoder(_cfg())(torch.zeros(1, 5, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="CUDA"):
        InternRMSNorm(128)(torch.zeros(5, 128, dtype=torch.bfloat16, requires_grad=True))


@pytest.mark.parametrize("kw,rate", [(dict(dropout=0.1), 0.0), (dict(attention_dropout=0.1), 0.0), (dict(), 0.2)])
def test_dropout_and_drop_path_are_refused_in_training_mode(kw, rate):
    layer = InternVisionEncoderLayer(_cfg(**kw), drop_path_rate=rate)
    layer.train()
    with pytest.raises(NotImplementedError, match="drop"):
        layer(torch.zeros(1, 5, 128, dtype=torch.bfloat16))
    layer.eval()                                           # inference mode: the rates are inert, the device check is next
    with pytest.raises(RuntimeError, match="CUDA"):
        layer(torch.zeros(1, 5, 128, dtype=torch.bfloat16))


def test_encoder_spreads_the_drop_path_rate_like_the_reference():
    enc = InternVisionEncoder(InternVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=3,
                                                 drop_path_rate=0.2))
    assert [round(l.drop_path_rate, 6) for l in enc.layers] == [0.0, 0.1, 0.2]      # modeling_intern_vit.py:226-229
    assert enc.gradient_checkpointing is True
