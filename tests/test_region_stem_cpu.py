"""CPU: the native region-encoder route's ABI (symbols, struct mirrors), its refusals before any launch, and the two identities its
pooling rests on -- the suffix-sum weight rule and the fold of the mean over levels into the weights -- against the module's own
statements in fp64.  Only refused calls reach the library, with fake non-null pointers: nothing touches a device."""
import ctypes

import pytest
import torch

import region_stem_inputs as I
from visionllm_amd import _lib
from visionllm_amd import region_encoder as A

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null

NEW_ENTRIES = ("vllm_region_encoder_sizeof", "vllm_region_encoder_saved_sizeof", "vllm_region_encoder_grads_sizeof",
               "vllm_region_encoder_workspace_bytes", "vllm_region_encoder_forward", "vllm_region_encoder_backward",
               "vllm_region_encoder_calls", "vllm_region_encoder_wgrad_launches", "vllm_layernorm_gelu_bf16", "vllm_region_im2col_bf16",
               "vllm_region_pool_weights_f32", "vllm_region_pool_bf16", "vllm_region_outer_bf16")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def _desc(**over):
    ints = dict(hidden=256, embed=64, out_dim=64, patch=14, n=3, H=56, W=84, levels=3, points=37, pixel_is_f32=0, eps=1e-6)
    ints.update(over)
    d = _lib.VllmRegionEncoder(**ints)
    for k in _lib.REGION_PARAMS:
        setattr(d, k, PTR)
    for l in range(d.levels if 0 <= d.levels <= 4 else 0):
        d.level[l], d.level_row_stride[l], d.level_image_stride[l] = PTR, d.embed, d.embed * 24
    return d


def _saved():
    return _lib.VllmRegionEncoderSaved(**{n: PTR for n, _ in _lib.VllmRegionEncoderSaved._fields_})


def _grads():
    g = _lib.VllmRegionEncoderGrads(**{k: PTR for k in _lib.REGION_PARAMS})
    g.level[1] = PTR
    return g


def _forward(d, ws, nbytes, sv=None):
    sv = sv or _saved()
    return _lib.lib().vllm_region_encoder_forward(ctypes.byref(d), vp(PTR), vp(PTR), vp(PTR), vp(PTR), vp(PTR), ctypes.byref(sv), vp(ws), nbytes, None)


def _backward(d, ws, nbytes, g=None):
    sv, g = _saved(), g or _grads()
    return _lib.lib().vllm_region_encoder_backward(ctypes.byref(d), vp(PTR), vp(PTR), vp(PTR), ctypes.byref(sv), ctypes.byref(g), vp(ws), nbytes, None)


def refused(rc, word):
    msg = _lib.lib().vllm_last_error().decode()
    assert rc == EINVAL and word in msg, (rc, msg)


def test_header_mirrors_and_exports_agree():
    L = _lib.lib()
    protos = _lib.parse_header()
    for n in NEW_ENTRIES:
        assert n in protos and hasattr(L, n), n
    _lib.check_struct_layouts()
    assert L.vllm_region_encoder_sizeof() == ctypes.sizeof(_lib.VllmRegionEncoder) == 12 * 4 + 12 * 8 + 3 * 4 * 8
    assert L.vllm_region_encoder_saved_sizeof() == ctypes.sizeof(_lib.VllmRegionEncoderSaved) == 9 * 8
    assert L.vllm_region_encoder_grads_sizeof() == ctypes.sizeof(_lib.VllmRegionEncoderGrads) == 16 * 8
    assert [n for n, _ in _lib.VllmRegionEncoder._fields_[12:24]] == [n for n, _ in _lib.VllmRegionEncoderGrads._fields_[:12]] == list(_lib.REGION_PARAMS)
    assert L.vllm_abi_version() == _lib.header_abi_version() == 2
    assert len(protos["vllm_region_encoder_forward"][1]) == 10 and len(protos["vllm_region_encoder_backward"][1]) == 9
    assert len(protos["vllm_layernorm_gelu_bf16"][1]) == 10


def test_workspace_query_needs_no_gpu_and_refuses_bad_descriptors():
    L = _lib.lib()
    small = L.vllm_region_encoder_workspace_bytes(ctypes.byref(_desc()))
    big = L.vllm_region_encoder_workspace_bytes(ctypes.byref(_desc(n=16, H=336, W=336, embed=1024, out_dim=4096, points=2304)))
    assert 0 < small < big and small % 256 == 0
    assert big > L.vllm_gemm_scratch_bytes()                     # 16 x 24 x 24 rows: the GEMMs get their stream-K scratch
    assert L.vllm_region_encoder_workspace_bytes(ctypes.byref(_desc(n=0))) >= 0
    for over, word in ((dict(hidden=192), "hidden"), (dict(hidden=64), "hidden"), (dict(embed=96), "embed"), (dict(out_dim=100), "out_dim"),
                       (dict(H=60), "multiples of patch"), (dict(W=85), "multiples of patch"), (dict(patch=7), "even"), (dict(levels=5), "levels"),
                       (dict(levels=0), "levels"), (dict(n=-1), "regions"), (dict(H=14 * 80, W=14 * 80), "4096"), (dict(pixel_is_f32=2), "pixel_is_f32")):
        assert L.vllm_region_encoder_workspace_bytes(ctypes.byref(_desc(**over))) == -1, over
        assert word in L.vllm_last_error().decode(), (over, L.vllm_last_error())
    assert L.vllm_region_encoder_workspace_bytes(None) == -1


@pytest.mark.parametrize("call", [_forward, _backward], ids=["forward", "backward"])
@pytest.mark.parametrize("shape", [dict(), dict(n=16, H=336, W=336, embed=1024, out_dim=4096, points=2304)], ids=["small", "model"])
def test_short_misaligned_and_null_workspaces_are_refused(call, shape):
    d = _desc(**shape)
    need = _lib.lib().vllm_region_encoder_workspace_bytes(ctypes.byref(d))
    assert need > 0
    refused(call(d, PTR, need - 1), "workspace")
    refused(call(d, PTR + 8, need), "workspace")                 # 16 bytes is the stated alignment: one step below it
    refused(call(d, PTR + 8, need + 4096), "workspace")          # room to spare does not excuse the pointer
    refused(call(d, 0, need), "workspace")


def test_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    big = 1 << 40
    for over, word in ((dict(hidden=192), "hidden"), (dict(embed=96), "embed"), (dict(H=60), "multiples of patch"), (dict(levels=5), "levels")):
        refused(_forward(_desc(**over), PTR, big), word)
        refused(_backward(_desc(**over), PTR, big), word)
    d = _desc()
    d.up_w = PTR + 8
    refused(_forward(d, PTR, big), "parameter")
    d = _desc()
    d.level_row_stride[1] = 68
    refused(_forward(d, PTR, big), "level 1")
    d = _desc()
    d.level[2] = PTR + 2
    refused(_forward(d, PTR, big), "level 2")
    sv = _saved()
    sv.pre2 = None
    refused(_forward(_desc(), PTR, big, sv), "saved")
    g = _grads()
    g.conv3_w = None                                             # conv3_b stays: a bias gradient needs its weight's pointer
    refused(_backward(_desc(), PTR, big, g), "bias gradient")
    g = _grads()
    g.level[3] = PTR                                             # the descriptor has three levels
    refused(_backward(_desc(), PTR, big, g), "level 3")
    p = vp(PTR)
    refused(L.vllm_layernorm_gelu_bf16(p, 100, p, p, p, p, 7, 100, 1e-6, None), "multiple of 64")
    refused(L.vllm_layernorm_gelu_bf16(p, 60, p, p, p, p, 7, 64, 1e-6, None), "ldx")
    refused(L.vllm_layernorm_gelu_bf16(vp(PTR + 8), 64, p, p, p, p, 7, 64, 1e-6, None), "aligned")
    refused(L.vllm_region_im2col_bf16(p, p, 0, p, 2, 56, 84, 14, 192, None), "Kpad")
    refused(L.vllm_region_im2col_bf16(p, p, 0, p, 2, 57, 84, 14, 256, None), "multiples")
    refused(L.vllm_region_pool_weights_f32(p, p, p, 2, 5, 4, 6, 37, None), "bad sizes")
    refused(L.vllm_region_outer_bf16(p, p, p, 2, 24, 60, None), "bad sizes")


# ---- Python: the switch and its refusals ---------------------------------------------------------------------------------------------------
def _enc(hidden=256, embed=64, out=64, patch=14, pool="grid_sample"):
    enc = A.RegionEncoder(hidden_dim=hidden, embed_dim=embed, out_dim=out, patch_size=patch, mask_pool_type=pool).to(torch.bfloat16)
    enc.native_branch = True
    return enc


def _args(n=2, H=56, W=84, embed=64, levels=3, patch=14):
    hw = (H // patch) * (W // patch)
    return (torch.zeros(n, 3, H, W, dtype=torch.bfloat16), torch.ones(n, 1, H, W, dtype=torch.bfloat16),
            [torch.zeros(n, hw, embed, dtype=torch.bfloat16) for _ in range(levels)])


def test_the_switch_is_a_class_level_default_that_is_off():
    assert A.RegionEncoder.native_branch is False
    enc = A.RegionEncoder(hidden_dim=32, embed_dim=16, out_dim=24, mask_pool_type="grid_sample")
    assert enc.native_branch is False and "native_branch" not in enc.__dict__


def test_native_mode_names_every_limit():
    with pytest.raises(NotImplementedError, match="grid_sample"):
        _enc(pool="mean")(*_args())
    with pytest.raises(ValueError, match="hidden_dim // 4"):
        _enc(hidden=192)(*_args())
    with pytest.raises(ValueError, match="hidden_dim // 4"):
        _enc(hidden=128)(*_args())
    with pytest.raises(ValueError, match="embed_dim 96"):
        _enc(embed=96)(*_args(embed=96))
    with pytest.raises(ValueError, match="out_dim 72"):
        _enc(out=72)(*_args())
    with pytest.raises(ValueError, match="multiples of patch_size"):
        _enc()(*_args(H=60))
    with pytest.raises(ValueError, match="at most 4 levels"):
        _enc()(*_args(levels=5))
    images, masks, levels = _args()
    with pytest.raises(NotImplementedError, match="pixel gradients"):
        _enc()(images.requires_grad_(True), masks, levels)
    with pytest.raises(RuntimeError, match="bf16 CUDA"):
        _enc()(*_args())                                         # CPU parameters: no fallback
    enc = _enc().float()
    with pytest.raises(RuntimeError, match="bf16 CUDA"):
        enc(*_args())


# ---- the identities -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3])
def test_suffix_weights_and_the_mean_fold_equal_the_module_statements(L):
    """fp64: the module's statements (feat = feat + level, masked mean per level, up_dim per level, mean over levels) against the folded
    form (suffix-sum weights, one pooling, one up_dim).  Region 1 has fewer valid points than P, region 2 none: it contributes the
    module's nan_to_num zero at every level, i.e. up_dim's bias."""
    n, h, w, C, O_, P = 3, 4, 6, 8, 5, 37
    gen = torch.Generator().manual_seed(10 + L)
    coords, valid = I.make_points(L, n, P, h, w, 20 + L, short=1, empty=2)
    stem = torch.randn(n, h, w, C, generator=gen, dtype=torch.float64)
    levels = [torch.randn(n, h, w, C, generator=gen, dtype=torch.float64) for _ in range(L)]
    up_w, up_b = torch.randn(O_, C, generator=gen, dtype=torch.float64), torch.randn(O_, generator=gen, dtype=torch.float64)
    ref = I.module_pool_statements(stem, levels, coords, valid, up_w, up_b)
    wk = I.pool_weights_ref(coords, valid, h, w)
    assert wk.shape == (L, n, h * w) and torch.equal(wk[:, 2], torch.zeros(L, h * w, dtype=torch.float64))
    a = I.level_weights_ref(coords, valid, h, w)
    for k in range(L):                                           # the rule itself: level k is in every pooled map l >= k
        assert torch.allclose(wk[k], a[k:].sum(0) / L, rtol=0, atol=1e-15)
    got = I.folded_pool(stem, levels, wk, up_w, up_b)
    assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12), (got - ref).abs().max()
    assert torch.allclose(got[2], up_b, rtol=0, atol=0)


def test_im2col_restatement_feeds_the_convolutions():
    """The row / column order the tests pin the kernel against IS the convolutions': conv1 as A1 W1^T, conv2 as the reshape [M1, C1] ->
    [M1 / 4, 4 C1] times the weight permuted to (dy, dx, c), both equal torch's Conv2d in fp64."""
    torch.manual_seed(3)
    n, H, W, patch, C1, C2 = 2, 28, 42, 14, 8, 12
    k = patch // 2
    images, masks = torch.randn(n, 3, H, W).bfloat16(), (torch.rand(n, 1, H, W) > 0.5).bfloat16()
    A1 = I.im2col_ref(images, masks, patch, 256).double()
    assert torch.equal(A1[:, 4 * k * k:], torch.zeros(A1.shape[0], 256 - 4 * k * k, dtype=torch.float64))
    w1, w2 = torch.randn(C1, 4, k, k, dtype=torch.float64), torch.randn(C2, C1, 2, 2, dtype=torch.float64)
    x = torch.cat([images, masks], 1).double()
    y1 = torch.nn.functional.conv2d(x, w1, stride=k)
    y2 = torch.nn.functional.conv2d(y1, w2, stride=2)
    g1 = A1[:, :4 * k * k] @ w1.reshape(C1, -1).T
    h2, w2_ = H // patch, W // patch
    assert torch.allclose(g1.reshape(n, h2, w2_, 2, 2, C1).permute(0, 5, 1, 3, 2, 4).reshape(n, C1, 2 * h2, 2 * w2_), y1, atol=1e-10)
    g2 = g1.reshape(-1, 4 * C1) @ w2.permute(0, 2, 3, 1).reshape(C2, 4 * C1).T
    assert torch.allclose(g2.reshape(n, h2, w2_, C2).permute(0, 3, 1, 2), y2, atol=1e-9)
