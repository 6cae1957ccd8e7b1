"""CPU: the boundary of the native DCNv3 layer (include/vllm_hip.h, section f3b) -- symbols, descriptor layout, the size query, the
argument gates (refused calls only, fake pointers: nothing is dereferenced, no device is touched) and the packing helper."""
import ctypes
import re
import subprocess

import pytest
import torch

from visionllm_amd import _lib

import dcnv3_layer_inputs as I

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
NEW = ("vllm_dcnv3_layer_desc_sizeof", "vllm_dcnv3_layer_workspace_bytes", "vllm_dcnv3_layer_forward", "vllm_dcnv3_layer_calls",
       "vllm_dwconv_ln_gelu_bf16", "vllm_dcnv3_sample_fused_bf16")
POINTERS = ("input_proj_w", "input_proj_b", "dw_w", "dw_b", "ln_w", "ln_b", "proj_w", "proj_b", "output_proj_w", "output_proj_b")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def desc(C=64, G=4, dwk=5, dil=1, cfs=1, n_proj=None, kernel=3, **ptrs):
    d = _lib.VllmDcnv3LayerDesc()
    d.channels, d.group, d.kernel_size, d.dw_kernel_size, d.dilation, d.center_feature_scale = C, G, kernel, dwk, dil, cfs
    d.n_proj = n_proj if n_proj is not None else ((28 if cfs else 27) * G + 7) // 8 * 8
    d.offset_scale, d.ln_eps = 1.0, 1e-6
    for n in POINTERS:
        setattr(d, n, ptrs.get(n, PTR))
    return d


def last_error():
    return _lib.lib().vllm_last_error().decode()


def test_symbols_are_declared_and_exported_and_the_abi_version_stays_2():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T vllm_" in line}
    for n in NEW:
        assert n in protos, n
        assert n in exported, n
    assert _lib.header_abi_version() == 2 and _lib.lib().vllm_abi_version() == 2
    assert "f3b. The whole DCNv3 layer, bf16 modules" in open(_lib.HEADER).read()


def test_descriptor_mirror_has_the_library_size_and_the_header_order():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.VllmDcnv3LayerDesc) == L.vllm_dcnv3_layer_desc_sizeof()
    _lib.check_struct_layouts()
    hdr = open(_lib.HEADER).read()
    body = hdr[hdr.index("typedef struct VllmDcnv3LayerDesc {"):hdr.index("} VllmDcnv3LayerDesc;")]
    order = [re.search(r"\b" + n + r"\b", body).start() for n, _ in _lib.VllmDcnv3LayerDesc._fields_]
    assert order == sorted(order), "field order differs from include/vllm_hip.h"
    assert L.vllm_dcnv3_layer_calls() >= 0


@pytest.mark.parametrize("case", I.CASES, ids=I.IDS)
def test_workspace_query_is_positive_and_monotone(case):
    C, G, H, W, N, dwk, dil, cfs, _ = case
    L = _lib.lib()
    d = desc(C, G, dwk, dil, int(cfs))
    q = lambda n, h, w: L.vllm_dcnv3_layer_workspace_bytes(ctypes.byref(d), n, h, w)
    base = q(N, H, W)
    assert base > 0
    # x_proj, x1 (reused for the blended core) bf16 and the fp32 projection rows, each piece rounded up to 256 bytes
    R = N * H * W
    a256 = lambda x: (x + 255) & ~255
    assert base == 2 * a256(R * C * 2) + a256(R * d.n_proj * 4)
    assert q(N + 1, H, W) >= base and q(N, H + 1, W) >= base and q(N, H, W + 1) >= base
    assert q(N + 3, H + 5, W + 2) > base
    assert q(0, H, W) == 0 and q(-1, H, W) < 0
    assert q(1 << 11, 1 << 10, 1 << 10) < 0          # N H W = 2^31


@pytest.mark.parametrize("kw,word", [
    (dict(C=80, G=10), "multiple of 64"),
    (dict(C=64, G=16), "group channels"),
    (dict(kernel=5), "kernel_size"),
    (dict(dwk=4), "dw_kernel_size"),
    (dict(dwk=9), "dw_kernel_size"),
    (dict(cfs=0, n_proj=108), "n_proj"),              # the used rows, but no multiple of 8
    (dict(cfs=1, n_proj=104), "n_proj"),              # a multiple of 8 below the used rows (112)
    (dict(dil=0), "dilation"),
    (dict(cfs=2), "center_feature_scale"),
], ids=["channels80", "group_channels4", "kernel5", "dwk_even", "dwk9", "n_proj108", "n_proj_short", "dilation0", "flag2"])
def test_refused_descriptors(kw, word):
    L = _lib.lib()
    d = desc(**kw)
    assert L.vllm_dcnv3_layer_workspace_bytes(ctypes.byref(d), 2, 5, 7) < 0
    assert word in last_error(), last_error()
    assert L.vllm_dcnv3_layer_forward(ctypes.byref(d), vp(PTR), 2, 5, 7, vp(PTR), vp(PTR), 1 << 30, None) == EINVAL
    assert word in last_error(), last_error()
    assert L.vllm_dcnv3_layer_workspace_bytes(None, 2, 5, 7) < 0


def test_short_misaligned_and_null_workspaces_are_refused():
    L = _lib.lib()
    d = desc()
    need = L.vllm_dcnv3_layer_workspace_bytes(ctypes.byref(d), 2, 5, 7)
    assert need > 0
    call = lambda w, n: L.vllm_dcnv3_layer_forward(ctypes.byref(d), vp(PTR), 2, 5, 7, vp(PTR), vp(w), n, None)
    calls = L.vllm_dcnv3_layer_calls()
    for w, n in ((PTR, need - 1), (PTR + 8, need), (PTR + 8, need + 4096), (0, need)):
        assert call(w, n) == EINVAL
        assert "workspace" in last_error(), last_error()
    assert L.vllm_dcnv3_layer_calls() == calls          # no refused call reached a launch


def test_null_and_misaligned_operands_have_their_own_messages():
    L = _lib.lib()
    d = desc()
    need = L.vllm_dcnv3_layer_workspace_bytes(ctypes.byref(d), 2, 5, 7)
    fwd = lambda dd, x, o: L.vllm_dcnv3_layer_forward(ctypes.byref(dd), vp(x), 2, 5, 7, vp(o), vp(PTR), need, None)
    assert fwd(d, 0, PTR) == EINVAL
    assert "null pointer (input / out)" in last_error() and "workspace" not in last_error()
    assert fwd(d, PTR, PTR + 8) == EINVAL
    assert "misaligned input / out" in last_error()
    for name in POINTERS:
        assert fwd(desc(**{name: PTR + 8}), PTR, PTR) == EINVAL, name
        assert "misaligned weight or bias" in last_error() and "workspace" not in last_error(), (name, last_error())
        assert fwd(desc(**{name: 0}), PTR, PTR) == EINVAL, name
        assert "missing weights" in last_error(), (name, last_error())
    assert L.vllm_dcnv3_layer_forward(ctypes.byref(d), vp(PTR), 1 << 11, 1 << 10, 1 << 10, vp(PTR), vp(PTR), 1 << 40, None) == EINVAL
    assert "2^31" in last_error()
    # N H W == 0: nothing to do, whatever the pointers are
    calls = L.vllm_dcnv3_layer_calls()
    assert L.vllm_dcnv3_layer_forward(ctypes.byref(d), None, 0, 5, 7, None, None, 0, None) == 0
    assert L.vllm_dcnv3_layer_calls() == calls


def test_kernel_entries_refuse_what_they_cannot_run():
    L = _lib.lib()
    p = vp(PTR)
    conv = lambda C=64, dwk=5, x=p, N=2: L.vllm_dwconv_ln_gelu_bf16(x, p, p, p, p, N, 5, 7, C, dwk, 1e-6, p, None)
    assert conv(C=60) == EINVAL and "multiple of 8" in last_error()
    assert conv(C=4104) == EINVAL and "at most 4096" in last_error()
    assert conv(dwk=2) == EINVAL and "dwk" in last_error()
    assert conv(x=None) == EINVAL and "null pointer" in last_error()
    assert conv(x=vp(PTR + 2)) == EINVAL and "misaligned" in last_error()
    assert conv(N=0, x=None) == 0
    samp = lambda G=4, D=16, ld=112, cfs=1, om=p, N=2: L.vllm_dcnv3_sample_fused_bf16(p, om, ld, N, 5, 7, G, D, 1, 1.0, cfs, p, None)
    assert samp(D=4) == EINVAL and "D must be" in last_error()
    assert samp(ld=108) == EINVAL and "ld_om" in last_error()          # 28 G = 112 columns are read with the flag
    assert samp(ld=110, cfs=0) == EINVAL and "ld_om" in last_error()   # enough columns (108), but rows must stay 16-byte aligned
    assert samp(om=None) == EINVAL and "null pointer" in last_error()
    assert samp(om=vp(PTR + 4)) == EINVAL and "misaligned" in last_error()
    assert samp(N=0, om=None) == 0


@pytest.mark.parametrize("cfs,G", [(True, 4), (False, 4), (True, 10), (False, 10)])
def test_packed_projection_rows_padding_and_cache(cfs, G):
    m = I.make_module(G * 16, G, 3, 1, cfs, 1.0, seed=3)
    assert m.native_layer is False
    w, b = m.packed_projection()
    used = (28 if cfs else 27) * G
    assert w.shape == ((used + 7) // 8 * 8, G * 16) and b.shape == (w.shape[0],)
    assert torch.equal(w[:18 * G], m.offset.weight) and torch.equal(b[:18 * G], m.offset.bias)
    assert torch.equal(w[18 * G:27 * G], m.mask.weight) and torch.equal(b[18 * G:27 * G], m.mask.bias)
    if cfs:
        assert torch.equal(w[27 * G:28 * G], m.center_feature_scale_proj_weight)
        assert torch.equal(b[27 * G:28 * G], m.center_feature_scale_proj_bias)
    assert not w[used:].any() and not b[used:].any()
    rw, rb, rused = I.pack_reference(m)
    assert rused == used and torch.equal(w, rw) and torch.equal(b, rb)
    # cached until a source changes: in place (version), or replaced (pointer)
    w2, b2 = m.packed_projection()
    assert w2 is w and b2 is b
    with torch.no_grad():
        m.mask.bias.add_(1.0)
    w3, b3 = m.packed_projection()
    assert w3 is not w and torch.equal(b3[18 * G:27 * G], m.mask.bias) and torch.equal(w3, w)
    assert m.packed_projection()[0] is w3
    m.offset.weight.data = m.offset.weight.data.clone() * 2
    assert torch.equal(m.packed_projection()[0][:18 * G], m.offset.weight)
    # a bf16 module packs bf16, the fp32 centre parameters rounded as the composed path rounds them (.to(x1.dtype))
    mb = I.as_bf16(m, "cpu")
    wb, bb = mb.packed_projection()
    assert wb.dtype == torch.bfloat16 and bb.dtype == torch.bfloat16
    if cfs:
        assert mb.center_feature_scale_proj_weight.dtype == torch.float32
        assert torch.equal(wb[27 * G:28 * G], mb.center_feature_scale_proj_weight.to(torch.bfloat16))


def test_the_switch_changes_nothing_on_the_cpu():
    """Off by default; on, a CPU tensor still takes the composed path (which raises 'Not implement on cpu' in the operator, as before)."""
    m = I.make_module(64, 4, 5, 1, True, 1.0)
    x = I.make_input(64, 5, 7, 2).float()
    assert m.native_layer is False
    m.native_layer = True
    with torch.no_grad():
        assert not m.native_layer_applies(x)
        with pytest.raises(RuntimeError, match="Not implement on cpu"):
            m(x)
    assert "native_layer" not in m.state_dict() and not any("native" in k for k in m.state_dict())
