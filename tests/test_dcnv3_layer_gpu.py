"""GPU: the native DCNv3 layer (vllm_dcnv3_layer_forward, include/vllm_hip.h section f3b) through the module switch and the C ABI, and
its two kernels alone, against fp64.

References: the whole layer against the same module in fp64 (the composed statements over the native fp64 operator, which
test_dcnv3_gpu.py pins to the oracle at 1e-12 -- no code shared with the new kernels); the conv + LayerNorm + GELU kernel against torch in
fp64; the fused sampling kernel against vllm_dcnv3_forward_f64 under an fp64 softmax, blended in fp64.  Every sampling test asserts from
its fp64 offsets that 40 .. 90 % of the sampling points are accepted, so the inside and the border / outside branches both run."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import dcnv3 as A

import dcnv3_layer_inputs as I
import workspace_guard as WG
from bounds import DEV, P, assert_bound, rel_rms, stream

pytestmark = pytest.mark.gpu
K = range(len(I.CASES))


def calls():
    return _lib.lib().vllm_dcnv3_layer_calls()


def native(mod, x):
    """mod(x) with the switch on, grad mode off; the switch is put back (the cached modules are shared)."""
    mod.native_layer = True
    try:
        with torch.no_grad():
            return mod(x)
    finally:
        mod.native_layer = False


@functools.lru_cache(maxsize=None)
def layer_case(k):
    """-> dict: the bf16 module and input on the GPU, the fp64 reference, the composed bf16 result and the accepted share (computed once,
    read-only for every test)."""
    C, G, H, W, N, dwk, dil, cfs, scale = I.CASES[k]
    m = I.make_module(C, G, dwk, dil, cfs, scale, seed=k)
    x = I.make_input(C, H, W, N, seed=k).to(DEV)
    mb, m64 = I.as_bf16(m, DEV), I.as_f64(m, DEV)
    with torch.no_grad():
        ref = m64(x.double())
        composed = mb(x)
    return dict(mb=mb, m64=m64, x=x, ref=ref, composed=composed, share=I.accepted_share(m64, x.double()))


@pytest.mark.parametrize("k", K, ids=I.IDS)
def test_whole_layer_through_the_module_switch(k):
    c = layer_case(k)
    assert 0.4 <= c["share"] <= 0.9, c["share"]
    mb, x = c["mb"], c["x"]
    assert mb.native_layer is False
    with torch.no_grad():
        assert mb.native_layer_applies(x)
    n0 = calls()
    out = native(mb, x)
    assert calls() == n0 + 1
    again = native(mb, x)
    assert calls() == n0 + 2
    assert out.dtype == torch.bfloat16 and out.shape == x.shape and torch.isfinite(out).all()
    assert torch.equal(out, again), "two runs of the native layer differ"
    err, err_ref = rel_rms(out, c["ref"]), rel_rms(c["composed"], c["ref"])
    print(json.dumps({"case": I.IDS[k], "native_rel_rms": err, "composed_bf16_rel_rms": err_ref, "accepted_share": c["share"]}))
    # internal tensors are fp32: at least as close to fp64 as the composed bf16 arithmetic (the fused deformable-attention layer's criterion)
    assert err <= max(1.05 * err_ref, 4e-3), (err, err_ref)


# ---- conv + LayerNorm + GELU alone ----------------------------------------------------------------------------------------------
def run_conv(x, conv, ln, dwk):
    out = torch.empty_like(x)
    N, H, W, C = x.shape
    _lib.check(_lib.lib().vllm_dwconv_ln_gelu_bf16(P(x), P(conv.weight), P(conv.bias), P(ln.weight), P(ln.bias), N, H, W, C, dwk,
                                                   float(ln.eps), P(out), stream()), "vllm_dwconv_ln_gelu_bf16")
    return out


def conv_case(C, H, W, N, dwk, seed):
    """The depth-wise conv and LayerNorm as DCNv3 builds them, parameters perturbed by 0.2 randn, in bf16 on the GPU, and an input."""
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(C, C, kernel_size=dwk, stride=1, padding=(dwk - 1) // 2, groups=C)
    ln = torch.nn.LayerNorm(C, eps=1e-6)
    with torch.no_grad():
        for p in list(conv.parameters()) + list(ln.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    return conv.to(DEV).to(torch.bfloat16), ln.to(DEV).to(torch.bfloat16), I.make_input(C, H, W, N, seed=seed).to(DEV)


CONV_EXTRA = [          # C, H, W, N, dwk: lane counts and strips the layer's cases do not reach
    (8, 4, 9, 2, 3),        # one lane per pixel; a full and a one-pixel strip
    (72, 5, 17, 1, 7),      # 9 lanes; 7 x 7 taps reach over the whole height; three strips
    (520, 3, 8, 1, 1),      # 65 lanes: the second wave holds one; 1 x 1 taps
    (2560, 2, 11, 1, 5),    # InternImage-H stage 4: five full waves, LDS reduction across them
    (4096, 1, 3, 1, 3),     # the widest accepted row: eight waves
]


@pytest.mark.parametrize("shape", [(c[0], c[2], c[3], c[4], c[5]) for c in I.CASES] + CONV_EXTRA,
                         ids=I.IDS + [f"c{c[0]}_k{c[4]}" for c in CONV_EXTRA])
def test_conv_ln_gelu_kernel_vs_fp64(shape):
    """All four borders are in every case (each map is smaller than two strips or has first / last rows and columns); dwk > H in the
    3 x 4 and the 7 x 7 cases."""
    C, H, W, N, dwk = shape
    conv, ln, x = conv_case(C, H, W, N, dwk, seed=C + dwk)
    out = run_conv(x, conv, ln, dwk)
    assert torch.equal(out, run_conv(x, conv, ln, dwk))
    ref, mag = I.conv_ln_gelu_ref(x, conv.weight, conv.bias, ln.weight, ln.bias, dwk, ln.eps)
    assert torch.isfinite(out).all()
    assert_bound(out, ref, mag, f"dwconv_ln_gelu C={C} {H}x{W} k={dwk}")
    # the module's own composed statements agree as well (bf16 between the passes: a loose cross-check of layout and tap order)
    with torch.no_grad():
        comp = torch.nn.functional.gelu(ln(conv(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)))
    assert rel_rms(out, ref) <= rel_rms(comp, ref) * 1.05 + 1e-3


@pytest.mark.parametrize("shape,at", [((64, 5, 7, 2, 5), (1, 0, 6)), ((64, 5, 7, 2, 5), (0, 4, 0)), ((320, 24, 40, 1, 5), (0, 23, 39)),
                                      ((128, 9, 6, 3, 3), (2, 4, 3)), ((64, 3, 4, 1, 5), (0, 0, 0))])
def test_conv_nan_pixel_stays_inside_its_windows(shape, at):
    """A NaN pixel (corners: where clamped border addresses point) reaches exactly the outputs whose window holds it; every other output is
    finite and has the bits of the run without the NaN."""
    C, H, W, N, dwk = shape
    conv, ln, x = conv_case(C, H, W, N, dwk, seed=C + dwk)
    clean = run_conv(x, conv, ln, dwk)
    xn = x.clone()
    n0, h0, w0 = at
    xn[n0, h0, w0, :] = float("nan")
    out = run_conv(xn, conv, ln, dwk)
    r = dwk // 2
    hh = torch.arange(H, device=DEV)[:, None]
    ww = torch.arange(W, device=DEV)[None, :]
    hit = torch.zeros(N, H, W, dtype=torch.bool, device=DEV)
    hit[n0] = ((hh - h0).abs() <= r) & ((ww - w0).abs() <= r)
    assert hit.any() and not hit.all()
    assert torch.isnan(out[hit]).all()
    assert torch.isfinite(out[~hit]).all()
    assert torch.equal(out[~hit], clean[~hit])


# ---- softmax + sampling + blend alone ---------------------------------------------------------------------------------------------
def run_sample(xp, om, ld, G, D, dil, scale, cfs):
    N, H, W, _ = xp.shape
    out = torch.empty_like(xp)
    _lib.check(_lib.lib().vllm_dcnv3_sample_fused_bf16(P(xp), P(om), ld, N, H, W, G, D, dil, scale, int(cfs), P(out), stream()),
               "vllm_dcnv3_sample_fused_bf16")
    return out


@pytest.mark.parametrize("cfs", [False, True], ids=["plain", "cfs"])
@pytest.mark.parametrize("k", K, ids=I.IDS)
def test_fused_sampling_kernel_vs_fp64_operator(k, cfs):
    C, G, H, W, N, _, dil, _, scale = I.CASES[k]
    D = C // G
    scale = float(np.float32(scale))          # the kernel's fp32 scale, exactly, for the fp64 reference as well
    om_cpu, ld, rejected = I.sampling_rows(G, H, W, N, dil, scale, cfs, seed=k)
    share = I.share_of_offsets(om_cpu[:, :18 * G].double().reshape(N, H, W, -1), dil, scale)
    assert 0.4 <= share <= 0.9, share
    xp = I.make_input(C, H, W, N, seed=50 + k).to(DEV)
    om = om_cpu.to(DEV)
    assert not torch.isfinite(om[:, (28 if cfs else 27) * G:]).any() and ld > (28 if cfs else 27) * G
    out = run_sample(xp, om, ld, G, D, dil, scale, cfs)
    assert torch.equal(out, run_sample(xp, om, ld, G, D, dil, scale, cfs))
    off = om[:, :18 * G].double().reshape(N, H, W, 18 * G).contiguous()
    msk = torch.softmax(om[:, 18 * G:27 * G].double().reshape(N, H, W, G, 9), -1).reshape(N, H, W, 9 * G).contiguous()
    core = A.dcnv3_forward(xp.double(), off, msk, 3, 3, 1, 1, dil, dil, dil, dil, G, D, scale)
    ref = core
    if cfs:
        s = torch.sigmoid(om[:, 27 * G:28 * G].double()).reshape(N, H, W, G, 1)
        ref = (core.reshape(N, H, W, G, D) * (1 - s) + xp.double().reshape(N, H, W, G, D) * s).reshape(N, H, W, C)
    assert torch.isfinite(ref).all() and torch.isfinite(out).all()
    err = (out.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2e-5 * (1 + ref.abs())     # one bf16 rounding on top of the fp32 operator's bar against the oracle
    worst = (err / bound).max().item()
    print(json.dumps({"case": I.IDS[k], "cfs": bool(cfs), "worst_error_over_bound": worst, "accepted_share": share}))
    assert worst <= 1.0, worst
    # pixels whose every point is rejected (NaN, infinite and huge offsets): exactly zero, or the centre feature alone
    rows = out.reshape(N * H * W, G, D)[rejected.to(DEV)]
    if cfs:
        want = (torch.sigmoid(om[rejected.to(DEV), 27 * G:28 * G].double())[..., None] * xp.double().reshape(-1, G, D)[rejected.to(DEV)])
        assert ((rows.double() - want).abs() <= 2.0 ** -8 * want.abs() + 1e-30).all()
    else:
        assert torch.equal(rows, torch.zeros_like(rows))


# ---- determinism, workspace, views, streams ---------------------------------------------------------------------------------------
def c_forward(mb, x, ws_ptr, ws_bytes):
    desc, keep = mb.native_descriptor()
    N, H, W, _ = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.lib().vllm_dcnv3_layer_forward(ctypes.byref(desc), P(x), N, H, W, P(out), ctypes.c_void_p(ws_ptr), ws_bytes, stream()),
               "vllm_dcnv3_layer_forward")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("k", [0, 1, 5], ids=[I.IDS[0], I.IDS[1], I.IDS[5]])
def test_workspace_content_and_guards(k):
    c = layer_case(k)
    mb, x = c["mb"], c["x"]
    N, H, W, C = x.shape
    desc, _ = mb.native_descriptor()
    need = _lib.lib().vllm_dcnv3_layer_workspace_bytes(ctypes.byref(desc), N, H, W)
    assert need > 0
    plain = native(mb, x)
    widest = max(C * 2, desc.n_proj * 4)
    for fill, skew in ((0x00, 0), (WG.HOSTILE, 16), (WG.PLAUSIBLE, 16)):
        ptr, nbytes, check = WG.guarded(need, fill, skew=skew, widest_row_bytes=widest)
        out = c_forward(mb, x, ptr, nbytes)
        check()
        assert torch.equal(out, plain), f"workspace fill {fill:#x} / skew {skew} changed the result"


def test_offset_view_and_caller_stream_give_the_same_bits():
    c = layer_case(0)
    mb, x = c["mb"], c["x"]
    plain = native(mb, x)
    buf = torch.zeros(x.numel() + 8, dtype=x.dtype, device=DEV)
    view = buf[1:1 + x.numel()].view(x.shape)          # 2 bytes into the allocation: not 16-byte aligned
    view.copy_(x)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    n0 = calls()
    assert torch.equal(native(mb, view), plain)
    assert calls() == n0 + 1
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = native(mb, x)
    side.synchronize()
    assert calls() == n0 + 2
    assert torch.equal(other, plain)
    # a non-contiguous input (a channels-first tensor viewed channels-last) is made contiguous first
    nchw = x.permute(0, 3, 1, 2).contiguous()
    assert torch.equal(native(mb, nchw.permute(0, 2, 3, 1)), plain)
    # nothing to do for an empty batch
    empty = native(mb, x[:0])
    assert empty.shape == (0,) + tuple(x.shape[1:])


# ---- routes ---------------------------------------------------------------------------------------------------------------------
ROUTES = {
    "fp32_module": dict(C=64, G=4, fp32=True),
    "grad_mode": dict(C=64, G=4, grad=True),
    "batch_norm": dict(C=64, G=4, kw=dict(norm_layer="BN")),
    "silu": dict(C=64, G=4, kw=dict(act_layer="SiLU")),
    "channels80": dict(C=80, G=10),
    "group_channels4": dict(C=64, G=16),
}


@pytest.mark.parametrize("name", list(ROUTES))
def test_other_configurations_keep_the_composed_path(name):
    r = ROUTES[name]
    m = I.make_module(r["C"], r["G"], 5, 1, True, 1.0, seed=7, **r.get("kw", {}))
    x = I.make_input(r["C"], 5, 7, 2, seed=7).to(DEV)
    if r.get("fp32"):
        mod, x = m.to(DEV), x.float()
    else:
        mod = I.as_bf16(m, DEV)
    assert mod.native_layer is False
    with torch.set_grad_enabled(bool(r.get("grad"))):
        off = mod(x)
        n0 = calls()
        mod.native_layer = True
        assert not mod.native_layer_applies(x)
        on = mod(x)
    assert calls() == n0
    assert torch.equal(on, off)
    if not r.get("grad") and not r.get("fp32") and not r.get("kw"):
        # (the native entry refuses these descriptors itself: the module's gate is not what keeps them out)
        desc, _ = mod.native_descriptor()
        assert _lib.lib().vllm_dcnv3_layer_workspace_bytes(ctypes.byref(desc), 2, 5, 7) < 0


def test_bf16_centre_parameters_are_served_too():
    """A model converted wholesale (.to(bfloat16)) holds the two centre-feature-scale parameters in bf16: same packed rows, same bits."""
    c = layer_case(0)
    mb, x = c["mb"], c["x"]
    import copy
    whole = copy.deepcopy(mb).to(torch.bfloat16)
    assert whole.center_feature_scale_proj_weight.dtype == torch.bfloat16
    n0 = calls()
    assert torch.equal(native(whole, x), native(mb, x))
    assert calls() == n0 + 2


def test_in_place_parameter_update_reaches_the_next_native_call():
    C, G, H, W, N, dwk, dil, cfs, scale = I.CASES[0]
    m = I.make_module(C, G, dwk, dil, cfs, scale, seed=0)
    x = I.make_input(C, H, W, N, seed=0).to(DEV)
    mb = I.as_bf16(m, DEV)
    before = native(mb, x)
    packed = mb.packed_projection()[1]
    assert mb.packed_projection()[1] is packed
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        new_bias = (torch.randn(mb.mask.bias.shape, generator=g) * 2).to(torch.bfloat16)
        mb.mask.bias.copy_(new_bias.to(DEV))
        m.mask.bias.copy_(new_bias.float())
    after = native(mb, x)
    assert mb.packed_projection()[1] is not packed, "the packed projection was not rebuilt"
    assert not torch.equal(after, before)
    m64 = I.as_f64(m, DEV)
    with torch.no_grad():
        ref = m64(x.double())
        composed = mb(x)
    share = I.accepted_share(m64, x.double())
    assert 0.4 <= share <= 0.9, share
    err, err_ref, err_stale = rel_rms(after, ref), rel_rms(composed, ref), rel_rms(before, ref)
    print(json.dumps({"native_rel_rms": err, "composed_bf16_rel_rms": err_ref, "stale_rel_rms": err_stale}))
    assert err <= max(1.05 * err_ref, 4e-3), (err, err_ref)
    assert err_stale > 10 * err, "the old mask bias explains the new reference as well as the new one does"
