"""GPU: the native deformable encoder layer (include/vllm_hip.h, section f2b) -- its three kernels against fp64, the whole layer
through the class switch against the module's own fp64 run, the layer chain, the slab option, views / streams / an exact guarded
workspace, and the routes that keep the composed path.

Bounds.  add_layernorm: the project's LayerNorm bound (test_vit_gpu.test_norms, test_region_stem_gpu.test_layernorm_gelu_on_short_rows),
|err| <= 1 bf16 ulp + 2^-20 (|n w| + |b|).  ReLU epilogue: the GEMM tests' ``assert_bound`` on relu(fp64 pre-activation); an output is
required to be an exact zero where the pre-activation is negative by more than that bound allows an fp32 evaluation to miss
(pre < -(1 bf16 ulp(pre) + 2^-17 sum|terms|)).  Whole layer: the fused-layer criterion of test_msda_gpu.test_fused_layer_vs_oracle,
rel_rms(native) <= max(1.05 rel_rms(composed bf16), 4e-3), both against deform_encoder_layer_inputs.reference (fp64, CPU)."""
import ctypes

import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import deformable_encoder as E
from visionllm_amd import ms_deform_attn as A

import deform_encoder_layer_inputs as I
import workspace_guard as G
from bounds import DEV, P, assert_bound, bf16_ulp, rel_rms, stream

pytestmark = pytest.mark.gpu
CLASSES = {"unipose": E.DeformableTransformerEncoderLayer, "gdino": E.GroundingDinoDeformableLayer}


def bf(t):
    return t.to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def calls():
    return _lib.lib().vllm_deform_enc_layer_calls()


@pytest.fixture
def switch(monkeypatch):
    """the class-level switch of both flavours on, for one test"""
    for cls in CLASSES.values():
        monkeypatch.setattr(cls, "native_layer", True)


@pytest.fixture
def slab_option():
    L = _lib.lib()
    old = L.vllm_set_option(b"deform_enc_ffn_slab_rows", 0)
    L.vllm_set_option(b"deform_enc_ffn_slab_rows", old)
    yield lambda v: L.vllm_set_option(b"deform_enc_ffn_slab_rows", v)
    L.vllm_set_option(b"deform_enc_ffn_slab_rows", old)


def view(rows, C, pad, lead, scale=1.0, shift=0.0):
    """a [rows, C] bf16 view with row stride C + pad that starts `lead` elements into its parent -> (parent, view)"""
    parent = bf(torch.randn(rows, C + pad, device=DEV) * scale + shift)
    v = parent[:, lead:lead + C]
    assert v.data_ptr() % 16 == 0 and v.data_ptr() != parent.data_ptr()
    return parent, v


# ---- add_layernorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 3, 257])
@pytest.mark.parametrize("C", [64, 128, 256, 320, 512])
def test_add_layernorm_against_fp64(C, rows):
    """With and without `res`, with and without `pos` / `y_pos`; every operand an offset view with a row stride of its own; outputs
    NaN-prefilled with wider rows.  An odd row count leaves the last half-wave without a row at C <= 256."""
    torch.manual_seed(C * 1000 + rows)
    L = _lib.lib()
    _, x = view(rows, C, 16, 8, 2.0, 0.3)
    _, res = view(rows, C, 24, 16)
    _, pos = view(rows, C, 8, 8, 0.5)
    w, b = bf(1 + 0.2 * torch.randn(C, device=DEV)), bf(0.2 * torch.randn(C, device=DEV))
    eps = 1e-5
    for with_res in (True, False):
        for with_pos in (True, False):
            yp, ypp = nan_bf16(rows, C + 40), nan_bf16(rows, C + 8)
            y, y_pos = yp[:, 32:32 + C], ypp[:, 8:8 + C]
            _lib.check(L.vllm_add_layernorm_bf16(P(x), C + 16, P(res) if with_res else None, C + 24, P(w), P(b), P(y), C + 40,
                                                 P(pos) if with_pos else None, C + 8, P(y_pos) if with_pos else None, C + 8, rows, C, eps,
                                                 stream()), "add_layernorm")
            torch.cuda.synchronize()
            xs = x.double() + (res.double() if with_res else 0)
            mean = xs.mean(-1, keepdim=True)
            n = (xs - mean) / torch.sqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + eps)
            ref = n * w.double() + b.double()
            err = (y.double() - ref).abs()
            u = ((err - 2.0 ** -20 * ((n * w.double()).abs() + b.double().abs())).clamp_min(0) / bf16_ulp(ref)).max().item()
            print(f"add_layernorm C{C} rows{rows} res{int(with_res)} pos{int(with_pos)}: max excess {u:.3f} bf16 ulp")
            assert u <= 1.0
            # nothing beyond the C columns of a row
            assert torch.isnan(yp[:, :32]).all() and torch.isnan(yp[:, 32 + C:]).all()
            assert torch.isnan(ypp[:, :8]).all() and (torch.isnan(ypp[:, 8:]).all() if not with_pos else True)
            if with_pos:
                yc, pc, want = y.contiguous(), pos.contiguous(), nan_bf16(rows, C)
                _lib.check(L.vllm_add_bf16(P(yc), P(pc), P(want), rows * C, stream()), "add_bf16")
                torch.cuda.synchronize()
                assert torch.equal(bits(y_pos), bits(want))
                assert torch.equal(bits(want), bits(yc + pc))


def test_add_layernorm_in_place_has_the_bits_of_out_of_place():
    torch.manual_seed(5)
    rows, C = 131, 256
    L = _lib.lib()
    x = bf(torch.randn(rows, C, device=DEV))
    w, b = bf(1 + 0.2 * torch.randn(C, device=DEV)), bf(0.2 * torch.randn(C, device=DEV))
    y, z = nan_bf16(rows, C), x.clone()
    for dst in (y, z):
        src = x if dst is y else z
        _lib.check(L.vllm_add_layernorm_bf16(P(src), C, None, 0, P(w), P(b), P(dst), C, None, 0, None, 0, rows, C, 1e-5, stream()), "add_layernorm")
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(z)) and not torch.isnan(y).any()


# ---- add ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "off_by_one_element"])
@pytest.mark.parametrize("n", [1, 7, 8, 4099])
def test_add_bf16_is_torch_bf16_add(n, lead):
    torch.manual_seed(n)
    a, b = bf(torch.randn(n + 16, device=DEV) * 3)[lead:lead + n], bf(torch.randn(n + 16, device=DEV))[lead:lead + n]
    parent = nan_bf16(n + 16)
    out = parent[lead:lead + n]
    _lib.check(_lib.lib().vllm_add_bf16(P(a), P(b), P(out), n, stream()), "add_bf16")
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(a + b))
    assert torch.isnan(parent[:lead]).all() and torch.isnan(parent[lead + n:]).all()


# ---- ReLU epilogue ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", [0x100, 0x200], ids=["128x128", "8phase"])
@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("N", [128, 1024])
@pytest.mark.parametrize("M", [77, 1100])
def test_relu_epilogue_against_fp64(M, N, K, force):
    torch.manual_seed(M + N + K)
    X, W, b = bf(torch.randn(M, K, device=DEV)), bf(torch.randn(N, K, device=DEV) / K ** 0.5), bf(0.3 * torch.randn(N, device=DEV))
    nan_row = 5
    X[nan_row] = float("nan")
    Y = nan_bf16(M, N)
    _lib.check(_lib.lib().vllm_gemm_bf16_relu(P(X), P(W), P(b), P(Y), M, N, K, K, K, N, force, stream()), "gemm_bf16_relu")
    torch.cuda.synchronize()
    assert torch.isnan(Y[nan_row]).all()          # relu(NaN) is NaN, as torch.relu
    keep = torch.ones(M, dtype=torch.bool, device=DEV)
    keep[nan_row] = False
    Xd, Wd, bd = X[keep].double(), W.double(), b.double()
    pre = Xd @ Wd.T + bd
    mag = Xd.abs() @ Wd.abs().T + bd.abs()
    out = Y[keep]
    assert not torch.isnan(out).any()
    assert_bound(out, pre.clamp_min(0), mag, f"relu epilogue M{M} N{N} K{K} force{force:#x}")
    clearly_negative = pre < -(bf16_ulp(pre) + 2.0 ** -17 * mag)
    frac = clearly_negative.double().mean().item()
    assert 0.3 <= frac <= 0.7, frac               # both branches
    assert (out[clearly_negative] == 0).all()
    assert (out >= 0).all()


# ---- the whole layer ----------------------------------------------------------------------------------------------------------------------------
def judged(native, composed, truth, what):
    e, ec = rel_rms(native.cpu(), truth), rel_rms(composed.cpu(), truth)
    print(f"{what}: rel rms native {e:.3e}, composed bf16 {ec:.3e}")
    assert torch.isfinite(native.float()).all()
    assert e <= max(1.05 * ec, 4e-3), (what, e, ec)


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("case", I.CASES, ids=I.IDS)
def test_layer_through_the_switch_against_its_own_fp64_run(flavour, case, monkeypatch):
    shape, with_pos, with_mask = case
    m = I.as_bf16(I.make_layer(flavour, shape), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    with torch.no_grad():
        before = calls()
        composed = I.call(flavour, m, t)
        assert calls() == before and m.native_layer is False
        monkeypatch.setattr(CLASSES[flavour], "native_layer", True)
        assert m.native_layer_applies(t["src"], t["pos"], t["reference_points"])
        native = I.call(flavour, m, t)
        assert calls() == before + 1
        again = I.call(flavour, m, t)
        assert calls() == before + 2
        if flavour == "gdino":
            res = m(t["src"], None if t["padding_mask"] is None else ~t["padding_mask"], t["pos"], t["reference_points"], t["spatial_shapes"],
                    t["level_start_index"])
            assert isinstance(res, tuple) and len(res) == 2 and res[1] is None and torch.equal(res[0], native)
    assert native.dtype == torch.bfloat16 and native.shape == t["src"].shape
    assert torch.equal(bits(native), bits(again))
    judged(native, composed, I.reference(flavour, *case)[0], f"{flavour} {case}")


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("with_pos", [True, False])
def test_chained_layers_have_the_bits_of_layers_that_each_add_pos(flavour, with_pos, switch):
    a = I.as_bf16(I.make_layer(flavour, "tile"), DEV)
    b = I.as_bf16(I.make_layer(flavour, "tile", activation="gelu"), DEV)
    with torch.no_grad():
        b.self_attn.value_proj.weight.mul_(0.5)
    t = I.to(I.make_inputs("tile", with_pos, True), DEV)
    with torch.no_grad():
        x = I.call(flavour, a, t)
        x = I.call(flavour, b, dict(t, src=x))
        before = calls()
        got = E.encoder_layers_forward([a, b], t["src"], t["pos"], t["reference_points"], t["spatial_shapes"], t["level_start_index"],
                                       t["padding_mask"])
        assert calls() == before + 2
    assert torch.equal(bits(got), bits(x))


@pytest.mark.parametrize("slab", [0, 64, 100])
def test_slab_heights_meet_the_same_criterion(slab, monkeypatch, slab_option):
    """322 rows: one slab, five full slabs and a short one, three slabs and a short one.  Bit identity across heights is not required."""
    case = ("tile", True, True)
    m = I.as_bf16(I.make_layer("unipose", "tile"), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    slab_option(slab)
    with torch.no_grad():
        composed = I.call("unipose", m, t)
        monkeypatch.setattr(CLASSES["unipose"], "native_layer", True)
        before = calls()
        native = I.call("unipose", m, t)
        assert calls() == before + 1
    judged(native, composed, I.reference("unipose", *case)[0], f"slab {slab}")


def test_offset_views_and_a_caller_stream(switch):
    case = ("small", True, True)
    m = I.as_bf16(I.make_layer("unipose", "small"), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    with torch.no_grad():
        want = I.call("unipose", m, t)
        tv = dict(t)
        for k in ("src", "pos"):          # 2 bytes into their parents: not 16-byte aligned
            parent = torch.zeros(t[k].numel() + 8, dtype=torch.bfloat16, device=DEV)
            parent[1:1 + t[k].numel()] = t[k].reshape(-1)
            tv[k] = parent[1:1 + t[k].numel()].view_as(t[k])
            assert tv[k].data_ptr() % 16 != 0
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        before = calls()
        with torch.cuda.stream(s):
            got = I.call("unipose", m, tv)
        s.synchronize()
        assert calls() == before + 1
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("fill", [G.HOSTILE, G.PLAUSIBLE], ids=["hostile", "plausible"])
@pytest.mark.parametrize("slab", [0, 64])
def test_exact_workspace_with_guards(fill, slab, switch, slab_option):
    """The C entry with exactly the queried bytes, 16-byte aligned and no better, whatever they held: the module's bits, guards intact."""
    case = ("tile", True, True)
    m = I.as_bf16(I.make_layer("unipose", "tile"), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    slab_option(slab)
    with torch.no_grad():
        want = I.call("unipose", m, t)
    L = _lib.lib()
    B, S, C = t["src"].shape
    d = _lib.VllmDeformEncLayerDesc()
    a = d.attn
    a.d_model, a.n_heads, a.n_levels, a.n_points, a.ref_dim = C, m.self_attn.n_heads, m.self_attn.n_levels, m.self_attn.n_points, 2
    a.geometry = A.known_geometry(t["spatial_shapes"], S)          # what the module's call passed
    d.d_ffn, d.act, d.norm1_eps, d.norm2_eps = m.linear1.out_features, 0, m.norm1.eps, m.norm2.eps
    for name in ("value_proj", "sampling_offsets", "attention_weights", "output_proj"):
        setattr(a, name + "_w", getattr(m.self_attn, name).weight.data_ptr())
        setattr(a, name + "_b", getattr(m.self_attn, name).bias.data_ptr())
    for name, mod in (("norm1", m.norm1), ("fc1", m.linear1), ("fc2", m.linear2), ("norm2", m.norm2)):
        setattr(d, name + "_w", mod.weight.data_ptr())
        setattr(d, name + "_b", mod.bias.data_ptr())
    need = L.vllm_deform_enc_layer_workspace_bytes(ctypes.byref(d), B, S)
    assert need > 0
    ws, nbytes, check = G.guarded(need, fill, skew=16, widest_row_bytes=d.d_ffn * 2)
    out, qout = nan_bf16(B, S, C), nan_bf16(B, S, C)
    mask = t["padding_mask"].to(torch.uint8)
    _lib.check(L.vllm_deform_enc_layer_forward(ctypes.byref(d), P(t["src"]), P(t["pos"]), None, P(t["reference_points"]), P(mask),
                                               P(t["spatial_shapes"]), P(t["level_start_index"]), B, S, P(out), P(qout),
                                               ctypes.c_void_p(ws), nbytes, stream()), "vllm_deform_enc_layer_forward")
    check()
    assert torch.equal(bits(out), bits(want))
    assert torch.equal(bits(qout), bits(want + t["pos"]))


@pytest.mark.parametrize("flavour", I.FLAVOURS)
def test_routes_that_keep_the_composed_path(flavour, switch):
    t = I.to(I.make_inputs("small"), DEV)

    def composed_only(m, tt, grad=False, **kw):
        before = calls()
        with torch.enable_grad() if grad else torch.no_grad():
            if flavour == "gdino":
                out = m(tt["src"], ~tt["padding_mask"], tt["pos"], tt["reference_points"], tt["spatial_shapes"], tt["level_start_index"], **kw)
                out = out if kw else out[0]
            else:
                assert not kw
                out = I.call(flavour, m, tt)
        assert calls() == before
        return out

    m = I.as_bf16(I.make_layer(flavour, "small"), DEV)
    with torch.no_grad():
        before = calls()
        I.call(flavour, m, t)
        assert calls() == before + 1                        # the baseline: this module and these inputs do take the native call
    if flavour == "gdino":
        out, attn = composed_only(m, t, output_attentions=True)
        assert attn is not None and attn.shape[:2] == t["src"].shape[:2]
    assert composed_only(m, t, grad=True).requires_grad      # grad enabled, trainable parameters
    m.train()
    composed_only(m, t)                                      # train() with dropout 0.1
    m.eval()
    f32 = I.make_layer(flavour, "small").to(DEV)
    assert composed_only(f32, I.to(I.make_inputs("small"), DEV, torch.float32)).dtype == torch.float32
    t4 = dict(t, reference_points=torch.cat([t["reference_points"], torch.full_like(t["reference_points"], 0.2)], -1))
    assert not m.native_layer_applies(t4["src"], t4["pos"], t4["reference_points"])
    with torch.no_grad():
        assert m.native_layer_reasons(t4["src"], t4["pos"], t4["reference_points"]) == ["reference_points: last dim 2"]
        assert m.native_layer_reasons(t["src"], t["pos"], t["reference_points"]) == []
    composed_only(m, t4)                                     # reference_points with last dim 4
    if flavour == "unipose":
        pre = I.as_bf16(I.make_layer(flavour, "small", activation="prelu"), DEV)
        composed_only(pre, t)
    else:
        silu = I.as_bf16(I.make_layer(flavour, "small", activation="silu"), DEV)
        composed_only(silu, t)
