"""GPU: the native deformable decoder layer (include/vllm_hip.h, section f2c) -- the masked attention kernel alone against fp64, the
whole layer of both flavours through the class switch against the module's own fp64 run, an exact guarded workspace, sequence-first
inputs, a caller stream, and the routes that keep the composed path.

Bounds.  Attention kernel: the bound of test_vit_gpu.test_attention_vs_oracle, |err| <= 1 bf16 ulp(ref) + 2^-8 sum_j p_j |v_j| (P is
rounded to bf16 before P V, fp32 accumulation, one rounding of the result); a row whose every key is masked must be NaN in all D outputs
of every head and no other element may be.  Whole layer: the fused-layer criterion of test_msda_gpu.test_fused_layer_vs_oracle,
rel_rms(native) <= max(1.05 rel_rms(composed bf16), 4e-3), both against deform_decoder_layer_inputs.reference (fp64, CPU)."""
import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import deformable_decoder as D

import deform_decoder_layer_inputs as I
import workspace_guard as G
from bounds import DEV, P, bf16_ulp, rel_rms, stream

pytestmark = pytest.mark.gpu
CLASSES = {"unipose": D.DeformableTransformerDecoderLayer, "gdino": D.GroundingDinoDecoderLayer}


def bits(t):
    return t.contiguous().view(torch.int16)


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def calls():
    return _lib.lib().vllm_deform_dec_layer_calls()


@pytest.fixture
def switch(monkeypatch):
    """the class-level switch of both flavours on, for one test"""
    for cls in CLASSES.values():
        monkeypatch.setattr(cls, "native_layer", True)


# ---- the attention kernel alone -----------------------------------------------------------------------------------------------------------------
def packed_operands(Dh, Lq, Lk, H, B):
    """q, k, v as offset views of packed parents with three different row strides -> (q, k, v), each [B, L, H D] with stride(2) == 1"""
    C = H * Dh
    q, k, v = (x.to(DEV) for x in I.mha_inputs(Dh, Lq, Lk, H, B))
    qp = torch.randn(B, Lq, 2 * C + 8, device=DEV).to(torch.bfloat16)
    kvp = torch.randn(B, Lk, 2 * C + 24, device=DEV).to(torch.bfloat16)
    vp = torch.randn(B, Lk, C + 16, device=DEV).to(torch.bfloat16)
    qv, kv, vv = qp[:, :, C:2 * C], kvp[:, :, 8:8 + C], vp[:, :, 16:16 + C]
    qv.copy_(q), kv.copy_(k), vv.copy_(v)
    for t in (qv, kv, vv):
        assert t.data_ptr() % 16 == 0 and t.stride(2) == 1
    assert len({qv.stride(1), kv.stride(1), vv.stride(1)}) == 3
    return qv, kv, vv


def run_mha(q, k, v, am, kp, H, Dh):
    """-> (the [B, Lq, H D] output view, its NaN-prefilled parent with wider rows)"""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    parent = nan_bf16(B, Lq, C + 40)
    out = parent[:, :, 32:32 + C]
    am8 = None if am is None else am.to(DEV).to(torch.uint8).contiguous()
    kp8 = None if kp is None else kp.to(DEV).to(torch.uint8).contiguous()
    _lib.check(_lib.lib().vllm_mha_fwd_bf16(P(q), q.stride(0), q.stride(1), P(k), k.stride(0), k.stride(1), P(v), v.stride(0), v.stride(1),
                                            P(out), out.stride(0), out.stride(1), P(am8), P(kp8), B, Lq, Lk, H, Dh, Dh ** -0.5, stream()),
               "vllm_mha_fwd_bf16")
    torch.cuda.synchronize()
    return out, parent


def judge_mha(out, parent, Dh, Lq, Lk, H, B, pattern, kpm, what):
    C = H * Dh
    ref, mag, share = I.mha_reference(Dh, Lq, Lk, H, B, pattern, kpm)
    assert torch.isnan(parent[:, :, :32]).all() and torch.isnan(parent[:, :, 32 + C:]).all(), f"{what}: wrote outside the H D columns"
    got = out.cpu().double().reshape(B, Lq, H, Dh)
    dead = torch.isnan(ref)
    dead_rows = dead.all(-1).all(-1)                       # [B, Lq]: the masks do not depend on the head
    assert torch.equal(dead, dead_rows[:, :, None, None].expand_as(dead))
    assert torch.equal(torch.isnan(got), dead), f"{what}: NaN exactly where every key of the row is masked"
    live = ~dead
    err = (got - ref).abs()[live]
    u = ((err - 2.0 ** -8 * mag[live]).clamp_min(0) / bf16_ulp(ref[live])).max().item() if live.any() else 0.0
    print(f"{what}: masked pairs {share:.3f}, rows with every key masked {int(dead_rows.sum())}, max excess {u:.3f} bf16 ulp")
    assert u <= 1.0, what
    return dead_rows


@pytest.mark.parametrize("B", I.MHA_B)
@pytest.mark.parametrize("H", I.MHA_H)
@pytest.mark.parametrize("L", I.MHA_L, ids=[f"{a}x{b}" for a, b in I.MHA_L])
@pytest.mark.parametrize("Dh", I.MHA_D)
def test_mha_kernel_against_fp64(Dh, L, H, B):
    """Without a mask, with each attention-mask pattern the shape can carry, each with and without the key-padding mask; two runs of every
    case bit-identical."""
    Lq, Lk = L
    torch.manual_seed(Dh + Lq + Lk + H + B)
    q, k, v = packed_operands(Dh, Lq, Lk, H, B)
    for pattern in [None] + I.mha_patterns(Lq, Lk):
        for kpm in (False, True):
            am, kp, dead_row = I.mha_masks(pattern, kpm, Lq, Lk, B)
            what = f"mha D{Dh} {Lq}x{Lk} H{H} B{B} {pattern} kpm{int(kpm)}"
            out, parent = run_mha(q, k, v, am, kp, H, Dh)
            dead_rows = judge_mha(out, parent, Dh, Lq, Lk, H, B, pattern, kpm, what)
            again, _ = run_mha(q, k, v, am, kp, H, Dh)
            assert torch.equal(bits(out), bits(again)), f"{what}: two runs differ"
            if dead_row is not None:
                assert dead_rows[:, dead_row].all()
            if pattern == "first_tile" and not kpm:
                # rows hidden from the whole first key tile have later keys: finite (the running maximum starts at -inf)
                assert not dead_rows.any() and torch.isfinite(out[:, :(Lq + 1) // 2].float()).all()


def test_mha_kernel_on_a_caller_stream():
    Dh, Lq, Lk, H, B = 32, 130, 130, 3, 2
    q, k, v = packed_operands(Dh, Lq, Lk, H, B)
    am, kp, _ = I.mha_masks("denoise", True, Lq, Lk, B)
    want, _ = run_mha(q, k, v, am, kp, H, Dh)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, parent = run_mha(q, k, v, am, kp, H, Dh)
    s.synchronize()
    assert torch.equal(bits(got), bits(want))
    judge_mha(got, parent, Dh, Lq, Lk, H, B, "denoise", True, "mha on a side stream")


# ---- the whole layer ----------------------------------------------------------------------------------------------------------------------------
def judged(native, composed, truth, what):
    e, ec = rel_rms(native.cpu(), truth), rel_rms(composed.cpu(), truth)
    print(f"{what}: rel rms native {e:.3e}, composed bf16 {ec:.3e}")
    assert torch.isfinite(native.float()).all()
    assert e <= max(1.05 * ec, 4e-3), (what, e, ec)


def through_the_switch(flavour, m, t, truth, what, monkeypatch):
    with torch.no_grad():
        before = calls()
        composed = I.call(flavour, m, t)
        assert calls() == before and m.native_layer is False
        monkeypatch.setattr(CLASSES[flavour], "native_layer", True)
        assert I.applies(flavour, m, t) == []
        native = I.call(flavour, m, t)
        assert calls() == before + 1
        again = I.call(flavour, m, t)
        assert calls() == before + 2
    assert native.dtype == torch.bfloat16 and native.shape == t["tgt"].shape
    assert torch.equal(bits(native), bits(again))
    judged(native, composed, truth, what)
    return native


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("case", I.CASES, ids=I.IDS)
def test_layer_through_the_switch_against_its_own_fp64_run(flavour, case, monkeypatch):
    shape = case[0]
    m = I.as_bf16(I.make_layer(flavour, shape), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    native = through_the_switch(flavour, m, t, I.reference(flavour, *case), f"{flavour} {case}", monkeypatch)
    if flavour == "gdino":
        with torch.no_grad():
            res = m(t["tgt"], t["pos"], t["reference_points"], t["spatial_shapes"], t["level_start_index"], t["memory"],
                    None if t["padding_mask"] is None else ~t["padding_mask"], t["memory_text"], t["text_mask"], t["self_attn_mask"])
        assert isinstance(res, tuple) and len(res) == 1 and torch.equal(res[0], native)


@pytest.mark.parametrize("variant", list(I.VARIANTS))
@pytest.mark.parametrize("ref_dim", [2, 4])
@pytest.mark.parametrize("shape", list(I.SHAPES))
def test_unipose_variants_through_the_switch(shape, ref_dim, variant, monkeypatch):
    """use_4D_normalizer, without the text attention, after rm_self_attn_modules(), and with neither attention block"""
    m = I.as_bf16(I.make_layer("unipose", shape, **I.VARIANTS[variant]), DEV)
    if "rm_sa" in I.VARIANTS[variant]:
        assert m.self_attn is None and m.norm2 is None
    t = I.to(I.make_inputs(shape, ref_dim, True, True), DEV)
    through_the_switch("unipose", m, t, I.reference("unipose", shape, ref_dim, True, True, variant), f"unipose {shape} ref{ref_dim} {variant}",
                       monkeypatch)


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("fill", [G.HOSTILE, G.PLAUSIBLE], ids=["hostile", "plausible"])
def test_exact_workspace_with_guards(flavour, fill, switch, monkeypatch):
    """The C entry with exactly the queried bytes, 16-byte aligned and no better, whatever they held: the bits of a clean run, guards intact."""
    case = ("tile", 4, True, True)
    m = I.as_bf16(I.make_layer(flavour, "tile"), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    with torch.no_grad():
        want = I.call(flavour, m, t)
    checks = []

    def exact(device, nbytes, what, slot=0):
        _lib.check(0 if nbytes >= 0 else -1, what)
        assert nbytes > 0
        _, n, check = G.guarded(nbytes, fill, skew=16, widest_row_bytes=I.SHAPES["tile"]["F"] * 2)
        checks.append(check)
        return check.workspace, n
    monkeypatch.setattr(_lib, "sized_workspace", exact)
    with torch.no_grad():
        before = calls()
        got = I.call(flavour, m, t)
        assert calls() == before + 1
    assert len(checks) == 1 and checks[0].workspace.data_ptr() % 32 == 16
    checks[0]()
    assert torch.equal(bits(got), bits(want))


def test_sequence_first_layouts_and_a_caller_stream(switch):
    """UniPose: transposed views of batch-first tensors (what ``call`` passes), contiguous sequence-first tensors, and views that are not
    16-byte aligned, on a side stream: the same bits."""
    case = ("small", 4, True, True)
    m = I.as_bf16(I.make_layer("unipose", "small"), DEV)
    t = I.to(I.make_inputs(*case), DEV)
    assert not t["tgt"].transpose(0, 1).is_contiguous()
    tr = lambda x: x.transpose(0, 1)
    args = lambda tgt, pos, ref, mem: (tgt, pos, None, None, ref, t["memory_text"], t["text_mask"], mem, t["padding_mask"], t["level_start_index"],
                                       t["spatial_shapes"], None, t["self_attn_mask"], None)
    with torch.no_grad():
        before = calls()
        want = I.call("unipose", m, t)
        sf = m(*args(tr(t["tgt"]).contiguous(), tr(t["pos"]).contiguous(), tr(t["reference_points"]).contiguous(), tr(t["memory"]).contiguous()))
        assert sf.shape == (t["tgt"].shape[1], t["tgt"].shape[0], t["tgt"].shape[2])
        off = {}
        for key in ("tgt", "pos"):          # 2 bytes into their parents: not 16-byte aligned
            parent = torch.zeros(t[key].numel() + 8, dtype=torch.bfloat16, device=DEV)
            parent[1:1 + t[key].numel()] = t[key].reshape(-1)
            off[key] = parent[1:1 + t[key].numel()].view_as(t[key])
            assert off[key].data_ptr() % 16 != 0
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = I.call("unipose", m, dict(t, **off))
        s.synchronize()
        assert calls() == before + 3
    assert torch.equal(bits(sf.transpose(0, 1)), bits(want))
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("flavour", I.FLAVOURS)
def test_routes_that_keep_the_composed_path(flavour, monkeypatch):
    t = I.to(I.make_inputs("small"), DEV)
    Lq, B = t["tgt"].shape[1], t["tgt"].shape[0]

    def composed_only(m, tt, grad=False, **kw):
        """switch on: no native call, and the result of the switch off"""
        with torch.enable_grad() if grad else torch.no_grad():
            monkeypatch.setattr(CLASSES[flavour], "native_layer", False)
            off = I.call(flavour, m, tt, **kw)
            monkeypatch.setattr(CLASSES[flavour], "native_layer", True)
            before = calls()
            assert I.applies(flavour, m, tt, **kw) != []
            on = I.call(flavour, m, tt, **kw)
            assert calls() == before
        first = lambda o: o[0] if isinstance(o, tuple) else o
        assert torch.equal(first(on), first(off))
        return on

    m = I.as_bf16(I.make_layer(flavour, "small"), DEV)
    monkeypatch.setattr(CLASSES[flavour], "native_layer", True)
    with torch.no_grad():
        before = calls()
        I.call(flavour, m, t)
        assert calls() == before + 1                        # the baseline: this module and these inputs do take the native call
    fmask = torch.zeros(Lq, Lq, dtype=torch.bfloat16, device=DEV).masked_fill(t["self_attn_mask"], float("-inf"))
    composed_only(m, dict(t, self_attn_mask=fmask))          # a float mask
    heads = I.SHAPES["small"]["M"]
    composed_only(m, dict(t, self_attn_mask=t["self_attn_mask"][None].expand(B * heads, Lq, Lq).contiguous()))   # a per-head (3-d) mask
    f32 = I.make_layer(flavour, "small").to(DEV)
    assert composed_only(f32, I.to(I.make_inputs("small"), DEV, torch.float32)).dtype == torch.float32
    assert composed_only(m, t, grad=True).requires_grad      # grad enabled, trainable parameters
    m.train()
    composed_reasons = I.applies(flavour, m, t)
    assert "active dropout" in composed_reasons
    m.eval()
    if flavour == "gdino":
        out = composed_only(m, t, output_attentions=True)
        assert isinstance(out, tuple) and len(out) == 4 and out[1].shape == (B, heads, Lq, Lq)
    d16 = I.as_bf16(I.make_layer(flavour, "small", heads=4), DEV)          # head dim 16
    composed_only(d16, t)
