"""GPU: the native Grounding-DINO decoder (include/vllm_hip.h, section f2d) -- its two row kernels alone against fp64, the whole decoder
through the class switch against the module's own fp64 run, an exact guarded workspace, offset views, bf16 reference points, a caller
stream, and the routes that keep the composed path.

Bounds.
  Sine embedding: |err| <= 1 bf16 ulp(ref) + 2^-19.  The absolute term is the argument's fp32 error through a slope of at most 1: |arg| < 8
  and its roundings (the product with the ratio, the product with 2 pi, the division) give at most 3 * 2^-24 * 8.  reference_points_input
  is one fp32 product: the bits of torch's.
  Box refinement: |err| <= 1/4 * 2^-17 * (sum_c |h w| + |b| + |logit(ref)|) + 2^-22, the project's GEMM term bound through sigmoid's slope
  of at most 1/4; 2^-22 is two fp32 roundings of a result in [0, 1] with room for expf / logf.
  Whole decoder: the layer tests' criterion on every intermediate[l] and intermediate_reference_points[l],
  rel_rms(native) <= max(1.05 rel_rms(composed bf16), 4e-3), both against deform_decoder_inputs.reference (fp64, CPU)."""
import math

import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import deformable_decoder as D

import deform_decoder_inputs as I
import workspace_guard as G
from bounds import DEV, P, bf16_ulp, rel_rms, stream

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def calls():
    return _lib.lib().vllm_deform_decoder_calls()


def layer_calls():
    return _lib.lib().vllm_deform_dec_layer_calls()


# ---- the reference-point kernel alone -----------------------------------------------------------------------------------------------------------
def run_embed(ref, vr, dim_t, Lv, Pf):
    """-> (reference_points_input [B, Lq, L, 4], the sine view [B Lq, 4 P], its NaN-prefilled parent with wider rows)"""
    B, Lq = ref.shape[:2]
    parent = torch.full((B * Lq, 4 * Pf + 24), float("nan"), dtype=torch.bfloat16, device=DEV)
    sine = parent[:, 8:8 + 4 * Pf]
    rpi = torch.full((B, Lq, Lv, 4), float("nan"), dtype=torch.float32, device=DEV)
    assert sine.data_ptr() % 16 == 0
    _lib.check(_lib.lib().vllm_refpoint_embed_bf16(P(ref), P(vr), P(dim_t), B, Lq, Lv, 4, Pf, P(rpi), P(sine), parent.stride(0), stream()),
               "vllm_refpoint_embed_bf16")
    torch.cuda.synchronize()
    return rpi, sine, parent


@pytest.mark.parametrize("Pf", [32, 128])
@pytest.mark.parametrize("Lv", [1, 4])
@pytest.mark.parametrize("rows", [1, 37, 130])
def test_refpoint_kernel_against_fp64(rows, Lv, Pf):
    B, Lq = (2, rows // 2) if rows % 2 == 0 else (1, rows)
    g = torch.Generator().manual_seed(rows * 100 + Lv * 10 + Pf)
    ref = torch.rand(B, Lq, 4, generator=g)
    special = torch.tensor([0.0, 0.5, 1.0, 0.5])
    ref.view(-1)[:4] = special          # row 0: the zero crossings of sin and cos at ref = 0.5 (ratio 1 below), and both ends
    if rows > 1:
        ref.view(-1)[4:8] = torch.tensor([1.0, 0.0, 0.5, 1.0])
    vr = 1.0 - 0.5 * torch.rand(B, Lv, 2, generator=g)
    vr[0, 0] = 1.0                      # so that level 0 of image 0 keeps 0, 0.5 and 1 exactly
    ref, vr = ref.to(DEV), vr.to(DEV)
    dim_t = D.GroundingDinoDecoder._dim_t(Pf, torch.device(DEV))
    rpi, sine, parent = run_embed(ref, vr, dim_t, Lv, Pf)
    what = f"refpoint rows {rows} L {Lv} P {Pf}"
    want_rpi = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
    assert torch.equal(bits(rpi), bits(want_rpi)), f"{what}: reference_points_input is not torch's fp32 product"
    assert torch.isnan(parent[:, :8]).all() and torch.isnan(parent[:, 8 + 4 * Pf:]).all(), f"{what}: wrote outside the 4 P columns"
    lvl0 = want_rpi[:, :, 0].double().cpu()
    dt = dim_t.double().cpu()
    even = torch.arange(Pf) % 2 == 0
    truth = torch.cat([torch.where(even, a.sin(), a.cos()) for a in (lvl0[:, :, k, None] * (2 * math.pi) / dt for k in (1, 0, 2, 3))], -1)
    truth = truth.reshape(rows, 4 * Pf)
    got = sine.double().cpu()
    assert torch.isfinite(got).all()
    excess = ((got - truth).abs() - 2.0 ** -19).clamp_min(0) / bf16_ulp(truth)
    print(f"{what}: max excess {excess.max().item():.3f} bf16 ulp, max |err| {(got - truth).abs().max().item():.3e}")
    assert excess.max().item() <= 1.0, what
    # the exact inputs: sin(0) = 0 and cos(0) = 1 in every feature of x = 0
    assert torch.equal(got[0, Pf:2 * Pf], torch.where(even, 0.0, 1.0).double())
    rpi2, sine2, _ = run_embed(ref, vr, dim_t, Lv, Pf)
    assert torch.equal(bits(sine), bits(sine2)) and torch.equal(bits(rpi), bits(rpi2)), f"{what}: two runs differ"


# ---- the refine kernel alone -------------------------------------------------------------------------------------------------------------------
EPS = 1e-5
SPECIAL = (0.0, 1.0, 1e-6, 1.0 - 1e-6, -0.1, 1.1, 0.5)


def run_refine(h, W, b, ref, out):
    R, C = h.shape
    _lib.check(_lib.lib().vllm_box_refine_f32(P(h), h.stride(0), P(W), P(b), P(ref), P(out), R, C, EPS, stream()), "vllm_box_refine_f32")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("R", [1, 37, 130])
def test_refine_kernel_against_fp64(R, C):
    g = torch.Generator().manual_seed(R * 1000 + C)
    parent = torch.randn(R, C + 16, generator=g).relu().to(torch.bfloat16).to(DEV)          # rows wider than C
    h = parent[:, 8:8 + C]
    W = (0.1 * torch.randn(4, C, generator=g)).to(torch.bfloat16).to(DEV)
    b = (0.1 * torch.randn(4, generator=g)).to(torch.bfloat16).to(DEV)
    assert h.data_ptr() % 16 == 0 and h.stride(0) == C + 16
    base = torch.rand(R, 4, generator=g)
    # every special value in every case: R = 1 has four slots, so it runs twice
    for chunk in ([SPECIAL] if R > 1 else [SPECIAL[:4], SPECIAL[4:]]):
        ref = base.clone()
        ref.view(-1)[:len(chunk)] = torch.tensor(chunk)
        ref = ref.to(DEV)
        what = f"refine R {R} C {C} specials {chunk[0]}.."
        got = run_refine(h, W, b, ref, torch.full_like(ref, float("nan")))
        h64, W64, b64, r64 = h.double().cpu(), W.double().cpu(), b.double().cpu(), ref.double().cpu()
        eps64 = float(torch.tensor(EPS, dtype=torch.float32))
        x = r64.clamp(0, 1)
        logit = torch.log(x.clamp(min=eps64) / (1 - x).clamp(min=eps64))
        truth = torch.sigmoid(h64 @ W64.T + b64 + logit)
        mag = h64.abs() @ W64.abs().T + b64.abs() + logit.abs()
        err = (got.double().cpu() - truth).abs()
        bound = 0.25 * 2.0 ** -17 * mag + 2.0 ** -22
        print(f"{what}: max |err| {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}")
        assert torch.isfinite(got).all() and (err <= bound).all(), what
        alias = ref.clone()
        run_refine(h, W, b, alias, alias)
        assert torch.equal(bits(alias), bits(got)), f"{what}: the in-place form differs"
        again = run_refine(h, W, b, ref, torch.full_like(ref, float("nan")))
        assert torch.equal(bits(again), bits(got)), f"{what}: two runs differ"


# ---- the whole decoder -------------------------------------------------------------------------------------------------------------------------
def judged(native, composed, truth, what):
    e, ec = rel_rms(native.cpu(), truth), rel_rms(composed.cpu(), truth)
    print(f"{what}: rel rms native {e:.3e}, composed bf16 {ec:.3e}")
    assert torch.isfinite(native.float()).all()
    assert e <= max(1.05 * ec, 4e-3), (what, e, ec)


def check_outputs(out, t):
    last, inter, irp = out
    Lq = t["tgt"].shape[1]
    assert last.dtype == torch.bfloat16 and last.shape == (I.B, Lq, I.C)
    assert inter.dtype == torch.bfloat16 and inter.shape == (I.B, I.LAYERS, Lq, I.C)
    assert irp.dtype == t["reference_points"].dtype and irp.shape == (I.B, I.LAYERS, Lq, 4)
    assert torch.equal(last, inter[:, -1])


@pytest.mark.parametrize("case", I.CASES, ids=I.IDS)
def test_decoder_through_the_switch_against_its_own_fp64_run(case, monkeypatch):
    Lq, with_masks, box = case
    m = I.as_bf16(I.make_decoder(box), DEV)
    t = I.to(I.make_inputs(Lq, with_masks), DEV)
    truth_inter, truth_ref = I.reference(*case)
    with torch.no_grad():
        before, before_layer = calls(), layer_calls()
        composed = I.call(m, t)
        assert (calls(), layer_calls()) == (before, before_layer) and m.native_decoder is False
        monkeypatch.setattr(D.GroundingDinoDecoder, "native_decoder", True)
        assert I.reasons(m, t) == []
        native = I.call(m, t)
        assert calls() == before + 1
        again = I.call(m, t)
        assert calls() == before + 2 and layer_calls() == before_layer          # the layer entry's counter is not touched
    assert isinstance(native, tuple) and len(native) == 3
    check_outputs(native, t)
    check_outputs(composed, t)
    assert not native[1].is_contiguous() and native[1].transpose(0, 1).is_contiguous()          # views of the layer-major buffers
    for a, b in zip(native, again):
        assert torch.equal(bits(a), bits(b)), f"{case}: two runs differ"
    for l in range(I.LAYERS):
        judged(native[1][:, l], composed[1][:, l], truth_inter[:, l], f"{I.IDS[I.CASES.index(case)]} intermediate[{l}]")
        judged(native[2][:, l], composed[2][:, l], truth_ref[:, l], f"{I.IDS[I.CASES.index(case)]} reference_points[{l}]")
    if box is None:
        assert torch.equal(native[2], t["reference_points"][:, None].expand(-1, I.LAYERS, -1, -1))
    else:
        assert not torch.equal(native[2][:, 0], native[2][:, 1])


def test_return_dict_and_bf16_reference_points(monkeypatch):
    m = I.as_bf16(I.make_decoder("shared"), DEV)
    t = I.to(I.make_inputs(37), DEV)
    monkeypatch.setattr(D.GroundingDinoDecoder, "native_decoder", True)
    with torch.no_grad():
        tup = I.call(m, t)
        before = calls()
        out = I.call(m, t, return_dict=True)
        assert calls() == before + 1
        assert isinstance(out, D.GroundingDinoDecoderOutput) and out.hidden_states is None and out.attentions is None
        for a, b in zip((out.last_hidden_state, out.intermediate_hidden_states, out.intermediate_reference_points), tup):
            assert torch.equal(a, b)
        # bf16 reference points: widened once on entry, fp32 through every layer, returned in the caller's dtype
        tb = dict(t, reference_points=t["reference_points"].to(torch.bfloat16), valid_ratios=t["valid_ratios"].to(torch.bfloat16))
        assert I.reasons(m, tb) == []
        got = I.call(m, tb)
        assert calls() == before + 2
        want = I.call(m, dict(t, reference_points=tb["reference_points"].float(), valid_ratios=tb["valid_ratios"].float()))
    check_outputs(got, tb)
    assert torch.equal(bits(got[1]), bits(want[1])) and torch.equal(bits(got[2]), bits(want[2].to(torch.bfloat16)))


@pytest.mark.parametrize("fill", [G.HOSTILE, G.PLAUSIBLE], ids=["hostile", "plausible"])
def test_exact_workspace_with_guards(fill, monkeypatch):
    """The C entry with exactly the queried bytes, 16-byte aligned and no better, whatever they held: the bits of a clean run, guards intact."""
    m = I.as_bf16(I.make_decoder("per_layer"), DEV)
    t = I.to(I.make_inputs(70), DEV)
    monkeypatch.setattr(D.GroundingDinoDecoder, "native_decoder", True)
    with torch.no_grad():
        want = I.call(m, t)
    checks = []

    def exact(device, nbytes, what, slot=0):
        _lib.check(0 if nbytes >= 0 else -1, what)
        assert nbytes > 0 and what == "vllm_deform_decoder_workspace_bytes"
        _, n, check = G.guarded(nbytes, fill, skew=16, widest_row_bytes=4 * I.NPOS * 2)
        checks.append(check)
        return check.workspace, n
    monkeypatch.setattr(_lib, "sized_workspace", exact)
    with torch.no_grad():
        before = calls()
        got = I.call(m, t)
        assert calls() == before + 1
    assert len(checks) == 1 and checks[0].workspace.data_ptr() % 32 == 16
    checks[0]()
    for a, b in zip(got, want):
        assert torch.equal(bits(a), bits(b))


def test_offset_views_and_a_caller_stream(monkeypatch):
    """inputs that are views 2 or 4 bytes into their parents (not 16-byte aligned), on a side stream: the same bits"""
    m = I.as_bf16(I.make_decoder("shared"), DEV)
    t = I.to(I.make_inputs(70), DEV)
    monkeypatch.setattr(D.GroundingDinoDecoder, "native_decoder", True)
    off = {}
    for key in ("tgt", "memory", "memory_text", "reference_points", "valid_ratios"):
        parent = torch.zeros(t[key].numel() + 8, dtype=t[key].dtype, device=DEV)
        parent[1:1 + t[key].numel()] = t[key].reshape(-1)
        off[key] = parent[1:1 + t[key].numel()].view_as(t[key])
        assert off[key].data_ptr() % 16 != 0
    with torch.no_grad():
        want = I.call(m, t)
        before = calls()
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = I.call(m, dict(t, **off))
        s.synchronize()
        assert calls() == before + 1
    for a, b in zip(got, want):
        assert torch.equal(bits(a), bits(b))


def test_the_layers_keep_their_own_switch_when_the_decoder_switch_is_off(monkeypatch):
    m = I.as_bf16(I.make_decoder("shared"), DEV)
    t = I.to(I.make_inputs(37), DEV)
    monkeypatch.setattr(D.GroundingDinoDecoderLayer, "native_layer", True)
    with torch.no_grad():
        before, before_layer = calls(), layer_calls()
        out = I.call(m, t)
        assert calls() == before and layer_calls() == before_layer + I.LAYERS
    check_outputs(out, t)
    assert out[1].is_contiguous()          # the composed path stacks


def test_routes_that_keep_the_composed_path(monkeypatch):
    t = I.to(I.make_inputs(37), DEV)
    cls = D.GroundingDinoDecoder

    def composed_only(m, tt, grad=False, **kw):
        """switch on: no native call, and the result of the switch off"""
        with torch.enable_grad() if grad else torch.no_grad():
            monkeypatch.setattr(cls, "native_decoder", False)
            off = I.call(m, tt, **kw)
            monkeypatch.setattr(cls, "native_decoder", True)
            before, before_layer = calls(), layer_calls()
            assert I.reasons(m, tt, **kw) != []
            on = I.call(m, tt, **kw)
            assert (calls(), layer_calls()) == (before, before_layer)
        for a, b in zip(on[:3], off[:3]):
            assert torch.equal(bits(a.detach()), bits(b.detach()))
        return on

    m = I.as_bf16(I.make_decoder("shared"), DEV)
    monkeypatch.setattr(cls, "native_decoder", True)
    with torch.no_grad():
        before = calls()
        I.call(m, t)
        assert calls() == before + 1                        # the baseline: this module and these inputs do take the native call
    out = composed_only(m, t, output_attentions=True)
    assert len(out) == 4 and len(out[3]) == 3 and out[3][0][0].shape == (I.B, I.HEADS, 37, 37)
    out = composed_only(m, t, output_hidden_states=True)
    assert len(out) == 4 and len(out[3]) == I.LAYERS + 1
    assert composed_only(m, t, grad=True)[0].requires_grad                  # grad enabled, trainable parameters
    fmask = torch.zeros(37, 37, dtype=torch.bfloat16, device=DEV).masked_fill(t["self_attn_mask"], float("-inf"))
    composed_only(m, dict(t, self_attn_mask=fmask))                         # a reason of the layers': a float mask
    f32 = I.make_decoder("shared").to(DEV)
    assert composed_only(f32, I.to(I.make_inputs(37), DEV, torch.float32))[0].dtype == torch.float32
    m.query_scale = torch.nn.Identity()
    composed_only(m, t)
    m.query_scale = None
    two = I.as_bf16(I.make_decoder(), DEV)
    two.bbox_embed = [D.GroundingDinoMLPPredictionHead(I.C, I.C, 4, 2).to(DEV).to(torch.bfloat16)] * I.LAYERS          # two-layer heads
    composed_only(two, t)
    still = I.as_bf16(I.make_decoder("shared", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0), DEV)
    still.train()                                                           # training mode (no dropout, so that two runs agree)
    composed_only(still, t)
    with torch.no_grad():
        before = calls()
        I.call(m, t)
        assert calls() == before + 1                        # and the module still takes the native call afterwards
