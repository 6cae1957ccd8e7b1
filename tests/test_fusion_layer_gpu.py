"""GPU: the native fusion layer (include/vllm_hip.h, section f2f) -- the cross-attention kernel alone against fp64 with one split and with
the keys split, the whole layer through the class switch against the module's own fp64 run, an image without a text token, an exact
guarded workspace, offset views, a caller stream, and the routes that keep the composed path.

Bounds.  Attention kernel: the bound of test_deform_decoder_layer_gpu.judge_mha, |err| <= 1 bf16 ulp(ref) + 2^-8 sum_j p_j |v_j| (P is
rounded to bf16 before P V, fp32 accumulation, one rounding of the result); a row whose every key is masked must be NaN in all D outputs
of every head and no other element may be.  Whole layer: the decoder layer's criterion, for each of the two outputs
rel_rms(native) <= max(1.05 rel_rms(composed bf16), 4e-3), both against fusion_layer_inputs.reference (fp64, CPU)."""
import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import fusion_layer as FL

import fusion_layer_inputs as I
import workspace_guard as G
from bounds import DEV, P, bf16_ulp, rel_rms, stream

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view(torch.int16)


def nan_bf16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=DEV)


def calls():
    return _lib.lib().vllm_fusion_layer_calls()


@pytest.fixture
def switch(monkeypatch):
    monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", True)


# ---- the attention kernel alone -----------------------------------------------------------------------------------------------------------------
def packed_operands(D, Lq, Lk, H, B):
    """q, k, v as offset views of packed parents with three different row strides -> (q, k, v), each [B, L, H D] with stride(2) == 1"""
    C = H * D
    q, k, v = (x.to(DEV) for x in I.xattn_inputs(D, Lq, Lk, H, B))
    qp = torch.randn(B, Lq, 2 * C + 8, device=DEV).to(torch.bfloat16)
    kvp = torch.randn(B, Lk, 2 * C + 24, device=DEV).to(torch.bfloat16)
    vp = torch.randn(B, Lk, C + 16, device=DEV).to(torch.bfloat16)
    qv, kv, vv = qp[:, :, C:2 * C], kvp[:, :, 8:8 + C], vp[:, :, 16:16 + C]
    qv.copy_(q), kv.copy_(k), vv.copy_(v)
    for t in (qv, kv, vv):
        assert t.data_ptr() % 16 == 0 and t.stride(2) == 1
    assert len({qv.stride(1), kv.stride(1), vv.stride(1)}) == 3
    return qv, kv, vv


def run_xattn(q, k, v, kp, H, D, want_splits):
    """-> (the [B, Lq, H D] output view, its NaN-prefilled parent with wider rows); the plan is asserted before the launch"""
    B, Lq, C = q.shape
    Lk = k.shape[1]
    L = _lib.lib()
    splits, kps = I.plan(B, Lq, Lk, H, D)
    assert splits == want_splits and kps % I.KEY_TILE == 0 and (splits == 1 or Lk - 2 * kps == 1)
    need = L.vllm_xattn_workspace_bytes(B, Lq, Lk, H, D)
    assert (need > 0) == (splits > 1)
    ws = nan_bf16(need // 2) if need else None          # hostile content: every partial slot a NaN until its split writes it
    parent = nan_bf16(B, Lq, C + 40)
    out = parent[:, :, 32:32 + C]
    kp8 = None if kp is None else kp.to(DEV).to(torch.uint8).contiguous()
    _lib.check(L.vllm_xattn_fwd_bf16(P(q), q.stride(0), q.stride(1), P(k), k.stride(0), k.stride(1), P(v), v.stride(0), v.stride(1), P(out),
                                     out.stride(0), out.stride(1), P(kp8), B, Lq, Lk, H, D, D ** -0.5, P(ws), need, stream()),
               "vllm_xattn_fwd_bf16")
    torch.cuda.synchronize()
    return out, parent


def judge_xattn(out, parent, D, Lq, Lk, H, B, pattern, what):
    C = H * D
    ref, mag, share, _ = I.xattn_reference(D, Lq, Lk, H, B, pattern)
    assert torch.isnan(parent[:, :, :32]).all() and torch.isnan(parent[:, :, 32 + C:]).all(), f"{what}: wrote outside the H D columns"
    got = out.cpu().double().reshape(B, Lq, H, D)
    dead = torch.isnan(ref)
    dead_rows = dead.all(-1).all(-1)                       # [B, Lq]: the mask does not depend on the head
    assert torch.equal(dead, dead_rows[:, :, None, None].expand_as(dead))
    assert torch.equal(torch.isnan(got), dead), f"{what}: NaN exactly where every key of the row is masked"
    live = ~dead
    err = (got - ref).abs()[live]
    u = ((err - 2.0 ** -8 * mag[live]).clamp_min(0) / bf16_ulp(ref[live])).max().item() if live.any() else 0.0
    print(f"{what}: masked keys {share:.3f}, rows with every key masked {int(dead_rows.sum())}, max excess {u:.3f} bf16 ulp")
    assert u <= 1.0, what
    return dead_rows


@pytest.mark.parametrize("case", I.xattn_cases(), ids=lambda c: "D{}-{}x{}-H{}-B{}".format(*c[:5]))
def test_xattn_kernel_against_fp64(case):
    """Without a mask and with each key-mask pattern the shape can carry; two runs of every case bit-identical."""
    D, Lq, Lk, H, B, long_keys = case
    torch.manual_seed(D + Lq + Lk + H + B)
    q, k, v = packed_operands(D, Lq, Lk, H, B)
    splits, kps = I.plan(B, Lq, Lk, H, D)
    for pattern in I.patterns(Lk, long_keys):
        kp, _, dead_images = I.key_mask(pattern, B, Lk, kps)
        what = f"xattn D{D} {Lq}x{Lk} H{H} B{B} {pattern}"
        out, parent = run_xattn(q, k, v, kp, H, D, 3 if long_keys else 1)
        dead_rows = judge_xattn(out, parent, D, Lq, Lk, H, B, pattern, what)
        again, _ = run_xattn(q, k, v, kp, H, D, 3 if long_keys else 1)
        assert torch.equal(bits(out), bits(again)), f"{what}: two runs differ"
        assert sorted(set(dead_rows.nonzero()[:, 0].tolist())) == dead_images and all(dead_rows[b].all() for b in dead_images)


@pytest.mark.parametrize("long_keys", [False, True], ids=["one_split", "split"])
def test_xattn_kernel_on_a_caller_stream(long_keys):
    D, Lq, H, B = 256, 65, 3, 2
    Lk = I.lk3(B, Lq, H, D) if long_keys else 65
    q, k, v = packed_operands(D, Lq, Lk, H, B)
    kp, _, _ = I.key_mask("ragged", B, Lk)
    want, _ = run_xattn(q, k, v, kp, H, D, 3 if long_keys else 1)
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got, parent = run_xattn(q, k, v, kp, H, D, 3 if long_keys else 1)
    s.synchronize()
    assert torch.equal(bits(got), bits(want))
    judge_xattn(got, parent, D, Lq, Lk, H, B, "ragged", "xattn on a side stream")


# ---- the whole layer ----------------------------------------------------------------------------------------------------------------------------
def judged(native, composed, truth, what):
    """rel rms over the elements where the fp64 run is finite; NaN exactly where it is NaN"""
    dead = torch.isnan(truth)
    got, comp = native.cpu().double(), composed.cpu().double()
    assert torch.equal(torch.isnan(got), dead), f"{what}: NaN exactly where the fp64 run is NaN"
    assert torch.isfinite(got[~dead]).all()
    z = lambda x: torch.where(dead, torch.zeros_like(truth), torch.nan_to_num(x))
    e, ec = rel_rms(z(got), z(truth)), rel_rms(z(comp), z(truth))
    print(f"{what}: rel rms native {e:.3e}, composed bf16 {ec:.3e}, NaN elements {int(dead.sum())}")
    assert e <= max(1.05 * ec, 4e-3), (what, e, ec)


def through_the_switch(m, t, truth, what, monkeypatch):
    with torch.no_grad():
        before = calls()
        cv, ct, cw = I.call(m, t)
        assert calls() == before and m.native_layer is False and cw[0] is not None and cw[1] is not None
        monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", True)
        assert I.reasons(m, t) == []
        nv, nt, nw = I.call(m, t)
        assert calls() == before + 1
        av, at_, _ = I.call(m, t)
        assert calls() == before + 2
    assert nw == (None, None)          # the [B H, S, Lt] weight tensors are never built
    for n, x in ((nv, t["vision"]), (nt, t["text"])):
        assert n.dtype == torch.bfloat16 and n.shape == x.shape
    assert torch.equal(bits(nv), bits(av)) and torch.equal(bits(nt), bits(at_))
    judged(nv, cv, truth[0], what + " vision")
    judged(nt, ct, truth[1], what + " text")
    return nv, nt


@pytest.mark.parametrize("name,masks", I.LAYER_CASES, ids=[f"{s}-{m}" for s, m in I.LAYER_CASES])
def test_layer_through_the_switch_against_its_own_fp64_run(name, masks, monkeypatch):
    sh = I.shape_of(name)
    assert I.plan(sh.B, sh.Lt, sh.S, sh.H, sh.D)[0] == (3 if name == "split" else 1)
    m = I.as_bf16(I.make_layer(name), DEV)
    t = I.to(I.make_inputs(name, masks), DEV)
    truth = I.reference(name, masks)
    nv, _ = through_the_switch(m, t, truth, f"{name} {masks}", monkeypatch)
    if masks == I.DEAD:          # image 1 has no text token: its vision output is NaN, image 0's and the text output are not
        assert torch.isnan(nv[1]).all() and not torch.isnan(nv[0]).any() and torch.isnan(truth[0][1]).all()


@pytest.mark.parametrize("name", list(I.LAYER_SHAPES))
@pytest.mark.parametrize("fill", [G.HOSTILE, G.PLAUSIBLE], ids=["hostile", "plausible"])
def test_exact_workspace_with_guards(name, fill, switch, monkeypatch):
    """The C entry with exactly the queried bytes, 16-byte aligned and no better, whatever they held: the bits of a clean run, guards intact."""
    sh = I.shape_of(name)
    m = I.as_bf16(I.make_layer(name), DEV)
    t = I.to(I.make_inputs(name, "both"), DEV)
    with torch.no_grad():
        want = I.call(m, t)
    checks = []

    def exact(device, nbytes, what, slot=0):
        _lib.check(0 if nbytes >= 0 else -1, what)
        assert nbytes > 0
        _, n, check = G.guarded(nbytes, fill, skew=16, widest_row_bytes=sh.E * 2)
        checks.append(check)
        return check.workspace, n
    monkeypatch.setattr(_lib, "sized_workspace", exact)
    with torch.no_grad():
        before = calls()
        got = I.call(m, t)
        assert calls() == before + 1
    assert len(checks) == 1 and checks[0].workspace.data_ptr() % 32 == 16
    checks[0]()
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))


def test_offset_views_and_a_caller_stream(switch):
    """Inputs that are views 2 bytes into their parents (not 16-byte aligned) and rows of a wider parent, on a side stream: the same bits."""
    name = "split"
    m = I.as_bf16(I.make_layer(name), DEV)
    t = I.to(I.make_inputs(name, "both"), DEV)
    with torch.no_grad():
        before = calls()
        want = I.call(m, t)
        off = {}
        for key in ("vision", "text"):
            parent = torch.zeros(t[key].numel() + 8, dtype=torch.bfloat16, device=DEV)
            parent[1:1 + t[key].numel()] = t[key].reshape(-1)
            off[key] = parent[1:1 + t[key].numel()].view_as(t[key])
            assert off[key].data_ptr() % 16 != 0
        wide = torch.zeros(*t["vision"].shape[:2], t["vision"].shape[2] + 8, dtype=torch.bfloat16, device=DEV)
        wide[:, :, 8:] = t["vision"]
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = I.call(m, dict(t, **off))
            got2 = I.call(m, dict(t, vision=wide[:, :, 8:]))
        s.synchronize()
        assert calls() == before + 3
    for g in (got, got2):
        assert torch.equal(bits(g[0]), bits(want[0])) and torch.equal(bits(g[1]), bits(want[1]))


def test_routes_that_keep_the_composed_path(monkeypatch):
    name = "one_split"
    t = I.to(I.make_inputs(name, "both"), DEV)

    def composed_only(m, tt, grad=False):
        """switch on: no native call, and the result of the switch off"""
        with torch.enable_grad() if grad else torch.no_grad():
            monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", False)
            off = I.call(m, tt)
            monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", True)
            before = calls()
            assert I.reasons(m, tt) != []
            on = I.call(m, tt)
            assert calls() == before
        assert on[2][0] is not None and torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
        return on

    m = I.as_bf16(I.make_layer(name), DEV)
    monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", True)
    with torch.no_grad():
        before = calls()
        I.call(m, t)
        assert calls() == before + 1                        # the baseline: this module and these inputs do take the native call
    f32 = I.copy.deepcopy(I.make_layer(name)).to(DEV)
    assert composed_only(f32, I.to(I.make_inputs(name, "both"), DEV, torch.float32))[0].dtype == torch.float32
    assert composed_only(m, t, grad=True)[0].requires_grad      # grad enabled, trainable parameters
    m.train()
    assert "training mode" in I.reasons(m, t)
    composed_only(m, t)
    m.eval()
    d64 = FL.GroundingDinoFusionLayer(I.config(name, encoder_attention_heads=8)).to(DEV).to(torch.bfloat16).eval()          # head dim 64
    assert d64.attn.head_dim == 64
    composed_only(d64, t)
