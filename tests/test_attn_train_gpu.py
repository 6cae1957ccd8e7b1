"""GPU: training through the FlashAttention hook (bring-up hook B4) -- the training forward (``vllm_attn_fwd_train_qkvpacked_*``:
the inference kernel's ``out`` bits plus the row log-sum-exp) and the native backward (``vllm_attn_bwd_qkvpacked_*``), through the C
ABI and through the hook's autograd node.  The yardstick is torch's fp64 autograd of the reference's ``_naive_attn`` statements on
the same 16-bit-rounded tensors (attn_train_inputs.py), never the code under test; per element with the derived bounds of that
module, and as a whole tensor against torch's own 16-bit autograd of the same statements (the parity contract, DESIGN section 5:
relative rms error against fp64 at most 1.25 x torch's)."""
import pytest
import torch
from torch import nn

import attn_train_inputs as ati
from bounds import P, stream
from visionllm_amd import _lib
from visionllm_amd.flash_attention import FlashAttention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S_GRID = [1, 5, 32, 33, 63, 64, 65, 97, 128, 129, 193, 257, 577, 1025]
DTYPES = [torch.bfloat16, torch.float16]
# Whole-tensor contract: rel rms against fp64 <= 1.25 x torch's 16-bit autograd.  At S = 1 -- and only there -- torch's error is EXACTLY
# zero (softmax of one score is 1, dS = 0 * anything, dV = dO), while dS = p (dO.v - delta) here is the difference of two fp32 sums of
# the same terms in two orders (MFMA chain / dot2 chain): ~2^-24 relative, measured 1.1e-8 of the tensor.  The ratio cannot resolve
# that, so at S = 1 it stops at fp32 accumulation's own resolution, 2^-20 of the tensor's rms -- 2^-12 of a bf16 spacing.
RMS_FLOOR_S1 = 2.0 ** -20
B, H = 3, 3          # 9 (batch, head) pairs: one full group of 8 on the XCDs and a group with one live member


def entry(name, dtype):
    return getattr(_lib.lib(), name + ("_f16" if dtype == torch.float16 else "_bf16"))


def fwd_train(qkv, scale):
    """-> (out, lse) through the C ABI; both pre-filled with NaN."""
    Bq, S, _, Hq, D = qkv.shape
    out = torch.full((Bq, S, Hq, D), float("nan"), dtype=qkv.dtype, device=qkv.device)
    lse = torch.full((Bq, Hq, S), float("nan"), dtype=torch.float32, device=qkv.device)
    _lib.check(entry("vllm_attn_fwd_train_qkvpacked", qkv.dtype)(P(qkv), P(out), P(lse), Bq, S, Hq, D, scale, stream()))
    return out, lse


def fwd_infer(qkv, scale):
    Bq, S, _, Hq, D = qkv.shape
    out = torch.full((Bq, S, Hq, D), float("nan"), dtype=qkv.dtype, device=qkv.device)
    _lib.check(entry("vllm_attn_fwd_qkvpacked", qkv.dtype)(P(qkv), P(out), Bq, S, Hq, D, scale, stream()))
    return out


def bwd(qkv, out, lse, dout, scale, expect=0, ws=None, ws_bytes=None, grad=None):
    """-> grad_qkv through the C ABI, pre-filled with NaN: every element must be written."""
    Bq, S, _, Hq, D = qkv.shape
    L = _lib.lib()
    need = L.vllm_attn_bwd_workspace_bytes(Bq, S, Hq, D)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=qkv.device)
    g = torch.full(tuple(qkv.shape), float("nan"), dtype=qkv.dtype, device=qkv.device) if grad is None else grad
    rc = entry("vllm_attn_bwd_qkvpacked", qkv.dtype)(P(qkv), P(out), P(lse), P(dout), Bq, S, Hq, D, scale, P(g), P(ws),
                                                     need if ws_bytes is None else ws_bytes, stream())
    assert rc == expect, (rc, L.vllm_last_error().decode())
    torch.cuda.synchronize()
    return g


def hook_grads(qkv, dout, **kw):
    x = qkv.detach().clone().requires_grad_(True)
    out, _ = FlashAttention(**kw)(x)
    assert out.grad_fn is not None
    out.backward(dout)
    return out.detach(), x.grad


def check_grads(name, S, D, dtype, hook=True):
    qkv, dout = (t.to(DEV) for t in ati.case(name, B, S, H, D, dtype))
    scale = D ** -0.5
    ref, bound, _ = ati.grad_bounds(qkv, dout, scale, dtype)           # fp64, on the device
    out, lse = fwd_train(qkv, scale)
    g = bwd(qkv, out, lse, dout, scale)
    assert torch.isfinite(g.float()).all(), f"{name} S{S} D{D} {dtype}: grad_qkv has unwritten or non-finite elements"
    worst, at = ati.worst_factor(g, ref, bound)
    _, g16 = ati.autograd_grads(qkv, dout, scale, dtype)               # torch's own 16-bit autograd of _naive_attn
    ours, theirs = ati.rel_rms(g, ref), ati.rel_rms(g16, ref)
    print(f"attn_bwd {name} S{S} D{D} {dtype}: {worst:.3f} of the per-element bound; rel rms {ours:.3e} (torch 16-bit {theirs:.3e})")
    assert worst <= 1.0, f"{name} S{S} D{D} {dtype}: {worst:.2f} x the bound at flat element {at} (q/k/v index {(at // (H * D)) % 3})"
    yard = theirs
    if name == "near_one_hot" and dtype == torch.float16:       # (see test_gradients_on_the_extreme_cases)
        yard = max(theirs, ati.rel_rms(ati.emulate(qkv, dout, scale, dtype)[2], ref))
    limit = max(1.25 * yard, RMS_FLOOR_S1 if S == 1 else 0.0)
    assert ours <= limit, f"{name} S{S} D{D} {dtype}: rel rms {ours:.3e} > 1.25 x {yard:.3e} (torch's 16-bit autograd: {theirs:.3e})"
    if hook:
        out_h, g_h = hook_grads(qkv, dout)
        assert torch.equal(out_h, out) and torch.equal(g_h, g), "the hook does not give the C ABI's bits"


@pytest.mark.parametrize("variant", [32, 194, 1090])
@pytest.mark.parametrize("D", [64, 128])
def test_training_forward_same_out_bits_and_lse(D, variant):
    """Every schedule the launcher can pick (class-token split on / off / keys only, the spare-wave class row, trimmed waves, ragged
    tiles, S = 1): out is the inference call's bit for bit, every lse element is written and within the bound of the fp64 value."""
    old = _lib.set_option("attn_variant", variant)
    try:
        for S in S_GRID:
            for dtype in (DTYPES if S in (1, 65, 129, 577, 1025) else DTYPES[:1]):
                for name in (("random", "key0_dominant", "key0_far_below") if S in (65, 577, 1025) else ("random",)):
                    qkv = ati.case(name, B, S, H, D, dtype)[0].to(DEV)
                    scale = D ** -0.5
                    out, lse = fwd_train(qkv, scale)
                    assert torch.equal(out, fwd_infer(qkv, scale)), f"{name} S{S} {dtype}: out differs from the inference call"
                    assert torch.isfinite(lse).all(), f"{name} S{S} {dtype}: lse has unwritten elements"
                    q, k, _ = ati._split(qkv)
                    ref = torch.logsumexp(scale * (q @ k.transpose(-2, -1)), -1)
                    err = float((lse.double() - ref).abs().max())
                    print(f"attn_fwd_train variant {variant} {name} S{S} D{D} {dtype}: lse {err / ati.lse_bound(dtype):.3f} of the bound")
                    assert err <= ati.lse_bound(dtype), f"{name} S{S} {dtype}: lse off by {err:.3e}"
    finally:
        _lib.set_option("attn_variant", old)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", S_GRID)
def test_gradients_against_fp64_autograd(S, D, dtype):
    check_grads("random", S, D, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [65, 577])
@pytest.mark.parametrize("name", [c for c in ati.CASES if c != "random"])
def test_gradients_on_the_extreme_cases(name, S, D, dtype):
    """Per element and as a whole tensor on every case, through the C ABI and through the hook.  One yardstick differs: for
    ``near_one_hot`` in fp16 the whole-tensor limit is 1.25 x the LARGER of torch's 16-bit autograd and the CPU emulation of the
    contract's own rounding points (attn_train_inputs.emulate).  There the true dQ and dK are ~0 (dS -> 0 is the point of the case) and
    what either implementation returns for them is cancellation residue, ~50 % (here) and ~35 % (torch) of their rms: delta read from
    the ROUNDED out -- the e_i term of the per-element bound, of which 0.34 is used -- cancels less exactly against dO.v than the naive
    path's sum over its own rounded P.  At S 65 / D 64 that is 9.376e-05 against torch's 7.037e-05, a ratio of 1.33, and the emulation
    gives 9.375e-05: the figure belongs to the contract's delta, not to the kernel, and no kernel that follows the contract can meet
    1.25 x torch there.  Every other (case, S, D, dtype) is held to 1.25 x torch's (measured <= 1.21; bf16 near_one_hot 1.19)."""
    check_grads(name, S, D, dtype)


def test_softmax_scale_and_empty_batch():
    qkv, dout = (t.to(DEV) for t in ati.case("random", 2, 97, 2, 64, torch.bfloat16))
    ref, bound, _ = ati.grad_bounds(qkv, dout, 0.2, torch.bfloat16)
    _, g = hook_grads(qkv, dout, softmax_scale=0.2)
    assert ati.worst_factor(g, ref, bound)[0] <= 1.0
    e = torch.empty(0, 97, 3, 2, 64, dtype=torch.bfloat16, device=DEV, requires_grad=True)
    out, _ = FlashAttention()(e)
    out.sum().backward()
    assert e.grad.shape == e.shape


@pytest.mark.parametrize("D,S", [(64, 577), (128, 1025)])
def test_backward_40_launches_identical(D, S):
    """The form of test_race_screen_gpu.py: fresh NaN-filled outputs every launch, every result equal to the first bit for bit."""
    qkv, dout = (t.to(DEV) for t in ati.case("spiked_key", 4, S, 4, D, torch.bfloat16))
    scale = D ** -0.5
    out, lse = fwd_train(qkv, scale)
    first = bwd(qkv, out, lse, dout, scale)
    assert torch.isfinite(first.float()).all()
    for i in range(40):
        again = bwd(qkv, out, lse, dout, scale)
        assert torch.equal(again.view(torch.int16), first.view(torch.int16)), f"launch {i} differs from the first"


def test_autograd_plumbing():
    qkv = ati.case("random", 2, 129, 2, 64, torch.bfloat16)[0].to(DEV)
    m = FlashAttention()
    base, _ = m(qkv)
    assert base.grad_fn is None and not base.requires_grad
    out, _ = m(qkv.clone().requires_grad_(True))
    assert out.grad_fn is not None and torch.equal(out, base)
    with torch.no_grad():
        o, _ = m(qkv.clone().requires_grad_(True))
    assert o.grad_fn is None and torch.equal(o, base)
    with torch.inference_mode():
        o, _ = m(qkv.clone())
    assert torch.equal(o, base)
    m.train()                                       # training mode with dropout 0 is the supported training call
    out, _ = m(qkv.clone().requires_grad_(True))
    assert out.grad_fn is not None
    with pytest.raises(NotImplementedError):
        m(qkv.clone().requires_grad_(True), causal=True)
    with pytest.raises(NotImplementedError):
        FlashAttention(attention_dropout=0.1).train()(qkv.clone().requires_grad_(True))


class _RMS(nn.Module):                              # InternRMSNorm, modeling_intern_vit.py:33-44
    def __init__(self, C):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(C))
        self.eps = 1e-6

    def forward(self, x):
        dt = x.dtype
        x = x.to(torch.float32)
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps)
        return self.weight * x.to(dt)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_gradient_reaches_the_qkv_linear(dtype):
    """InternAttention._flash_attn's statements (modeling_intern_vit.py:145-160) around the hook: Linear -> q / k RMSNorm ->
    torch.stack -> hook -> rearrange.  The Linear's weight gradient against the same graph with _naive_attn in fp64."""
    torch.manual_seed(3)
    Bn, S, Hn, D = 2, 193, 4, 64
    C = Hn * D
    lin, qn, kn = nn.Linear(C, 3 * C).to(DEV), _RMS(C).to(DEV), _RMS(C).to(DEV)
    with torch.no_grad():
        qn.weight.uniform_(0.5, 1.5)
        kn.weight.uniform_(0.5, 1.5)
    x = torch.randn(Bn, S, C, device=DEV)
    gy = torch.randn(Bn, S, C, device=DEV)
    mods = nn.ModuleList([lin, qn, kn])

    def graph(dt, attn):
        mods.to(dt)
        mods.zero_grad(set_to_none=True)
        qkv = lin(x.to(dt)).reshape(Bn, S, 3, Hn, D)
        q, k, v = qkv.unbind(2)
        q = qn(q.flatten(-2, -1)).view(q.shape)
        k = kn(k.flatten(-2, -1)).view(k.shape)
        ctx = attn(torch.stack([q, k, v], dim=2))
        ctx.reshape(Bn, S, C).backward(gy.to(dt))
        return lin.weight.grad.detach().double().clone(), qn.weight.grad.detach().double().clone()

    def naive(qkv):
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        return ati.naive_attn(q, k, v, D ** -0.5)
    # parameters rounded to the 16-bit type once, so that all three graphs start from the same numbers
    mods.to(dtype)
    w16 = [p.detach().clone() for p in mods.parameters()]

    def reset():
        with torch.no_grad():
            for p, w in zip(mods.parameters(), w16):
                p.copy_(w)
    mods.to(torch.float64); reset()
    ref_w, ref_n = graph(torch.float64, naive)
    mods.to(dtype); reset()
    t_w, t_n = graph(dtype, naive)
    reset()
    our_w, our_n = graph(dtype, lambda t: FlashAttention()(t)[0])
    assert float(our_w.abs().max()) > 0
    for what, ours, theirs, ref in (("qkv weight", our_w, t_w, ref_w), ("q_norm weight", our_n, t_n, ref_n)):
        a, b = ati.rel_rms(ours, ref), ati.rel_rms(theirs, ref)
        print(f"{what} {dtype}: rel rms {a:.3e} (torch 16-bit {b:.3e})")
        assert a <= 1.25 * b, f"{what}: rel rms {a:.3e} > 1.25 x torch's {b:.3e}"


def _odd_view(t, off=3):
    """The same values as a contiguous view at an odd storage offset."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def test_operand_placement_views_and_streams():
    """qkv and grad_out as views at odd storage offsets and as non-contiguous views; the call on a non-default stream (and on a
    non-current device if there is one): the same bits as the plain call."""
    dtype, S, D = torch.bfloat16, 129, 64
    qkv, dout = (t.to(DEV) for t in ati.case("random", B, S, H, D, dtype))
    out0, g0 = hook_grads(qkv, dout)
    # odd storage offsets
    out1, g1 = hook_grads(_odd_view(qkv), _odd_view(dout))
    assert torch.equal(out1, out0) and torch.equal(g1, g0)
    # non-contiguous: qkv as a permuted view, grad_out as the caller's rearrange gives it ('b s (h d)' consumer of 'b h s d' memory)
    x = qkv.permute(2, 0, 1, 3, 4).contiguous().permute(1, 2, 0, 3, 4).detach().requires_grad_(True)
    assert not x.is_contiguous()
    out2, _ = FlashAttention()(x)
    out2.backward(dout.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3))
    assert torch.equal(out2.detach(), out0) and torch.equal(x.grad, g0)
    # a side stream
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        out3, g3 = hook_grads(qkv, dout)
    s.synchronize()
    assert torch.equal(out3, out0) and torch.equal(g3, g0)
    if torch.cuda.device_count() > 1:
        other = "cuda:1"
        out4, g4 = hook_grads(qkv.to(other), dout.to(other))      # the current device stays 0
        assert out4.device == torch.device(other) and torch.equal(out4.to(DEV), out0) and torch.equal(g4.to(DEV), g0)


def test_refused_calls_write_nothing():
    dtype, S, D = torch.bfloat16, 65, 64
    qkv, dout = (t.to(DEV) for t in ati.case("random", 1, S, 2, D, dtype))
    scale = D ** -0.5
    out, lse = fwd_train(qkv, scale)
    nan = lambda g: bool(torch.isnan(g.float()).all())
    # workspace too small
    assert nan(bwd(qkv, out, lse, dout, scale, expect=-1, ws_bytes=15))
    # misaligned pointers
    assert nan(bwd(_odd_view(qkv), out, lse, dout, scale, expect=-1))
    assert nan(bwd(qkv, out, lse, _odd_view(dout), scale, expect=-1))
    g = _odd_view(torch.full(tuple(qkv.shape), float("nan"), dtype=dtype, device=DEV))
    assert nan(bwd(qkv, out, lse, dout, scale, expect=-1, grad=g))
    # D = 32
    q32 = torch.randn(1, S, 3, 2, 32, device=DEV).to(dtype)
    o32 = torch.full((1, S, 2, 32), float("nan"), dtype=dtype, device=DEV)
    g32 = torch.full((1, S, 3, 2, 32), float("nan"), dtype=dtype, device=DEV)
    L = _lib.lib()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    assert L.vllm_attn_bwd_qkvpacked_bf16(P(q32), P(o32), P(lse), P(o32), 1, S, 2, 32, scale, P(g32), P(ws), 1 << 16, stream()) == -1
    l32 = torch.full((1, 2, S), float("nan"), dtype=torch.float32, device=DEV)
    assert L.vllm_attn_fwd_train_qkvpacked_bf16(P(q32), P(o32), P(l32), 1, S, 2, 32, scale, stream()) == -1
    torch.cuda.synchronize()
    assert nan(g32) and nan(o32) and nan(l32)
