"""GPU: training through the visual-token splice (modeling_visionllmv2.py:582-605) -- the only statement through which the LLM loss
reaches the projector.  ``splice_visual_tokens`` under autograd (an in-place node, native backward
``vllm_splice_visual_tokens_backward_bf16``) against torch's own autograd of the reference's statements on the same tensors
(splice_train_inputs.reference_splice), never against the code under test.  Pure moves are compared bit for bit (``torch.equal``:
-0.0 == 0.0); the repeat rule's fp32 sums against fp64 autograd with a bound derived from the formats."""
import ctypes

import pytest
import torch

import splice_train_inputs as SI
from bounds import bf16_ulp, stream
from splice_train_inputs import IMP
from visionllm_amd import _lib
from visionllm_amd.splice import splice_status_ok, splice_visual_tokens

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def native_grads(c, need=(True, True), emb=None, feats=None, grad_out=None, **kw):
    """-> (spliced, d/d emb, d/d feats) through the public function; the embeddings it splices into are a non-leaf clone."""
    e = (c["emb"] if emb is None else emb).detach().clone().requires_grad_(need[0])
    f = (c["feats"] if feats is None else feats).detach().clone().requires_grad_(need[1])
    x = e.clone()
    out = splice_visual_tokens(x, c["ids"], IMP, f, c["split"], **kw)
    assert out is x and (out.grad_fn is not None) == any(need)
    if any(need):
        (out * 1).backward(c["grad_out"] if grad_out is None else grad_out)    # (frozen embeddings: the gradient arrives through a later op)
    return out.detach(), e.grad, f.grad


def capi_backward(c, want=(True, True), grad_out=None, expect=0):
    """Forward and backward through the C ABI; the outputs are pre-filled with NaN: every element must be written."""
    L_ = _lib.lib()
    B, L, T, C, n_tiles = c["B"], c["L"], c["T"], c["C"], c["n_tiles"]
    tps = None if c["split"] is None else (ctypes.c_int32 * B)(*c["split"])
    ws = torch.empty(int(L_.vllm_splice_workspace_ints(B, L, n_tiles)), dtype=torch.int32, device=DEV)
    x = c["emb"].clone()
    _lib.check(L_.vllm_splice_visual_tokens_bf16(_lib.ptr(c["ids"]), IMP, _lib.ptr(c["feats"]), tps, B, L, n_tiles, T, C, _lib.ptr(x),
                                                 _lib.ptr(ws), None, stream()))
    g = c["grad_out"] if grad_out is None else grad_out
    ge = torch.full((B, L, C), float("nan"), dtype=torch.bfloat16, device=DEV) if want[0] else None
    gf = torch.full((n_tiles, T, C), float("nan"), dtype=torch.bfloat16, device=DEV) if want[1] else None
    rc = L_.vllm_splice_visual_tokens_backward_bf16(_lib.ptr(ws), _lib.ptr(g), B, L, n_tiles, T, C, _lib.ptr(ge), _lib.ptr(gf), stream())
    assert rc == expect, (rc, L_.vllm_last_error().decode())
    torch.cuda.synchronize()
    return ge, gf, ws


def check_pure_move(c):
    out_r, ge_r, gf_r = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"])
    sel = (c["ids"] == IMP).reshape(-1)
    for what, run in (("autograd", lambda: native_grads(c)[1:]), ("C ABI", lambda: capi_backward(c)[:2])):
        ge, gf = run()
        assert ge is not None and gf is not None, f"{what}: a gradient is missing (embeddings {ge is not None}, features {gf is not None})"
        assert ge.shape == c["emb"].shape and gf.shape == c["feats"].shape and ge.dtype == gf.dtype == torch.bfloat16
        assert torch.equal(ge, ge_r), f"{what}: embedding gradient differs from torch's autograd of the reference"
        assert torch.equal(gf, gf_r), f"{what}: feature gradient differs from torch's autograd of the reference"
        assert int((ge.reshape(-1, c["C"])[sel] != 0).sum()) == 0, f"{what}: a slot row of the embedding gradient is not zero"
        assert torch.equal(ge.reshape(-1, c["C"])[~sel], c["grad_out"].reshape(-1, c["C"])[~sel])
        for t in c["dropped"]:
            assert int((gf[t] != 0).sum()) == 0, f"{what}: dropped tile {t} has a gradient"
    return out_r


# ---- 1: pure moves are exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["equal", "anyres_dropped", "one_tile_per_sample", "no_slot"])
@pytest.mark.parametrize("C", [64, 2056])      # 8 and 257 16-byte chunks a row: below a wave, and the unrolled mover with a tail
def test_pure_moves_are_exact(name, C):
    c = SI.case(name, C, DEV, seed=C + len(name))
    out_r = check_pure_move(c)
    assert torch.equal(native_grads(c)[0], out_r)        # (and the node's forward is the reference's forward)


def test_pure_moves_are_exact_at_the_benchmark_shape():
    check_pure_move(SI.case("bench", 4096, DEV, seed=4))


# ---- 2: the repeat rule: k terms added in fp32 in ascending slot order, rounded to bf16 once ---------------------------------------
@pytest.mark.parametrize("name", ["repeat2", "repeat3"])
@pytest.mark.parametrize("C", [64, 2056])
def test_repeat_rule_against_fp64(name, C):
    """Bound, per element: |err| <= 1 bf16 ulp of the fp64 value + 2^-20 sum|terms|.  The k <= 3 terms are bf16 values; adding them
    in fp32 makes k - 1 roundings of at most 2^-24 of a partial sum each, partial sums are at most sum|terms|, so the fp32 sum is
    within 2 * 2^-24 sum|terms| < 2^-20 sum|terms| of the exact one; rounding it to bf16 moves it by at most half an ulp at its own
    magnitude, which is at most one ulp at the exact value's.  Nothing in the bound is measured."""
    c = SI.case(name, C, DEV, seed=C)
    k = int(name[-1])
    assert int((c["ids"] == IMP).sum()) == k * c["n_tiles"] * c["T"]
    _, ge, gf = native_grads(c)
    _, ge64, gf64 = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"], torch.float64)
    _, _, mag = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"].abs(), torch.float64)   # sum |terms|
    assert gf is not None, "image_features.grad is None"
    err = (gf.double() - gf64).abs()
    bound = bf16_ulp(gf64) + 2.0 ** -20 * mag
    worst = (err / bound).max().item()
    print(f"{name} C={C}: worst |err| / bound = {worst:.3f}, max |err| = {err.max().item():.3g}")
    assert bool((err <= bound).all()), f"worst |err| / bound = {worst}"
    assert torch.equal(ge.double(), ge64)                     # the embedding gradient stays a pure move
    _, ge2, gf2 = native_grads(c)
    assert torch.equal(ge2.view(torch.int16), ge.view(torch.int16)) and torch.equal(gf2.view(torch.int16), gf.view(torch.int16))
    ge3, gf3, _ = capi_backward(c)
    assert torch.equal(ge3.view(torch.int16), ge.view(torch.int16)) and torch.equal(gf3.view(torch.int16), gf.view(torch.int16))


# ---- 3: a mismatch with check=False: nothing was written, so nothing flows to the features ------------------------------------------
def test_mismatch_without_check():
    c = SI.case("mismatch", 64, DEV)
    e = c["emb"].clone().requires_grad_(True)
    f = c["feats"].clone().requires_grad_(True)
    out, status = splice_visual_tokens(e.clone(), c["ids"], IMP, f, c["split"], check=False, return_status=True)
    assert status.grad_fn is None and not status.requires_grad and status.dtype == torch.int32
    assert [int(v) for v in status.cpu()][1:] == [6, 1, 13]
    with pytest.raises(RuntimeError, match="shape mismatch: 13 <im_patch> slots cannot take 6 visual tokens"):
        splice_status_ok(status)
    assert torch.equal(out.detach(), c["emb"])
    out.backward(c["grad_out"])
    assert torch.equal(e.grad, c["grad_out"])
    assert f.grad is not None and f.grad.shape == f.shape and int((f.grad != 0).sum()) == 0
    ge, gf, _ = capi_backward(c)
    assert torch.equal(ge, c["grad_out"]) and int((gf != 0).sum()) == 0
    with pytest.raises(RuntimeError, match="shape mismatch"):       # check=True raises as before, also under autograd
        splice_visual_tokens(e.clone(), c["ids"], IMP, f, c["split"])


# ---- 4: only one side needs a gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["equal", "anyres_dropped"])
@pytest.mark.parametrize("need", [(False, True), (True, False)])
def test_one_side_needs_a_gradient(name, need):
    c = SI.case(name, 64, DEV, seed=3)
    _, ge_r, gf_r = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"])
    _, ge, gf = native_grads(c, need=need)
    if need[0]:
        assert gf is None and torch.equal(ge, ge_r)
    else:
        assert ge is None and gf is not None and torch.equal(gf, gf_r)
    ge2, gf2, _ = capi_backward(c, want=need)                       # NULL for the other output
    assert torch.equal(ge2, ge_r) if need[0] else torch.equal(gf2, gf_r)


# ---- 5: operands at storage offsets that are not 16-byte aligned, the whole step on a caller stream --------------------------------
def offset_view(t, off, differentiable):
    """``t`` as a contiguous view ``off`` bytes into a larger NaN-filled buffer; differentiable: the buffer is a non-leaf made from
    ``t`` (torch.cat), so gradients flow back to it."""
    k = off // 2
    pad = torch.full((k,), float("nan"), dtype=t.dtype, device=t.device)
    tail = torch.full((32,), float("nan"), dtype=t.dtype, device=t.device)
    buf = torch.cat([pad, t.reshape(-1), tail]) if differentiable else torch.cat([pad, t.detach().reshape(-1), tail])
    v = buf[k:k + t.numel()].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == off % 16
    return v


@pytest.mark.parametrize("name", ["anyres_dropped", "repeat3"])
def test_offset_views_and_a_caller_stream(name):
    c = SI.case(name, 64, DEV, seed=5)
    _, ge0, gf0 = native_grads(c)                                    # aligned operands, default stream
    side = torch.cuda.Stream(device=DEV)
    for offs in [(2, 0, 0), (0, 6, 0), (0, 0, 10), (2, 4, 6), (14, 8, 12), (8, 8, 8)]:
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            e = c["emb"].clone().requires_grad_(True)
            f = c["feats"].clone().requires_grad_(True)
            x = offset_view(e, offs[0], True)
            assert offs[0] == 0 or x.data_ptr() % 16 != 0
            out = splice_visual_tokens(x, c["ids"], IMP, offset_view(f, offs[1], True), c["split"])
            assert out is x
            out.backward(offset_view(c["grad_out"], offs[2], False))
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(e.grad.view(torch.int16), ge0.view(torch.int16)), offs
        assert torch.equal(f.grad.view(torch.int16), gf0.view(torch.int16)), offs


# ---- 6: end to end with the projector's native backward -----------------------------------------------------------------------------
def test_end_to_end_with_the_projector():
    from visionllm_amd.bridge import build_vl_bridge
    c = SI.case("equal", 256, DEV, seed=6)
    torch.manual_seed(0)
    br = build_vl_bridge("mlp2x_gelu", 128, 256).to(DEV).to(torch.bfloat16)
    x = torch.randn(c["n_tiles"], c["T"], 128, device=DEV).to(torch.bfloat16)
    w = torch.randn(c["B"], c["L"], 256, device=DEV).to(torch.bfloat16)
    table = c["emb"].clone().requires_grad_(True)                   # stands for the LLM's embedding output

    def step(splice):
        table.grad = None
        for p in br.parameters():
            p.grad = None
        out = splice(table.clone(), br(x))
        (out.float() * w.float()).sum().backward()
        return {n: p.grad.clone() for n, p in br.named_parameters()}, table.grad.clone(), out.detach()
    g_ref, t_ref, o_ref = step(lambda e, f: SI.reference_splice(e, c["ids"], f, c["split"]))
    g_nat, t_nat, o_nat = step(lambda e, f: splice_visual_tokens(e, c["ids"], IMP, f, c["split"]))
    assert torch.equal(o_nat, o_ref) and torch.equal(t_nat, t_ref)
    assert set(g_nat) == set(g_ref) and len(g_nat) == 4
    for n in g_ref:
        assert float(g_ref[n].float().abs().max()) > 0
        assert torch.equal(g_nat[n], g_ref[n]), f"grad of {n} differs"


# ---- 7: errors and the paths that build no node -------------------------------------------------------------------------------------
def test_leaf_embeddings_raise_torchs_in_place_error():
    c = SI.case("equal", 64, DEV)
    with pytest.raises(RuntimeError, match="leaf Variable that requires grad .* in-place operation"):
        splice_visual_tokens(c["emb"].clone().requires_grad_(True), c["ids"], IMP, c["feats"], c["split"])
    with pytest.raises(RuntimeError, match="leaf Variable that requires grad .* in-place operation"):      # the reference's statement
        SI.reference_splice(c["emb"].clone().requires_grad_(True), c["ids"], c["feats"], c["split"])


def test_no_node_without_grad():
    c = SI.case("anyres_dropped", 64, DEV)
    want = splice_visual_tokens(c["emb"].clone(), c["ids"], IMP, c["feats"], c["split"])
    assert want.grad_fn is None and not want.requires_grad
    e = c["emb"].clone().requires_grad_(True)
    f = c["feats"].clone().requires_grad_(True)
    with torch.no_grad():
        x = e.clone()
        out = splice_visual_tokens(x, c["ids"], IMP, f, c["split"])
    assert out is x and out.grad_fn is None and not out.requires_grad and torch.equal(out, want)
    with torch.inference_mode():
        x = e.clone()
        out, status = splice_visual_tokens(x, c["ids"], IMP, f, c["split"], return_status=True)
        assert out is x and torch.equal(out, want) and splice_status_ok(status)
    ref = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"])[0]
    assert torch.equal(want, ref)


def test_second_backward_through_a_retained_graph():
    c = SI.case("repeat2", 64, DEV)
    e = c["emb"].clone().requires_grad_(True)
    f = c["feats"].clone().requires_grad_(True)
    out = splice_visual_tokens(e.clone(), c["ids"], IMP, f, c["split"])
    out.backward(c["grad_out"], retain_graph=True)
    ge, gf = e.grad.clone(), f.grad.clone()
    e.grad = f.grad = None
    out.backward(c["grad_out"])
    assert torch.equal(e.grad.view(torch.int16), ge.view(torch.int16)) and torch.equal(f.grad.view(torch.int16), gf.view(torch.int16))


def test_float_features_get_a_float_gradient():
    """The conversion to bf16 stays outside the node: torch differentiates it, and the gradient has image_features' dtype and shape."""
    c = SI.case("equal", 64, DEV)
    f32 = c["feats"].float().requires_grad_(True)
    out = splice_visual_tokens(c["emb"].clone(), c["ids"], IMP, f32, c["split"])
    (out * 1).backward(c["grad_out"])
    gf_r = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"])[2]
    assert f32.grad.dtype == torch.float32 and torch.equal(f32.grad, gf_r.float())


def test_non_finite_grad_out_at_a_slot_row_gives_zero():
    """Deliberate departure (include/vllm_hip.h): the reference's ``* 0.0`` turns inf / NaN arriving at an overwritten row into NaN in
    the embedding gradient; the native backward writes the derivative of an overwritten row, 0.  The feature gradient is a move
    either way."""
    c = SI.case("equal", 64, DEV)
    sel = (c["ids"] == IMP).reshape(-1)
    slots = torch.nonzero(sel).reshape(-1)
    g = c["grad_out"].clone()
    g.view(-1, 64)[slots[0], 3] = float("inf")
    g.view(-1, 64)[slots[5], 0] = float("nan")
    _, ge_r, gf_r = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], g)
    assert bool(torch.isnan(ge_r.view(-1, 64)[slots[0], 3])) and bool(torch.isnan(ge_r.view(-1, 64)[slots[5], 0]))   # the reference
    _, ge, gf = native_grads(c, grad_out=g)
    assert int((ge.view(-1, 64)[sel] != 0).sum()) == 0 and torch.equal(ge.view(-1, 64)[~sel], g.view(-1, 64)[~sel])
    assert torch.equal(gf.nan_to_num(nan=7.0, posinf=9.0), gf_r.nan_to_num(nan=7.0, posinf=9.0))
    assert int(torch.isnan(gf).sum()) == 1 and int(torch.isinf(gf).sum()) == 1


# ---- 8: the C ABI directly ----------------------------------------------------------------------------------------------------------
def test_capi_refuses_a_misaligned_grad_out_and_accepts_no_outputs():
    c = SI.case("equal", 64, DEV)
    g = offset_view(c["grad_out"], 8, False)
    ge, gf, ws = capi_backward(c, grad_out=g, expect=-1)
    assert "16-byte aligned" in _lib.lib().vllm_last_error().decode()
    assert bool(torch.isnan(ge).all()) and bool(torch.isnan(gf).all())          # nothing was written
    L_ = _lib.lib()
    args = (c["B"], c["L"], c["n_tiles"], c["T"], c["C"])
    assert L_.vllm_splice_visual_tokens_backward_bf16(_lib.ptr(ws), _lib.ptr(c["grad_out"]), *args, None, None, stream()) == 0
    odd = offset_view(ge, 4, False)
    assert L_.vllm_splice_visual_tokens_backward_bf16(_lib.ptr(ws), _lib.ptr(c["grad_out"]), *args, _lib.ptr(odd), _lib.ptr(gf), stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(gf).all())
