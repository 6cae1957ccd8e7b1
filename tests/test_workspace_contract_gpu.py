"""GPU: the caller-workspace contract of every workspace-taking entry of the C ABI.

The size queries' answers are pinned by test_workspace_sizes_cpu.py; this file pins what they are FOR: a call given exactly that many
bytes, aligned as include/vllm_hip.h says and no better, stays inside them and does not care what was in them.  In the product the
workspace is always dirty (``_lib.workspace`` is one grow-only buffer per stream that every orchestrator takes in turn); every other
test hands a fresh ``torch.empty``.

Every case makes three runs (``three_runs``):
  (a) baseline  a roomy, allocator-aligned, zero-filled workspace;
  (b) hostile   exactly the query's bytes, filled with 0xFF (NaN in every floating type, non-zero flags, -1 ints), the pointer 16-byte
                aligned and not 32 (8 and not 16 for the point-sample backward, 4 and not 8 for the splice), guard bytes on both sides;
  (c) hostile   exactly the query's bytes, filled with 0x3F (finite, plausible values), allocator-aligned, guarded.
Outputs of (b) and (c) must be the baseline's BITS (these entries document run-to-run identical results, so no tolerance is involved),
no guard byte may change, and -- two identically wrong runs must not pass -- the baseline goes through the bound its entry already
has against its fp64 / oracle reference, with the existing helpers and bounds unchanged.

How the workspace reaches the C call.  The primitives (GEMM with stream-K scratch, weight-gradient GEMM, the three row-wise backwards,
attention backward, point-sample backward, DCNv3 half backward, the splice, the embeddings) are called straight through ctypes.  The
orchestrators whose descriptors the Python mirrors pack (vllm_vit_forward, vllm_bridge_forward, the projector's and the encoder layer's
training calls, vllm_msda_layer_forward) run through those mirrors with ``_lib.sized_workspace`` replaced: a mirror makes one C call
per workspace request and passes the tensor's pointer and the query's byte count through untouched, so the request IS the C call's
workspace.  Every request gets a fresh buffer with the run's own fill, so a training step's backward starts from 0xFF in run (b) -- the
"refilled with 0xFF between forward and backward" of a shared workspace -- and from 0x3F in run (c), never from what the forward left.

The stream-K flags.  A hostile fill makes every flag non-zero, and the only protection is the one reset per orchestrated call.  That
reset is pinned only where the tail is TAKEN, so the cases below read ``vllm_gemm_sk_launches()`` and assert it: taken in
vllm_gemm_bf16_sk, vllm_vit_forward (the folded-norm cases), vllm_bridge_forward (1024 x 4096 x 1024), vllm_bridge_forward_train / vllm_bridge_backward (1024 -> 4096, 1024 rows)
and vllm_vit_layer_forward_train / vllm_vit_layer_backward (hidden 1024, 1154 rows); asserted NOT taken in the hidden-128 / 128 -> 256
cases of 1024 rows, where the scratch is carved but K / 64 iterations of the few tiles cannot feed every compute unit -- those cases pin
sizes, guards and content of the other pieces, not the reset.  vllm_vit_embed_forward's GEMM (K = 640, at most 1285 x 256 outputs
here) never plans the tail: its reset is not pinned by this file.

One output is outside bit identity: grad_input of vllm_dcnv3_backward_f16 is summed with fp32 atomics in arrival order (the header says
so; test_half_precision_forward_and_backward compares it with a tolerance for the same reason) -- it gets that test's bound in every run
and the NaN check; grad_offset / grad_mask are compared bit for bit."""
import ast
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import attn_train_inputs as ati
import embed_train_inputs as E
import region_train_inputs as RT
import splice_train_inputs as SI
import vit_layer_train_inputs as VI
import workspace_guard as WG
from bounds import P, assert_bound, bf16_ulp, stream
from conftest import golden_sd, load_golden
from visionllm_amd import _lib

os.environ.setdefault("VLLM_GEMM_SK_FIX", "0")   # as test_vit_gpu.py: the stream-K tail wherever it is possible (the default charges its fix-up)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
bf = lambda t: t.to(torch.bfloat16)  # noqa: E731


# ---- the three runs ------------------------------------------------------------------------------------------------------------------------
class Workspaces:
    """Hands out the workspaces of one run.  ``fill`` None: the baseline's (zeros, a MiB to spare, the allocator's alignment); otherwise
    ``workspace_guard.guarded`` buffers of exactly the bytes asked for.  ``take(nbytes)`` -> (uint8 tensor whose data_ptr is the workspace
    pointer -- None where none is needed --, nbytes) for a direct C call; called as ``_lib.sized_workspace`` it serves a Python mirror."""

    def __init__(self, fill, skew, widest_row_bytes=0):
        self.fill, self.skew, self.widest = fill, skew, widest_row_bytes
        self.sizes, self.checks, self.views = [], [], []

    def take(self, nbytes, null_if_zero=True):
        nbytes = int(nbytes)
        self.sizes.append(nbytes)
        if nbytes == 0 and null_if_zero:
            return None, 0
        if self.fill is None:
            t = torch.zeros(nbytes + WG.MIB, dtype=torch.uint8, device=DEV)
            self.views.append(t)
            return t, nbytes
        _, _, check = WG.guarded(nbytes, self.fill, self.skew, self.widest, device=DEV)
        self.checks.append(check)
        self.views.append(check.workspace)
        assert nbytes == 0 or check.workspace.data_ptr() % 256 == self.skew % 256
        return check.workspace, nbytes

    def __call__(self, device, nbytes, what, slot=0):      # _lib.sized_workspace
        _lib.check(0 if nbytes >= 0 else -1, what)
        return self.take(nbytes, null_if_zero=False)

    def dirty(self):
        """what the next user of a shared workspace leaves behind: every workspace handed out so far is overwritten with 0xFF (a hostile run's;
        the baseline's stay as the calls left them)"""
        if self.fill is not None:
            for v in self.views:
                v.fill_(WG.HOSTILE)

    def finish(self):
        torch.cuda.synchronize()
        for c in self.checks:
            c()


RUNS = (("baseline", None, 0), ("0xFF skewed", WG.HOSTILE, None), ("0x3F aligned", WG.PLAUSIBLE, 0))


def same_bits(got, base, tag):
    assert set(got) == set(base), (tag, set(got) ^ set(base))
    for k, b in base.items():
        g = got[k]
        if b is None:
            assert g is None, (tag, k)
            continue
        assert g.dtype == b.dtype and g.shape == b.shape, (tag, k)
        if g.is_floating_point():
            extra = torch.isnan(g) & ~torch.isnan(b)
            assert not bool(extra.any()), f"{tag}: {k} holds {int(extra.sum())} NaN the baseline does not"
        gb, bb = g.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
        if not torch.equal(gb, bb):
            diff = (gb != bb).nonzero()
            raise AssertionError(f"{tag}: {k} differs from the baseline in {diff.shape[0]} bytes, first at byte {diff[0].tolist()}")


def three_runs(run, skew=16, widest_row_bytes=0, patch=None, exempt=()):
    """run(W: Workspaces) -> {name: tensor or None}.  -> the baseline's outputs (for the caller's bound) and the three Workspaces."""
    outs, spaces = [], []
    for tag, fill, sk in RUNS:
        W = Workspaces(fill, skew if sk is None else sk, widest_row_bytes)
        if patch is not None:
            patch.setattr(_lib, "sized_workspace", W)
        out = run(W)
        W.finish()
        outs.append(out)
        spaces.append(W)
    if patch is not None:
        patch.undo()
    assert spaces[0].sizes, "the case never asked for a workspace"
    for (tag, _, _), out, W in zip(RUNS[1:], outs[1:], spaces[1:]):
        assert W.sizes == spaces[0].sizes, (tag, W.sizes, spaces[0].sizes)
        same_bits({k: v for k, v in out.items() if k not in exempt}, {k: v for k, v in outs[0].items() if k not in exempt}, tag)
    return outs, spaces


def nan_bf16(*shape):
    return torch.full(shape, NAN, device=DEV).to(torch.bfloat16)


def test_the_guard_notices_one_stray_byte_on_either_side():
    """the helper itself: a byte written one past the workspace's end, or one in front of its start, fails ``check()`` and is located"""
    for where in ("behind", "front"):
        _, n, check = WG.guarded(1000, WG.HOSTILE, skew=16, device=DEV)
        check()
        buf = check.buffer
        assert buf.numel() == WG.FRONT + 16 + 1000 + WG.MIB and int(check.workspace[0]) == WG.HOSTILE and int(buf[WG.FRONT + 15]) == WG.GUARD
        at = WG.FRONT + 16 + 1000 + 7 if where == "behind" else WG.FRONT + 16 - 3
        buf[at] = 0
        with pytest.raises(AssertionError, match="byte 7 behind" if where == "behind" else "byte 3 in front"):
            check()
    check.workspace.fill_(0)      # writes inside the workspace are the callee's business
    buf[at] = WG.GUARD
    check()


# ---- vllm_gemm_bf16_sk ---------------------------------------------------------------------------------------------------------------------
SK_FLAGS, SK_SLOT = 4096, 262144      # include/vllm_hip.h: "resets its first 4096 bytes (flags)"; one fp32 partial tile of 256 x 256


@pytest.mark.parametrize("epi", [0, 3])
@pytest.mark.parametrize("cut", [False, True], ids=["full", "cut_to_256_slots"])
def test_gemm_stream_k_scratch(epi, cut):
    """4096 x 1024 x 1024, automatic schedule: 64 tiles on 256 CUs, every tile shared by four blocks through the scratch.  With the scratch
    cut to the slots of exactly 256 CUs the tail is either planned and stays inside, or not planned: both are legal, overrunning is not."""
    L = _lib.lib()
    M, N, K = 4096, 1024, 1024
    torch.manual_seed(M + N + K + epi)
    x, w, b = bf(torch.randn(M, K, device=DEV)), bf(torch.randn(N, K, device=DEV) / math.sqrt(K)), bf(torch.randn(N, device=DEV))
    ls, res = bf(0.1 + 0.05 * torch.randn(N, device=DEV)), bf(torch.randn(M, N, device=DEV))
    nbytes = SK_FLAGS + 256 * SK_SLOT if cut else L.vllm_gemm_scratch_bytes()
    assert nbytes <= L.vllm_gemm_scratch_bytes()
    took = []

    def run(W):
        ws, n = W.take(nbytes)
        y = nan_bf16(M, N)
        before = L.vllm_gemm_sk_launches()
        _lib.check(L.vllm_gemm_bf16_sk(P(x), P(w), P(b), P(y), M, N, K, K, K, N, epi, P(ls) if epi == 3 else None, P(res) if epi == 3 else None, N, 0,
                                       P(ws), n, stream()), "vllm_gemm_bf16_sk")
        took.append(L.vllm_gemm_sk_launches() - before)
        torch.cuda.synchronize()
        assert bool((ws[:SK_FLAGS] == 0).all()), "flags must be left zero"
        return dict(y=y)

    outs, _ = three_runs(run, widest_row_bytes=SK_SLOT // 256)
    print(f"stream-K launches per run: {took}")
    assert len(set(took)) == 1, took
    if not cut:
        assert took[0] == 1, "the stream-K tail was expected to be taken"
    z = x.double() @ w.double().t() + b.double()
    mag = x.double().abs() @ w.double().abs().t() + b.double().abs()
    if epi == 3:
        z, mag = res.double() + z * ls.double(), res.double().abs() + mag * ls.double().abs()
    assert_bound(outs[0]["y"], z, mag, f"gemm stream-K epi {epi} cut {cut}")


# ---- vllm_gemm_wgrad_bf16 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,split", [(4096, 1024, 256, True), (2304, 512, 512, True), (2300, 512, 512, True), (77, 64, 640, False)])
def test_wgrad_partials(M, N, K, split):
    L = _lib.lib()
    torch.manual_seed(M + N + K)
    dy, a = bf(torch.randn(M, N, device=DEV)), bf(torch.randn(M, K, device=DEV))
    need = L.vllm_gemm_wgrad_workspace_bytes(M, N, K)
    assert (need > 0) == split
    routes = []

    def run(W):
        ws, n = W.take(need)               # (77, 64, 640): the query answers 0 and NULL / 0 is accepted
        dw, db = nan_bf16(N, K), nan_bf16(N)
        before = L.vllm_gemm_wgrad_split_launches()
        _lib.check(L.vllm_gemm_wgrad_bf16(P(dy), N, P(a), K, M, N, K, P(dw), K, P(db), P(ws), n, stream()), "vllm_gemm_wgrad_bf16")
        routes.append(L.vllm_gemm_wgrad_split_launches() - before)
        return dict(dw=dw, db=db)

    outs, _ = three_runs(run, widest_row_bytes=K * 4)
    assert routes == [1 if split else 0] * 3, routes
    assert_bound(outs[0]["dw"], dy.double().T @ a.double(), dy.double().abs().T @ a.double().abs(), f"wgrad {M}x{N}x{K}")
    assert_bound(outs[0]["db"], dy.double().sum(0), dy.double().abs().sum(0), f"db {M}x{N}")


# ---- the three row-wise backwards ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", VI.NORM_SHAPES)
@pytest.mark.parametrize("G", [1, 2])
def test_rmsnorm_backward_partials(rows, C, G):
    """(rows 300 / 77 / 64 / 33: none but 64 is a multiple of the 2 or 4 rows a block works on at a time)"""
    L = _lib.lib()
    need = L.vllm_rmsnorm_backward_workspace_bytes(rows, C, G)
    assert need > 0
    if G == 1:
        x, gy, gres, w = VI.norm_case(rows, C, device=DEV)

        def run(W):
            ws, n = W.take(need)
            gx, gw = nan_bf16(rows, C), nan_bf16(C)
            _lib.check(L.vllm_rmsnorm_backward_bf16(P(x), C, P(gy), C, P(w), None, 1, VI.EPS, rows, C, P(gx), C, P(gres), C, P(gw), None, P(ws), n,
                                                    stream()), "vllm_rmsnorm_backward_bf16")
            return dict(gx=gx, gw=gw)

        base = three_runs(run, widest_row_bytes=C * 4)[0][0]
        rx, rw, mx, mw = VI.rms_bwd_ref(x, gy, w, gres)
        assert VI.excess_ulp(base["gx"], rx, mx) <= 1.0 and VI.excess_ulp(base["gw"], rw, mw) <= 1.0
        return
    xq, gq, _, wq = VI.norm_case(rows, C, seed=1, device=DEV)
    xk, gk, xv, wk = VI.norm_case(rows, C, seed=2, device=DEV)
    _, gv, _, _ = VI.norm_case(rows, C, seed=3, device=DEV)
    qkv, g0 = torch.cat([xq, xk, xv], 1).contiguous(), torch.cat([gq, gk, gv], 1).contiguous()

    def run2(W):
        ws, n = W.take(need)
        g, gwq, gwk = g0.clone(), nan_bf16(C), nan_bf16(C)
        _lib.check(L.vllm_rmsnorm_backward_bf16(P(qkv), 3 * C, P(g), 3 * C, P(wq), P(wk), 2, VI.EPS, rows, C, P(g), 3 * C, None, 0, P(gwq), P(gwk),
                                                P(ws), n, stream()), "vllm_rmsnorm_backward_bf16 G=2")
        return dict(g=g, gwq=gwq, gwk=gwk)

    base = three_runs(run2, widest_row_bytes=C * 4)[0][0]
    assert torch.equal(base["g"][:, 2 * C:], g0[:, 2 * C:]), "the v block changed"
    for x_, g_, w_, out, gw in ((xq, gq, wq, base["g"][:, :C], base["gwq"]), (xk, gk, wk, base["g"][:, C:2 * C], base["gwk"])):
        rx, rw, mx, mw = VI.rms_bwd_ref(x_, g_, w_)
        assert VI.excess_ulp(out, rx, mx) <= 1.0 and VI.excess_ulp(gw, rw, mw) <= 1.0


@pytest.mark.parametrize("rows,C", VI.NORM_SHAPES)
def test_layerscale_backward_partials(rows, C):
    L = _lib.lib()
    go, y, _, w = VI.norm_case(rows, C, seed=1, device=DEV)
    ls = bf(0.1 * w.float())
    need = L.vllm_layerscale_backward_workspace_bytes(rows, C)
    assert need > 0

    def run(W):
        ws, n = W.take(need)
        gy, gls = nan_bf16(rows, C), nan_bf16(C)
        _lib.check(L.vllm_layerscale_backward_bf16(P(go), C, P(y), C, P(ls), rows, C, P(gy), C, P(gls), P(ws), n, stream()),
                   "vllm_layerscale_backward_bf16")
        return dict(gy=gy, gls=gls)

    base = three_runs(run, widest_row_bytes=C * 4)[0][0]
    ry, rls, mls = VI.ls_bwd_ref(go, y, ls)
    assert VI.excess_ulp(base["gy"], ry, torch.zeros_like(ry)) <= 1.0 and VI.excess_ulp(base["gls"], rls, mls) <= 1.0


@pytest.mark.parametrize("rows,C", [(300, 128), (64, 12800)])
def test_layernorm_backward_partials(rows, C):
    """reference and bounds: test_bridge_train_gpu.py::test_layernorm_backward_against_fp64"""
    L = _lib.lib()
    torch.manual_seed(rows + C)
    x = bf(torch.randn(rows, C, device=DEV) * 2 + 0.5)
    gam, bet = bf(1 + 0.1 * torch.randn(C, device=DEV)), bf(0.1 * torch.randn(C, device=DEV))
    gy = torch.randn(rows, C, device=DEV)
    eps = 1e-5
    need = L.vllm_layernorm_backward_workspace_bytes(rows, C)
    assert need > 0

    def run(W):
        ws, n = W.take(need)
        gx, gw, gb = nan_bf16(rows, C), nan_bf16(C), nan_bf16(C)
        _lib.check(L.vllm_layernorm_backward_bf16(P(x), C, P(gy), C, P(gam), eps, rows, C, P(gx), C, P(gw), P(gb), P(ws), n, stream()),
                   "vllm_layernorm_backward_bf16")
        return dict(gx=gx, gw=gw, gb=gb)

    base = three_runs(run, widest_row_bytes=2 * C * 4)[0][0]
    xd = x.double().requires_grad_(True)
    gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (C,), gd, bd, eps).backward(gy.double())
    mean = x.double().mean(1, keepdim=True)
    r = 1.0 / torch.sqrt(((x.double() - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x.double() - mean) * r
    assert_bound(base["gw"], gd.grad, (gy.double() * xh).abs().sum(0), "LayerNorm grad_w")
    assert_bound(base["gb"], bd.grad, gy.double().abs().sum(0), "LayerNorm grad_b")
    g = gy.double() * gam.double()
    mag = r * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)) * 4
    assert_bound(base["gx"], xd.grad, mag, "LayerNorm grad_x")


# ---- vllm_attn_bwd_qkvpacked_* -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [65, 193])
def test_attn_backward_delta(S, D, dtype):
    """partial last query tiles; delta [B, H, S] lives in the workspace between the two kernels"""
    import test_attn_train_gpu as TA
    B, H = 2, 2
    qkv, dout = (t.to(DEV) for t in ati.case("random", B, S, H, D, dtype))
    scale = D ** -0.5
    out, lse = TA.fwd_train(qkv, scale)
    need = _lib.lib().vllm_attn_bwd_workspace_bytes(B, S, H, D)
    assert need >= B * H * S * 4

    def run(W):
        ws, n = W.take(need)
        return dict(g=TA.bwd(qkv, out, lse, dout, scale, ws=ws, ws_bytes=n))

    base = three_runs(run, widest_row_bytes=S * 4)[0][0]
    ref, bound, _ = ati.grad_bounds(qkv, dout, scale, dtype)
    worst, at = ati.worst_factor(base["g"], ref, bound)
    print(f"attn_bwd S{S} D{D} {dtype}: {worst:.3f} of the per-element bound")
    assert worst <= 1.0, (worst, at)


# ---- vllm_point_sample_mean_backward_{f32,bf16} --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W_,Pn", [(2, 9, 80, 80, 500), (4, 256, 24, 24, 2304)])
def test_point_sample_mean_backward_accumulators(N, C, H, W_, Pn):
    """80 x 80: A and the counts in the workspace (8-byte alignment is what the header promises: skew 8); 24 x 24: the query answers 0 and
    NULL / 0 is accepted.  The last region of a case has no valid point (region_train_inputs.make_case)."""
    L = _lib.lib()
    c, v, g = RT.make_case(N, C, H, W_, Pn, N * 1000 + C + H + Pn)
    assert not bool(v[N - 1].any())
    cd, vd, gd = c.to(DEV), v.to(torch.uint8).to(DEV), g.to(DEV)
    need = L.vllm_point_sample_backward_workspace_bytes(N, C, H, W_, Pn)
    assert (need > 0) == (H == 80)

    def run(W):
        out = {}
        for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            ws, n = W.take(need)
            gi = torch.full((N, C, H, W_), NAN, device=DEV, dtype=dt)
            fn = getattr(L, f"vllm_point_sample_mean_backward_{name}")
            _lib.check(fn(P(cd), P(vd), P(gd), N, C, H, W_, Pn, P(gi), P(ws), n, stream()), f"vllm_point_sample_mean_backward_{name}")
            out[name] = gi
        return out

    base = three_runs(run, skew=8, widest_row_bytes=H * W_ * 8)[0][0]
    ref = RT.mean_reference(c, v, g, C, H, W_)
    out = base["f32"].cpu()
    live = v.sum(1) > 0
    assert torch.equal(out[~live], torch.zeros_like(out[~live]))
    err, bound = (out.double() - ref)[live].abs(), RT.mean_bound(ref, c, v, g, H, W_)[live]
    assert bool((err <= bound).all()), f"worst err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}"
    assert torch.equal(base["bf16"], base["f32"].to(torch.bfloat16))


# ---- vllm_dcnv3_backward_f16 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c16", "c5"])
def test_dcnv3_half_backward_widened_copies(tag):
    L = _lib.lib()
    g = load_golden("dcnv3_half.npz")
    kh, kw, sh, sw, ph, pw, dh, dw, G, Cg = [int(v) for v in g[f"{tag}.params"]]
    scale = float(g[f"{tag}.offset_scale"])
    h = lambda k: torch.from_numpy(g[f"{tag}.{k}"]).to(DEV)  # noqa: E731
    inp, off, msk, go = h("input"), h("offset"), h("mask"), h("grad_out")
    N, H, W_, _ = inp.shape
    geo = (N, H, W_, G, Cg, kh, kw, sh, sw, ph, pw, dh, dw)
    need = L.vllm_dcnv3_backward_f16_workspace(*geo)
    assert need > 0

    def run(W):
        ws, n = W.take(need)
        gi, gof, gm = (torch.full(t.shape, NAN, device=DEV, dtype=torch.float16) for t in (inp, off, msk))
        _lib.check(L.vllm_dcnv3_backward_f16(P(inp), P(off), P(msk), P(go), *geo, scale, P(gi), P(gof), P(gm), P(ws), n, stream()),
                   "vllm_dcnv3_backward_f16")
        return dict(grad_input=gi, grad_offset=gof, grad_mask=gm)

    outs, _ = three_runs(run, widest_row_bytes=W_ * G * Cg * 4, exempt=("grad_input",))     # (module docstring: fp32 atomics)
    for out in outs:
        for key, ours in out.items():
            ref = g[f"{tag}.{key}"].astype(np.float32)
            assert not bool(torch.isnan(ours).any()), key
            np.testing.assert_allclose(ours.float().cpu().numpy(), ref, rtol=2e-3, atol=2e-3 * max(np.abs(ref).max(), 1e-3), err_msg=key)


# ---- the splice: its forward leaves the slot list in the workspace, its backward reads it ---------------------------------------------------
@pytest.mark.parametrize("name", ["anyres_dropped", "repeat3", "no_slot"])
def test_splice_workspace(name):
    L_ = _lib.lib()
    c = SI.case(name, 64, DEV, seed=64 + len(name))
    B, L, T, C, n_tiles = c["B"], c["L"], c["T"], c["C"], c["n_tiles"]
    tps = (ctypes.c_int32 * B)(*c["split"])
    words = L_.vllm_splice_workspace_ints(B, L, n_tiles)

    def run(W):
        ws, n = W.take(4 * words)
        assert ws.data_ptr() % 4 == 0
        x, status = c["emb"].clone(), torch.full((4,), -7, dtype=torch.int32, device=DEV)
        _lib.check(L_.vllm_splice_visual_tokens_bf16(P(c["ids"]), SI.IMP, P(c["feats"]), tps, B, L, n_tiles, T, C, P(x), P(ws), P(status), stream()))
        ge, gf = nan_bf16(B, L, C), nan_bf16(n_tiles, T, C)
        _lib.check(L_.vllm_splice_visual_tokens_backward_bf16(P(ws), P(c["grad_out"]), B, L, n_tiles, T, C, P(ge), P(gf), stream()))
        torch.cuda.synchronize()
        return dict(x=x, status=status, header=ws[:16].clone(), ge=ge, gf=gf)

    base = three_runs(run, skew=4, widest_row_bytes=L * 4)[0][0]       # (int32 words: 4-byte alignment is all the header asks)
    n_slots = int((c["ids"] == SI.IMP).sum())
    assert [int(v) for v in base["status"].cpu()][:3] == [n_slots, (n_tiles - len(c["dropped"])) * T, 0]
    assert int(base["header"].view(torch.int32)[3]) == n_slots
    if name == "repeat3":      # test_splice_train_gpu.py::test_repeat_rule_against_fp64
        _, ge64, gf64 = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"], torch.float64)
        _, _, mag = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"].abs(), torch.float64)
        assert bool(((base["gf"].double() - gf64).abs() <= bf16_ulp(gf64) + 2.0 ** -20 * mag).all())
        assert torch.equal(base["ge"].double(), ge64)
    else:                      # pure moves are exact
        out_r, ge_r, gf_r = SI.reference_grads(c["emb"], c["ids"], c["feats"], c["split"], c["grad_out"])
        assert torch.equal(base["x"], out_r) and torch.equal(base["ge"], ge_r) and torch.equal(base["gf"], gf_r)


# ---- vllm_vit_embed_forward / vllm_vit_embed_backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, E.SPLIT_CASE])
def test_embed_train_workspace(idx):
    import test_embed_train_gpu as TE
    L = _lib.lib()
    n, image, patch, C, bias, pdt = E.CASES[idx]
    c = E.make_case(*E.CASES[idx], seed=idx, device=DEV)
    d = TE.desc_of(c, image, patch)
    need = L.vllm_vit_embed_workspace_bytes(ctypes.byref(d), n)
    S = (image // patch) ** 2 + 1
    if idx == E.SPLIT_CASE:
        assert L.vllm_gemm_wgrad_workspace_bytes(n * S, C, E.kpad_for(patch)) > 0
    routes = []

    def run(W):
        ws, nb = W.take(need)
        out = nan_bf16(n, S, C)
        _lib.check(L.vllm_vit_embed_forward(ctypes.byref(d), P(c["pix"]), n, P(out), P(ws), nb, stream()), "vllm_vit_embed_forward")
        W.dirty()
        before = L.vllm_gemm_wgrad_split_launches()
        rc, bufs = TE.c_backward(c, image, patch, d=d, ws=(ws, nb))
        routes.append(L.vllm_gemm_wgrad_split_launches() - before)
        assert rc == 0, L.vllm_last_error()
        for name in TE.NAMES:
            assert c[name] is None or TE.untouched(bufs, name), name
        return dict(out=out, **{k: bufs[k][1] for k in TE.NAMES})

    base = three_runs(run, widest_row_bytes=E.kpad_for(patch) * 4)[0][0]
    assert routes == [1 if idx == E.SPLIT_CASE else 0] * 3, routes
    ref, mag = E.reference(c, patch)
    for name in TE.NAMES:
        assert E.excess_ulp(base[name].cpu(), ref[name], mag[name]) <= 1.0, name
    fwd = E.embeddings(*(c[k].cpu().double() for k in ("pix", "w", "b", "cls", "pos")), patch)
    assert VI.rel_rms(base["out"].cpu(), fwd) < 2.0 ** -8


# ---- vllm_vit_layer_forward_train / vllm_vit_layer_backward --------------------------------------------------------------------------------
LAYER_CASES = [VI.LAYER_CONFIGS[0], VI.LAYER_CONFIGS[1], (128, 2, 256, 4, 256, True, False),     # tiny with / without QK-norm; B S = 1024: scratch carved
               VI.LAYER_CONFIGS[2]]                                                               # hidden 1024, 1154 rows: the stream-K tail is taken
FROZEN = {"all": None,
          "scales_and_norms": {"ls1", "ls2", "norm1.weight", "norm2.weight", "attn.q_norm.weight", "attn.k_norm.weight"},     # test_frozen_subsets
          "fc2_bias_alone": {"mlp.fc2.bias"}}
LAYER_RUNS = [(0, "all"), (1, "all"), (2, "all"), (3, "all")] + [(i, f) for i in (0, 1) for f in ("scales_and_norms", "fc2_bias_alone")]   # (frozen: the tiny ones)


@pytest.mark.parametrize("idx,frozen", LAYER_RUNS)
def test_vit_layer_train_workspace(idx, frozen, monkeypatch):
    """The forward's [sk][xn][qkn] and everything the backward carves behind them; every request of the module is a fresh hostile buffer, so
    the backward starts from 0xFF where the forward left its pieces -- as after another layer's use of the shared workspace.  A frozen
    subset skips producers: no consumer may then read what they would have written."""
    import test_vit_layer_train_gpu as TL
    cfg = LAYER_CASES[idx]
    hidden, heads, inter, B, S, qkn, qkvb = cfg
    trainable = FROZEN[frozen]
    layer, params = TL.build_layer(cfg, seed=idx)
    x, gout = VI.make_io(B, S, hidden, seed=idx, device=DEV)
    need_x = trainable is None
    for n, p in layer.named_parameters():
        p.requires_grad_(trainable is None or n in trainable)

    L = _lib.lib()
    sk = []

    def run(W):      # (test_vit_layer_train_gpu.native_run with the route counter read around each of the two C calls)
        for p in layer.parameters():
            p.grad = None
        xx = x.detach().requires_grad_(need_x)
        c0 = L.vllm_gemm_sk_launches()
        y = layer(xx)
        c1 = L.vllm_gemm_sk_launches()
        y.backward(gout)
        sk.append((c1 - c0, L.vllm_gemm_sk_launches() - c1))
        return dict(y=y.detach(), gx=xx.grad, **{n: (p.grad.clone() if p.grad is not None else None) for n, p in layer.named_parameters()})

    outs, spaces = three_runs(run, widest_row_bytes=max(3 * hidden, inter) * 4, patch=monkeypatch)
    base = outs[0]
    print(f"layer {hidden}/{inter} rows {B * S} {frozen}: stream-K launches (forward, backward) per run {sk}")
    assert len(spaces[0].sizes) == 2, spaces[0].sizes                      # the forward's request and the backward's
    assert len(set(sk)) == 1, sk
    if B * S >= 1024:
        assert min(spaces[0].sizes) >= L.vllm_gemm_scratch_bytes()         # the stream-K scratch is carved
    if idx == 3:       # the case that pins the flag resets of vllm_vit_layer_forward_train and vllm_vit_layer_backward (module docstring)
        assert sk[0][0] >= 1 and sk[0][1] >= 1, sk
    else:
        assert sk[0] == (0, 0), sk
    for p in layer.parameters():
        p.requires_grad_(True)
    y64, g64, gx64 = VI.autograd_layer(params, x, gout, heads, torch.float64)
    y16, g16, gx16 = VI.autograd_layer(params, x, gout, heads, torch.bfloat16)
    rows = [("y", y16, y64)] + ([("gx", gx16, gx64)] if need_x else []) + [(n, g16[n], g64[n]) for n in g64 if trainable is None or n in trainable]
    for name, t16, t64 in rows:       # DESIGN section 5's rule, as test_layer_gradients
        rn, rt = VI.rel_rms(base[name], t64), VI.rel_rms(t16, t64)
        assert rn <= 1.25 * rt, f"{name}: {rn:.4g} > 1.25 x {rt:.4g}"
    for n in g64:
        if trainable is not None and n not in trainable:
            assert base[n] is None, n


@pytest.mark.parametrize("idx", [0, 2])
def test_vit_layer_forward_train_takes_the_head_of_the_workspace(idx):
    """The training forward is served by [sk][xn][qkn] alone (layer_train.cpp's layout comment; the number is derived here, as in
    test_workspace_contract_cpu.py): straight through the C ABI with exactly those bytes, hostile and guarded, it writes the bits the
    module's forward does with the backward's whole workspace."""
    import test_vit_layer_train_gpu as TL
    from visionllm_amd.intern_vit import _SAVED, _layer_desc
    L = _lib.lib()
    cfg = LAYER_CASES[idx]
    hidden, heads, inter, B, S, qkn, qkvb = cfg
    layer, _ = TL.build_layer(cfg, seed=idx)
    x, _ = VI.make_io(B, S, hidden, seed=idx, device=DEV)
    M = B * S
    a256 = lambda v: (v + 255) & ~255  # noqa: E731
    fwd = (a256(L.vllm_gemm_scratch_bytes()) if M >= 1024 else 0) + a256(M * hidden * 2) + (a256(M * 3 * hidden * 2) if qkn else 0)
    keep = []
    d = _layer_desc((heads, inter, VI.EPS), layer._params(), keep)
    assert 0 < fwd < L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), B, S)

    def run(W):
        ws, n = W.take(fwd)
        out = nan_bf16(B, S, hidden)
        saved = [nan_bf16(M, 3 * hidden), nan_bf16(M, hidden), torch.full((B, heads, S), NAN, device=DEV), nan_bf16(M, hidden), nan_bf16(M, hidden),
                 nan_bf16(M, inter), nan_bf16(M, inter), nan_bf16(M, hidden)]
        sv = _lib.VllmVitLayerSaved(**{k: t.data_ptr() for k, t in zip(_SAVED, saved)})
        _lib.check(L.vllm_vit_layer_forward_train(ctypes.byref(d), P(x), B, S, P(out), ctypes.byref(sv), P(ws), n, stream()), "vllm_vit_layer_forward_train")
        return dict(out=out, **dict(zip(_SAVED, saved)))

    base = three_runs(run, widest_row_bytes=3 * hidden * 2)[0][0]
    with torch.no_grad():
        assert torch.equal(base["out"], layer(x))
    for k, t in base.items():
        assert bool(torch.isfinite(t.float()).all()), k


# ---- vllm_bridge_forward_train / vllm_bridge_backward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_x", [False, True])
@pytest.mark.parametrize("kind,n,T,cin,cout,tail", [("linear", 3, 64, 128, 256, False), ("mlp2x_gelu", 3, 64, 128, 256, False),
                                                    ("internvl_mlp", 3, 64, 128, 256, False),
                                                    ("mlp2x_gelu", 4, 256, 128, 256, False),       # 1024 rows: the scratch is carved, the tail not planned
                                                    ("mlp2x_gelu", 4, 256, 1024, 4096, True)])     # 1024 rows of 64-iteration tiles: the tail is taken
def test_bridge_train_workspace(kind, n, T, cin, cout, tail, need_x, monkeypatch):
    """``tail``: whether the forward's and the backward's GEMMs take the stream-K tail, i.e. whether the case pins the flag reset of
    vllm_bridge_forward_train and of vllm_bridge_backward (module docstring)."""
    import test_bridge_train_gpu as TB
    L = _lib.lib()
    br = TB.make_bridge(kind, cin, cout, seed=cin + T)
    torch.manual_seed(T + 1)
    x = bf(torch.randn(n, T, cin, device=DEV))
    gout = bf(torch.randn(n, T, cout, device=DEV) / math.sqrt(cout))
    sk = []

    def run(W):      # (test_bridge_train_gpu.native_grads with the route counter read around each of the two C calls)
        for p in br.parameters():
            p.grad = None
        xx = x.detach().requires_grad_(need_x)
        c0 = L.vllm_gemm_sk_launches()
        y = br(xx)
        c1 = L.vllm_gemm_sk_launches()
        y.backward(gout)
        sk.append((c1 - c0, L.vllm_gemm_sk_launches() - c1))
        return dict(y=y.detach(), gx=xx.grad, **{k: p.grad.clone() for k, p in br.named_parameters()})

    outs, spaces = three_runs(run, widest_row_bytes=max(cin, cout) * 4, patch=monkeypatch)
    base = outs[0]
    print(f"bridge train {kind} {cin}->{cout} rows {n * T}: stream-K launches (forward, backward) per run {sk}")
    assert len(spaces[0].sizes) == 2 and len(set(sk)) == 1, sk
    if n * T >= 1024:
        assert min(spaces[0].sizes) >= L.vllm_gemm_scratch_bytes()
    if tail:
        assert sk[0][0] >= 1 and sk[0][1] >= 1, sk
    else:
        assert sk[0] == (0, 0), sk
    _, g16, gx16 = TB.torch_grads(br, x, gout, torch.bfloat16, need_x)
    _, g64, gx64 = TB.torch_grads(br, x, gout, torch.float64, need_x)
    for name in g64:
        TB.assert_rule(base[name], g16[name], g64[name], f"{kind} rows {n}x{T}: grad {name}")
    if need_x:
        TB.assert_rule(base["gx"], gx16, gx64, f"{kind}: x.grad")


def test_bridge_backward_accepts_null_where_the_query_answers_zero():
    """a Linear projector of 192 rows with a frozen input: no W^T, no split partials, no scratch -- the query answers 0 and NULL / 0 is legal"""
    import test_bridge_train_gpu as TB
    L = _lib.lib()
    br = TB.make_bridge("linear", 128, 256, seed=1)
    d, keep = TB._desc(br, "linear")
    rows = 192
    assert L.vllm_bridge_backward_workspace_bytes(ctypes.byref(d), rows, 0) == 0
    torch.manual_seed(2)
    x, gout = bf(torch.randn(rows, 128, device=DEV)), bf(torch.randn(rows, 256, device=DEV) / 16)
    arr = lambda ts: (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts] + [None] * (4 - len(ts))))  # noqa: E731
    gw, gb = nan_bf16(256, 128), nan_bf16(256)
    _lib.check(L.vllm_bridge_backward(ctypes.byref(d), P(x), rows, P(gout), arr([]), arr([]), None, None, arr([gw]), arr([gb]), None, None, None, 0,
                                      stream()), "vllm_bridge_backward")
    torch.cuda.synchronize()
    assert_bound(gw, gout.double().T @ x.double(), gout.double().abs().T @ x.double().abs(), "Linear grad_w")
    assert_bound(gb, gout.double().sum(0), gout.double().abs().sum(0), "Linear grad_b")


# ---- vllm_bridge_forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ps,n,hw,C,Cl", [("internvl_mlp", True, 3, 8, 128, 256),       # pixel-shuffle gathered by the LayerNorm
                                               ("mlp2x_gelu", False, 4, 16, 1024, 4096)])    # 1024 rows: the stream-K scratch is carved
def test_bridge_forward_workspace(kind, ps, n, hw, C, Cl, monkeypatch):
    from oracle import vit as V
    from visionllm_amd.bridge import build_vl_bridge
    torch.manual_seed(3)
    hidden = bf(torch.randn(n, 1 + hw * hw, C))
    br = build_vl_bridge(kind, C, Cl, use_pixelshuffle=ps)
    with torch.no_grad():
        for p in br.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    sd = {k: bf(v.detach()).float() for k, v in br.state_dict().items()}
    br = br.to(DEV).to(torch.bfloat16).requires_grad_(False)
    hd = hidden.to(DEV)
    L = _lib.lib()
    took = []

    def run(W):
        before = L.vllm_gemm_sk_launches()
        out = br.project_hidden_state(hd, ps)       # the fused path: CLS skipped / shuffled in-kernel
        took.append(L.vllm_gemm_sk_launches() - before)
        return dict(out=out)

    outs, spaces = three_runs(run, widest_row_bytes=max(4 * C, Cl) * 2, patch=monkeypatch)
    print(f"bridge {kind}: workspace {spaces[0].sizes}, stream-K launches per run {took}")
    assert len(spaces[0].sizes) == 1 and len(set(took)) == 1
    if not ps:
        assert n * hw * hw == 1024 and spaces[0].sizes[0] >= L.vllm_gemm_scratch_bytes()
        assert took[0] >= 1, "the stream-K tail (and with it the orchestrator's flag reset) was expected to be exercised"
    else:
        assert took[0] == 0
    ref = V.bridge_forward(sd, kind, V.select_features([hidden.float(), hidden.float()], -2, ps))
    o, r = outs[0]["out"].float().cpu(), ref.float()
    assert (o - r).abs().max().item() <= 1.5e-2 * (r.abs().max().item() + 1e-6)          # test_bridge_vs_oracle's bound


# ---- vllm_vit_forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("golden", ["internvit_small_d64", "clip_small_d64"])
def test_vit_forward_workspace_small_encoders(golden, monkeypatch):
    """The reference-pinned small encoders (QK-norm InternViT and CLIP; head_dim 64 -- the *_tiny fixtures have head_dim 32, which the
    attention kernel refuses) at n = 7 tiles.  Only the last hidden state is asked for: the others live in the workspace's ping-pong."""
    import test_vit_gpu as TV
    from oracle import vit as V
    g = load_golden(golden + ".npz")
    cfgd = ast.literal_eval(str(g["cfg"]))
    sd = golden_sd(g)
    if golden.startswith("clip"):
        from transformers import CLIPVisionConfig
        from visionllm_amd.clip_vit import CLIPVisionModel
        model = CLIPVisionModel(CLIPVisionConfig(**cfgd))
        assert not model.load_state_dict(sd, strict=False).missing_keys
        fwd = lambda s, c, xx: V.clip_vit_forward(s, c, xx)  # noqa: E731
        call = lambda m, xx: m(pixel_values=xx).last_hidden_state  # noqa: E731  (the encoder's last state; no other one is materialised)
    else:
        from visionllm_amd.intern_vit import InternVisionConfig, InternVisionModel
        model = InternVisionModel(InternVisionConfig(**cfgd))
        model.load_state_dict(sd, strict=True)
        fwd = V.intern_vit_forward
        call = lambda m, xx: m(xx).last_hidden_state  # noqa: E731
    model = model.to(DEV).to(torch.bfloat16)
    torch.manual_seed(7)
    x = torch.randn(7, *g["pixel_values"].shape[1:])
    xd = bf(x).to(DEV)

    def run(W):
        return dict(last=call(model, xd))

    outs, spaces = three_runs(run, widest_row_bytes=3 * cfgd["hidden_size"] * 2, patch=monkeypatch)
    assert len(spaces[0].sizes) == 1
    ref, lo = TV._oracle_errors(fwd, sd, cfgd, x)
    TV._check_states([outs[0]["last"]], [ref[-1]], [lo[-1]], golden)


@pytest.mark.parametrize("arch", ["internvit", "internvit_wide"])
def test_vit_forward_workspace_folded_norms(arch, monkeypatch):
    """The folded-norm statistics pieces: the narrow layout ([M][4][2], hidden 1024, one 448 tile = 1025 rows) and the wide one ([M][16],
    hidden 3200, 5 tiles = 5125 rows: the smallest batch whose four GEMMs all take the persistent schedule), two layers.  The wide layout's
    slots beyond ceil(3200 / 256) are read as zeros: the encoder clears them itself, whatever the workspace held.  Bound of the baseline:
    test_folded_norms_agree_with_launched_norms's, against the same model with its norms launched."""
    from visionllm_amd import intern_vit as IV
    from visionllm_amd.intern_vit import InternVisionConfig, InternVisionModel
    from visionllm_amd.vit_common import EncoderPlan
    torch.manual_seed(5)
    wide = arch == "internvit_wide"
    cfgd = dict(hidden_size=3200 if wide else 1024, num_attention_heads=25 if wide else 16, intermediate_size=12800 if wide else 4096,
                num_hidden_layers=2, image_size=448, patch_size=14, qk_normalization=True, qkv_bias=False, hidden_act="gelu", layer_norm_eps=1e-6)
    n = 5 if wide else 1
    model = InternVisionModel(InternVisionConfig(**cfgd))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() >= 2 and "embedding" not in name:
                p.normal_(0, 0.02)
            elif "norm" in name and name.endswith("weight"):
                p.normal_(1.0, 0.2)
            elif name.endswith("ls1") or name.endswith("ls2"):
                p.fill_(0.1)
    x = bf(torch.randn(n, 3, 448, 448)).to(DEV)
    model = model.to(DEV).to(torch.bfloat16)
    L = _lib.lib()
    folded, sk = [], []

    def run(W):
        before, sk0 = L.vllm_vit_folded_gemm_launches(), L.vllm_gemm_sk_launches()
        out = model(x).last_hidden_state
        folded.append(L.vllm_vit_folded_gemm_launches() - before)
        sk.append(L.vllm_gemm_sk_launches() - sk0)
        return dict(last=out)

    outs, spaces = three_runs(run, widest_row_bytes=3 * cfgd["hidden_size"] * 2, patch=monkeypatch)
    assert folded == [2 * 2 + 2 * 1] * 3, folded          # proj + fc1 of both layers, fc2 / qkv between them
    print(f"vit_forward {arch}: stream-K launches per run {sk}")
    assert len(set(sk)) == 1 and sk[0] >= 1, sk           # the stream-K tail is taken: the case pins vllm_vit_forward's flag reset too
    monkeypatch.setattr(IV, "norm_folding_applies", lambda *a, **k: False)
    model._plan = EncoderPlan()                           # the same parameters with the norms launched: a descriptor without the prepared weights
    plain = model(x).last_hidden_state
    assert all(int(getattr(l, "qkv_w_ln") or 0) == 0 for l in model._plan.layers)
    a, b = outs[0]["last"].float(), plain.float()
    rms = ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()
    assert rms <= 6e-3, f"relative rms {rms:.4g} between folded and launched norms"


# ---- vllm_msda_layer_forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shapes,Lq", [([(12, 16), (6, 8), (3, 4)], 50),                       # decoder: few queries, the gather kernel
                                       ([(96, 96), (48, 48), (24, 24), (12, 12)], 900),        # decoder over >= 4096 value rows: the value is kept in bf16
                                       ([(72, 64), (36, 32), (18, 16), (9, 8)], None)],        # encoder (Lq == S): fp32 value, tiled kernels
                         ids=["decoder", "decoder_bf16_value", "encoder"])
def test_msda_layer_workspace(shapes, Lq, masked, monkeypatch):
    import test_msda_gpu as TM
    mod, q, ref, src, ss, lsi, mask = TM._layer_case(2, shapes, Lq, 2, 0, seed=len(shapes) * 7 + 2, masked=masked)

    def run(W):
        with torch.no_grad():
            return dict(out=mod(q, ref, src, ss, lsi, mask))

    outs, spaces = three_runs(run, widest_row_bytes=256 * 3 * 4, patch=monkeypatch)
    assert len(spaces[0].sizes) == 1 and spaces[0].sizes[0] > 0
    truth, ref_bf16 = TM._layer_truth(mod, q, ref, src, ss, lsi, mask)
    o = outs[0]["out"].double().cpu().numpy()
    rms = np.sqrt((truth ** 2).mean())
    err, err_ref = np.sqrt(((o - truth) ** 2).mean()) / rms, np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms
    assert err <= max(err_ref * 1.05, 4e-3), (err, err_ref)                 # test_fused_layer_vs_oracle's bound
    assert np.abs(o - truth).max() <= 2e-2 * np.abs(truth).max()


# ---- the path users take: one stream, one shared grow-only workspace ------------------------------------------------------------------------
def test_shared_workspace_is_dirty_between_the_ops_of_one_stream():
    """bridge -> encoder -> MSDA layer -> FlashAttention hook forward and backward -> one training layer's forward and backward on one
    stream, twice; the second time every buffer of ``_lib._workspaces`` is filled with 0xFF before each op and between the layer's
    forward and backward.  Every result must be the first pass's bits."""
    import test_bridge_train_gpu as TB
    import test_msda_gpu as TM
    import test_vit_layer_train_gpu as TL
    from visionllm_amd.flash_attention import FlashAttention
    from visionllm_amd.intern_vit import InternVisionConfig, InternVisionModel
    g = load_golden("internvit_small_d64.npz")
    enc = InternVisionModel(InternVisionConfig(**ast.literal_eval(str(g["cfg"]))))
    enc.load_state_dict(golden_sd(g), strict=True)
    enc = enc.to(DEV).to(torch.bfloat16)
    torch.manual_seed(11)
    pix = bf(torch.randn(7, *g["pixel_values"].shape[1:])).to(DEV)
    br = TB.make_bridge("internvl_mlp", 128, 256, seed=4).requires_grad_(False)
    hidden = bf(torch.randn(4, 1 + 256, 128, device=DEV))               # 1024 rows: the scratch is carved
    mod, q, ref, src, ss, lsi, mask = TM._layer_case(1, [(12, 16), (6, 8), (3, 4)], 50, 2, 0, seed=9)
    qkv, dout = (t.to(DEV) for t in ati.case("random", 2, 65, 2, 64, torch.bfloat16))
    layer, _ = TL.build_layer(VI.LAYER_CONFIGS[0], seed=0)
    x, gout = VI.make_io(2, 37, 128, seed=0, device=DEV)

    def dirty(on):
        if on:
            assert _lib._workspaces, "the ops were expected to share _lib.workspace"
            for buf in _lib._workspaces.values():
                buf.fill_(WG.HOSTILE)

    def one_pass(hostile):
        out = {}
        dirty(hostile)
        out["bridge"] = br.project_hidden_state(hidden, False)
        dirty(hostile)
        out["encoder"] = enc(pix).last_hidden_state
        dirty(hostile)
        with torch.no_grad():
            out["msda"] = mod(q, ref, src, ss, lsi, mask)
        dirty(hostile)
        xq = qkv.detach().clone().requires_grad_(True)
        o, _ = FlashAttention()(xq)
        dirty(hostile)
        o.backward(dout)
        out["attn"], out["attn_grad"] = o.detach(), xq.grad
        for p in layer.parameters():
            p.grad = None
        dirty(hostile)
        xx = x.detach().requires_grad_(True)
        y = layer(xx)
        dirty(hostile)
        y.backward(gout)
        out.update(layer_y=y.detach(), layer_gx=xx.grad, **{"layer." + n: p.grad.clone() for n, p in layer.named_parameters()})
        torch.cuda.synchronize()
        return out

    first = one_pass(False)
    second = one_pass(True)
    same_bits(second, first, "shared workspace filled with 0xFF")
    for k, v in first.items():
        assert bool(torch.isfinite(v.float()).all()), k
