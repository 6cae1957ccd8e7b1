"""GPU: every row-walking kernel past one trip per thread.

The kernel-alone tests give these kernels so few rows that their loop bodies run once.  Here each one gets the smallest shape of
multitrip_inputs.py for THIS device (its compute-unit count): some thread makes at least 3 trips, the last trip is ragged and so is the
last block.  Every test asserts that precondition before it launches -- for the three norm.hip kernels on the plan read back through the
host-only workspace queries -- and fails, never skips, where it does not hold.

Yardsticks: fp64 of the same statements, computed on the GPU a slice of rows at a time (multitrip_inputs.ref_slices), by the references
and bounds of the kernel-alone tests, imported from their modules:
  norm.hip backward kernels   rms_bwd_ref / ls_bwd_ref (vit_layer_train_inputs), ln_bwd_ref (clip_layer_train_inputs), ``excess_ulp``:
                              |err| <= 1 bf16 ulp + 2^-17 mag, for the row gradient AND the column sums (see ``judge_sums``)
  add_layernorm               1 bf16 ulp + 2^-20 (|n w| + |b|)                          (test_add_layernorm_against_fp64)
  box_refine                  1/4 * 2^-17 (sum|h w| + |b| + |logit|) + 2^-22            (test_refine_kernel_against_fp64)
  qs_tail                     2^-17 (sum|h w| + |b|) + 2^-22 / (p (1 - p)) + 2^-20, a quarter of it + 2^-22 for the reference points
                                                                                        (test_tail_kernel_against_fp64)
  refpoint_embed              1 bf16 ulp + 2^-19, the fp32 product bit-exact            (test_refpoint_kernel_against_fp64)
  segment sum                 1 bf16 ulp + (n - 1) 2^-23 sum|terms|                     (test_token_loops_train_gpu)
  add, conversions, movers    bit-exact
A fixture holds every test to multitrip_inputs.MEM_LIMIT of device memory at its peak."""
import math

import pytest
import torch

import clip_layer_train_inputs as CI
import multitrip_inputs as M
import query_selection_inputs as QI
import test_query_selection_gpu as QT
import vit_layer_train_inputs as VI
from bounds import DEV, P, bf16_ulp, excess_ulp, stream
from visionllm_amd import _lib
from visionllm_amd import deformable_decoder as D

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF = torch.bfloat16


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def bf(t):
    return t.to(BF)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    """bits(a) == bits(b) for two large 2-D views, a slice of rows at a time (no full contiguous copies)"""
    assert a.shape == b.shape
    return all(torch.equal(bits(a[lo:hi]), bits(b[lo:hi])) for lo, hi in M.ref_slices(a.shape[0], a.shape[1]))


def nan_bf16(*shape):
    return torch.full(shape, NAN, dtype=BF, device=DEV)


def padded(t, pad):
    """a copy of the 2-D tensor inside rows `pad` elements wider, the padding NaN"""
    full = nan_bf16(t.shape[0], t.shape[1] + pad)
    full[:, :t.shape[1]] = t
    return full


def view(rows, C, pad, lead, scale=1.0, shift=0.0):
    """a [rows, C] bf16 view with row stride C + pad that starts `lead` elements into its parent -> (parent, view)"""
    parent = torch.empty(rows, C + pad, dtype=BF, device=DEV)
    for a, b in M.ref_slices(rows, C + pad):
        parent[a:b] = bf(torch.randn(b - a, C + pad, device=DEV) * scale + shift)
    v = parent[:, lead:lead + C]
    assert v.data_ptr() % 16 == 0 and v.data_ptr() != parent.data_ptr()
    return parent, v


def rand_rows(rows, C, gen):
    """[rows, C] bf16 of randn, drawn a slice at a time (no fp32 copy of the whole)"""
    out = torch.empty(rows, C, dtype=BF, device=DEV)
    for a, b in M.ref_slices(rows, C):
        out[a:b] = bf(torch.randn(b - a, C, generator=gen, device=DEV))
    return out


def require(case):
    """the multi-trip precondition of a case, by the restated launch arithmetic for this device"""
    assert case.trips >= M.MIN_TRIPS and case.ragged, f"not a multi-trip shape on {cus()} compute units: {case}"
    return case


@pytest.fixture(autouse=True)
def memory_limit():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    yield
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak device memory {peak / 2 ** 20:.0f} MB")
    assert peak < M.MEM_LIMIT, f"{peak / 2 ** 20:.0f} MB of device memory"


# ---- norm.hip: rms_bwd_kernel, ln_res_bwd_kernel, ls_bwd_kernel ------------------------------------------------------------------------
def judge_sums(what, got, ref, mag, rows, nbv):
    """A column sum against fp64 by the kernel-alone tests' bound, unchanged: |err| <= 1 bf16 ulp + 2^-17 sum|terms|.  That term was set
    at 300 rows or fewer; here thousands of rows are added, so the figure a derivation from the kernel's fixed summation order gives is
    printed beside it: the longest chain of fp32 additions is rpb + ceil(nbv / 8) + 8 (a range's registers, a slice of
    colsum_reduce_kernel, its 8 slices), each rounding at most 2^-24 of a partial sum that is at most sum|terms|, so
    |err| <= 1 bf16 ulp + chain 2^-24 sum|terms|.  On 256 compute units the chain is 54 (nbv 343), 97 (nbv 684) or 182 (nbv 1367)
    additions, 2^-18.2 to 2^-16.5.  The unchanged bound holds -- measured there: at most 0.49 of it for every column sum of the three
    kernels, the rounding to bf16 alone -- so the unchanged bound is the one asserted and nothing had to be re-derived."""
    e = excess_ulp(got, ref, mag)
    chain = M.colsum_chain(rows, nbv)
    d = excess_ulp(got, ref, mag, rel_mag=chain * 2.0 ** -24)
    print(f"{what}: {e:.3f} of the bound (1 ulp + 2^-17 mag); {d:.3f} of 1 ulp + {chain} 2^-24 mag")
    assert e <= 1.0, what
    return e


class NormEntry:
    """one of the two norm backward entries behind one call signature; the plan is read back from the host-only size query"""

    def __init__(self, kind, rows, C):
        self.kind, self.rows, self.C, self.L = kind, rows, C, _lib.lib()
        if kind == "rms":
            self.eps, self.nsum, self.name = VI.EPS, 1, "vllm_rmsnorm_backward_bf16"
            self.wsb = self.L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 1)
        else:
            self.eps, self.nsum, self.name = CI.EPS, 2, "vllm_layernorm_backward_res_bf16"
            self.wsb = self.L.vllm_layernorm_backward_res_workspace_bytes(rows, C)
        assert self.wsb > 0 and self.wsb % (self.nsum * C * 4) == 0
        self.nbv = self.wsb // (self.nsum * C * 4)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=DEV)

    def sums(self):
        return [nan_bf16(self.C) for _ in range(self.nsum)]

    def __call__(self, x, gy, w, gx, gres, sums):
        ld = lambda t: 0 if t is None else t.stride(0)   # noqa: E731
        s = list(sums) if sums is not None else [None] * self.nsum
        if self.kind == "rms":
            rc = self.L.vllm_rmsnorm_backward_bf16(P(x), ld(x), P(gy), ld(gy), P(w), None, 1, self.eps, self.rows, self.C, P(gx), ld(gx), P(gres),
                                                   ld(gres), P(s[0]), None, P(self.ws), self.wsb, stream())
        else:
            rc = self.L.vllm_layernorm_backward_res_bf16(P(x), ld(x), P(gy), ld(gy), P(w), self.eps, self.rows, self.C, P(gx), ld(gx), P(gres),
                                                         ld(gres), P(s[0]), P(s[1]), P(self.ws), self.wsb, stream())
        _lib.check(rc, self.name)

    def reference(self, x, gy, w, gres, gx):
        """-> (excess of gx, [column sums], [their magnitudes]); the rows a slice at a time, the column sums added up in fp64"""
        ex, tot = 0.0, None
        for a, b in M.ref_slices(self.rows, self.C):
            gr = None if gres is None else gres[a:b]
            if self.kind == "rms":
                rx, rw, mx, mw = VI.rms_bwd_ref(x[a:b], gy[a:b], w, gr)
                part = [rw, mw]
            else:
                rx, rw, rb, mx, mw, mb = CI.ln_bwd_ref(x[a:b], gy[a:b], w, gr)
                part = [rw, rb, mw, mb]
            if gx is not None:
                ex = max(ex, excess_ulp(gx[a:b], rx, mx))
            tot = part if tot is None else [t + p for t, p in zip(tot, part)]
        return ex, tot[:self.nsum], tot[self.nsum:]


def norm_precondition(rows, nbv):
    """asserted before every launch of the three kernels, on the plan the library itself reports"""
    rpb = M.ceil_div(rows, nbv)
    assert rpb >= 3, f"{rows} rows in {nbv} ranges: {rpb} trips"
    assert rows % rpb != 0, f"{rows} rows in ranges of {rpb}: no range ends early"
    return rpb


def run_norm_backward(kind, C, with_dx, with_res):
    rows = M.norm_rows(C, cus())
    e = NormEntry(kind, rows, C)
    rpb = norm_precondition(rows, e.nbv)
    inputs = VI if kind == "rms" else CI
    x, gy, gres, w = inputs.norm_case(rows, C, device=DEV)
    xf, gyf = padded(x, 8), padded(gy, 16)
    grf = padded(gres, 24) if with_res else None
    gres = gres if with_res else None
    what = f"{kind} bwd {rows}x{C} rpb {rpb} nbv {e.nbv} dx{int(with_dx)} res{int(with_res)}"
    gx = nan_bf16(rows, C + 32) if with_dx else None
    sums = e.sums()
    e(xf[:, :C], gyf[:, :C], w, None if gx is None else gx[:, :C], None if grf is None else grf[:, :C], sums)
    torch.cuda.synchronize()
    ex, ref, mag = e.reference(x, gy, w, gres, None if gx is None else gx[:, :C])
    for name, got, r, m in zip(("grad_w", "grad_b"), sums, ref, mag):
        judge_sums(f"{what} {name}", got, r, m, rows, e.nbv)
    if with_dx:
        print(f"{what}: grad_x {ex:.3f} of the bound")
        assert ex <= 1.0, what
        assert torch.isnan(gx[:, C:]).all(), "wrote into the padding"
    # run-to-run identical; the column sums alone and the row gradient alone give the bits of the joint call
    gx2 = nan_bf16(rows, C + 32) if with_dx else None
    sums2 = e.sums()
    e(xf[:, :C], gyf[:, :C], w, None if gx2 is None else gx2[:, :C], None if grf is None else grf[:, :C], sums2)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(sums, sums2)), what
    if not with_dx:
        return
    assert torch.equal(bits(gx2[:, :C]), bits(gx[:, :C])) and torch.isnan(gx2[:, C:]).all(), what
    gx2.fill_(NAN)
    e(xf[:, :C], gyf[:, :C], w, gx2[:, :C], None if grf is None else grf[:, :C], None)
    assert torch.equal(bits(gx2[:, :C]), bits(gx[:, :C])) and torch.isnan(gx2[:, C:]).all(), f"{what}: the row gradient alone"
    del gx2
    sums3 = e.sums()
    e(xf[:, :C], gyf[:, :C], w, None, None, sums3)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(sums, sums3)), f"{what}: the column sums alone"
    # in place: grad_x is grad_y (row r + 1 is read before row r is stored, and from rpb = 2 on there is a row r + 1)
    g_in, sums4 = gyf.clone(), e.sums()
    e(xf[:, :C], g_in[:, :C], w, g_in[:, :C], None if grf is None else grf[:, :C], sums4)
    assert torch.equal(bits(g_in[:, :C]), bits(gx[:, :C])), f"{what}: in place differs from out of place"
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(sums, sums4)) and torch.isnan(g_in[:, C:]).all(), f"{what}: in place"


VARIANTS = [(False, False), (True, False), (True, True)]   # (grad_res is added into grad_x: there is none without it)


@pytest.mark.parametrize("with_dx,with_res", VARIANTS)
@pytest.mark.parametrize("C", M.NORM_C)
def test_rmsnorm_backward_past_one_row_per_range(C, with_dx, with_res):
    """rms_bwd_kernel, every template instance, ranges of 3 rows, the last one short (and at TPR 64 an empty virtual block in the last
    block): prefetched rows carried across trips, the LDS slot sequence of two sums a row (with grad_x) and of one (without)."""
    run_norm_backward("rms", C, with_dx, with_res)


@pytest.mark.parametrize("with_dx,with_res", VARIANTS)
@pytest.mark.parametrize("C", M.NORM_C_LN)
def test_layernorm_backward_res_past_one_row_per_range(C, with_dx, with_res):
    """ln_res_bwd_kernel likewise: four sums a row with grad_x, two without"""
    run_norm_backward("ln", C, with_dx, with_res)


@pytest.mark.parametrize("C", M.NORM_C)
def test_qk_norm_backward_in_place_on_a_qkv_slab_past_one_row_per_range(C):
    """G = 2 at rpb >= 3: the q and k blocks of a [rows, 3C] gradient rewritten in place in ONE launch have the bits of two out-of-place
    G = 1 launches on the slab's strided blocks, which are judged against fp64 first; the v block is not touched."""
    L = _lib.lib()
    rows = M.norm_rows(C, cus())
    wsb = L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 2)
    assert wsb > 0 and wsb % (2 * C * 4) == 0
    nbv = wsb // (2 * C * 4)
    norm_precondition(rows, nbv)
    assert L.vllm_rmsnorm_backward_workspace_bytes(rows, C, 1) * 2 == wsb
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    torch.manual_seed(C)
    _, qkv = view(rows, 3 * C, 8, 8, 1.5)
    _, g = view(rows, 3 * C, 8, 8)
    ld = 3 * C + 8
    wq, wk = (bf(1 + 0.1 * torch.randn(C, device=DEV)) for _ in range(2))
    gv = g[:, 2 * C:].clone()
    outs = []
    for k, w_ in enumerate((wq, wk)):
        o1, w1 = nan_bf16(rows, C), nan_bf16(C)
        _lib.check(L.vllm_rmsnorm_backward_bf16(P(qkv[:, k * C:]), ld, P(g[:, k * C:]), ld, P(w_), None, 1, VI.EPS, rows, C, P(o1), C, None, 0, P(w1),
                                                None, P(ws), wsb, stream()), "vllm_rmsnorm_backward_bf16 G=1")
        torch.cuda.synchronize()
        ex, rw, mw = 0.0, 0, 0
        for a, b in M.ref_slices(rows, C):
            rx, r_, mx, m_ = VI.rms_bwd_ref(qkv[a:b, k * C:(k + 1) * C], g[a:b, k * C:(k + 1) * C], w_)
            ex, rw, mw = max(ex, excess_ulp(o1[a:b], rx, mx)), rw + r_, mw + m_
        print(f"qk-norm slab {rows}x{C} block {k}: grad_x {ex:.3f} of the bound")
        assert ex <= 1.0
        judge_sums(f"qk-norm slab {rows}x{C} block {k} grad_w", w1, rw, mw, rows, nbv)
        outs.append((o1, w1))
    gwq, gwk = nan_bf16(C), nan_bf16(C)
    _lib.check(L.vllm_rmsnorm_backward_bf16(P(qkv), ld, P(g), ld, P(wq), P(wk), 2, VI.EPS, rows, C, P(g), ld, None, 0, P(gwq), P(gwk), P(ws), wsb,
                                            stream()), "vllm_rmsnorm_backward_bf16 G=2")
    torch.cuda.synchronize()
    assert torch.equal(bits(g[:, 2 * C:]), bits(gv)), "the v block changed"
    for k, (gw, name) in enumerate(((gwq, "q"), (gwk, "k"))):
        assert not torch.isnan(outs[k][0]).any() and not torch.isnan(outs[k][1]).any()
        assert torch.equal(bits(g[:, k * C:(k + 1) * C]), bits(outs[k][0])), f"{name} block: in place on the slab differs from out of place"
        assert torch.equal(bits(gw), bits(outs[k][1])), f"grad_w of the {name} block"


@pytest.mark.parametrize("C", M.NORM_C)
def test_layerscale_backward_past_one_row_per_range(C):
    """ls_bwd_kernel: two rows in flight, ranges of 3 rows (an odd count: the second slot of the last pair is past the range), the last
    range short; grad_y alone, grad_ls alone, and grad_y written over grad_out."""
    L = _lib.lib()
    rows = M.norm_rows(C, cus())
    wsb = L.vllm_layerscale_backward_workspace_bytes(rows, C)
    assert wsb > 0 and wsb % (C * 4) == 0
    nbv = wsb // (C * 4)
    rpb = norm_precondition(rows, nbv)
    go, y, _, w = VI.norm_case(rows, C, seed=1, device=DEV)
    ls = bf(0.1 * w.float())
    gof, yf = padded(go, 8), padded(y, 16)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def call(go_, gy_, gls_):
        _lib.check(L.vllm_layerscale_backward_bf16(P(go_), go_.stride(0), P(yf), C + 16, P(ls), rows, C, P(gy_), 0 if gy_ is None else gy_.stride(0),
                                                   P(gls_), P(ws), wsb, stream()), "vllm_layerscale_backward_bf16")

    gy, gls = nan_bf16(rows, C + 24), nan_bf16(C)
    call(gof, gy, gls)
    torch.cuda.synchronize()
    what = f"layerscale bwd {rows}x{C} rpb {rpb} nbv {nbv}"
    ey, rls, mls = 0.0, 0, 0
    for a, b in M.ref_slices(rows, C):
        ry, r, m = VI.ls_bwd_ref(go[a:b], y[a:b], ls)
        ey = max(ey, excess_ulp(gy[a:b, :C], ry, torch.zeros_like(ry)))
        rls, mls = rls + r, mls + m
    print(f"{what}: grad_y {ey:.3f} of the bound")
    assert ey <= 1.0, what
    judge_sums(f"{what} grad_ls", gls, rls, mls, rows, nbv)
    assert torch.isnan(gy[:, C:]).all(), "wrote into the padding"
    gy2, gls2 = nan_bf16(rows, C + 24), nan_bf16(C)
    call(gof, gy2, gls2)
    assert torch.equal(bits(gy2), bits(gy)) and torch.equal(bits(gls2), bits(gls)), f"{what}: two runs differ"
    gy2.fill_(NAN)
    gls2.fill_(NAN)
    call(gof, gy2, None)
    call(gof, None, gls2)
    assert torch.equal(bits(gy2), bits(gy)) and torch.equal(bits(gls2), bits(gls)), f"{what}: each output alone"
    del gy2
    g_in, gls3 = gof.clone(), nan_bf16(C)
    call(g_in, g_in, gls3)
    assert torch.equal(bits(g_in[:, :C]), bits(gy[:, :C])) and torch.isnan(g_in[:, C:]).all(), f"{what}: grad_y written over grad_out differs"
    assert torch.equal(bits(gls3), bits(gls)), f"{what}: grad_ls of the in-place call"


# ---- add_layernorm_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", M.ALN_C)
def test_add_layernorm_past_one_row_group_per_wave(C):
    """Every wave walks 3 row groups, five of them a fourth; an odd row count (C <= 256: the last half-wave has no row).  With and
    without `res`, with and without `pos` / `y_pos`, every operand an offset view with a row stride of its own, outputs NaN-prefilled;
    y_pos has the bits of vllm_add_bf16(y, pos), the in-place call the bits of the out-of-place one."""
    case = require(M.case(cus(), "add_layernorm", C=C))
    rows = case.sizes["rows"]
    torch.manual_seed(C)
    L = _lib.lib()
    xp, x = view(rows, C, 16, 8, 2.0, 0.3)
    _, res = view(rows, C, 24, 16)
    _, pos = view(rows, C, 8, 8, 0.5)
    w, b = bf(1 + 0.2 * torch.randn(C, device=DEV)), bf(0.2 * torch.randn(C, device=DEV))
    eps = 1e-5
    yp, ypp = nan_bf16(rows, C + 40), nan_bf16(rows, C + 8)
    y, y_pos = yp[:, 32:32 + C], ypp[:, 8:8 + C]

    def call(x_, y_, with_res, with_pos):
        _lib.check(L.vllm_add_layernorm_bf16(P(x_), x_.stride(0), P(res) if with_res else None, C + 24, P(w), P(b), P(y_), y_.stride(0),
                                             P(pos) if with_pos else None, C + 8, P(y_pos) if with_pos else None, C + 8, rows, C, eps, stream()),
                   "add_layernorm")
        torch.cuda.synchronize()

    for with_res, with_pos in ((False, False), (False, True), (True, False), (True, True)):
        yp.fill_(NAN)
        ypp.fill_(NAN)
        call(x, y, with_res, with_pos)
        u = 0.0
        for a, e in M.ref_slices(rows, C):
            xs = x[a:e].double() + (res[a:e].double() if with_res else 0)
            mean = xs.mean(-1, keepdim=True)
            n = (xs - mean) / torch.sqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + eps)
            ref = n * w.double() + b.double()
            err = (y[a:e].double() - ref).abs()
            u = max(u, ((err - 2.0 ** -20 * ((n * w.double()).abs() + b.double().abs())).clamp_min(0) / bf16_ulp(ref)).max().item())
            if with_pos:
                yc, pc, want = y[a:e].contiguous(), pos[a:e].contiguous(), nan_bf16(e - a, C)
                _lib.check(L.vllm_add_bf16(P(yc), P(pc), P(want), (e - a) * C, stream()), "add_bf16")
                torch.cuda.synchronize()
                assert torch.equal(bits(y_pos[a:e]), bits(want)), f"y_pos is not vllm_add_bf16(y, pos) in rows {a}..{e}"
                assert torch.equal(bits(want), bits(yc + pc))
        print(f"add_layernorm C{C} rows{rows} trips{case.trips} res{int(with_res)} pos{int(with_pos)}: max excess {u:.3f} bf16 ulp")
        assert u <= 1.0
        assert torch.isnan(yp[:, :32]).all() and torch.isnan(yp[:, 32 + C:]).all()
        assert torch.isnan(ypp[:, :8]).all() and (torch.isnan(ypp[:, 8:]).all() if not with_pos else True)
    # in place (x is y) against the y of the last out-of-place call
    zp = xp.clone()
    z = zp[:, 8:8 + C]
    call(z, z, True, False)
    assert same_bits(z, y), "the in-place call differs from the out-of-place one"
    assert torch.equal(bits(zp[:, :8]), bits(xp[:, :8])) and torch.equal(bits(zp[:, 8 + C:]), bits(xp[:, 8 + C:]))


# ---- box_refine_kernel ---------------------------------------------------------------------------------------------------------------
REFINE_EPS = 1e-5
SPECIAL = (0.0, 1.0, 1e-6, 1.0 - 1e-6, -0.1, 1.1, 0.5)


@pytest.mark.parametrize("C", M.REFINE_C)
def test_box_refine_past_one_row_group_per_wave(C):
    """`ref` holds 0, 1, both clamps' edges, values outside [0, 1] and whole NaN rows in EVERY trip of the walk (a NaN stays a NaN, as in
    torch.clamp); in place and out of place give the same bits."""
    case = require(M.case(cus(), "box_refine", C=C))
    R = case.sizes["rows"]
    rows_per_trip = case.sizes["nwaves"] * case.sizes["rows_per_group"]
    torch.manual_seed(C)
    _, h = view(R, C, 16, 8)
    h.relu_()
    W, b = bf(0.1 * torch.randn(4, C, device=DEV)), bf(0.1 * torch.randn(4, device=DEV))
    ref = torch.rand(R, 4, device=DEV)
    nan_rows = []
    for t in range(case.trips):
        r0 = t * rows_per_trip
        assert r0 + 3 < R
        ref[r0] = torch.tensor(SPECIAL[:4], device=DEV)
        ref[r0 + 1] = torch.tensor(SPECIAL[3:], device=DEV)
        nan_rows += [r0 + 2, min(r0 + rows_per_trip, R) - 1]
    ref[nan_rows] = NAN
    assert len(set(r // rows_per_trip for r in nan_rows)) == case.trips >= 3

    def run(ref_, out):
        _lib.check(_lib.lib().vllm_box_refine_f32(P(h), h.stride(0), P(W), P(b), P(ref_), P(out), R, C, REFINE_EPS, stream()), "vllm_box_refine_f32")
        torch.cuda.synchronize()
        return out

    got = run(ref, torch.full_like(ref, NAN))
    isnan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), isnan), "NaN rows of ref and NaN rows of the result differ"
    eps64 = float(torch.tensor(REFINE_EPS, dtype=torch.float32))
    worst = 0.0
    for a, e in M.ref_slices(R, C):
        h64, r64 = h[a:e].double(), ref[a:e].double()
        x = r64.clamp(0, 1)
        logit = torch.log(x.clamp(min=eps64) / (1 - x).clamp(min=eps64))
        truth = torch.sigmoid(h64 @ W.double().T + b.double() + logit)
        mag = h64.abs() @ W.double().abs().T + b.double().abs() + logit.abs()
        ok = ~isnan[a:e]
        err = (got[a:e].double() - truth).abs()[ok]
        bound = (0.25 * 2.0 ** -17 * mag + 2.0 ** -22)[ok]
        worst = max(worst, (err / bound).max().item())
    print(f"refine R {R} C {C} trips {case.trips}: max err / bound {worst:.3f}")
    assert worst <= 1.0
    alias = ref.clone()
    run(alias, alias)
    assert torch.equal(bits(alias), bits(got)), "the in-place form differs"
    assert torch.equal(bits(run(ref, torch.full_like(ref, NAN))), bits(got)), "two runs differ"


# ---- qs_tail_kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", M.REFINE_C)
def test_query_select_tail_past_one_row_group_per_wave(C):
    """box_refine's row count (every wave walks 3 row groups, five of them a fourth, the last group ragged) as k * B selected rows over
    the two-level threshold geometry of test_tail_kernel_against_fp64: every trip meets padded rows, invalid proposals and finite ones,
    since the indices are drawn from all of S.  That test's bound, unchanged."""
    rows = M.group_rows(C, cus())
    plan = M.group_plan(rows, C, cus())
    trips = M.ceil_div(plan["ngroups"], plan["nwaves"])
    assert trips >= M.MIN_TRIPS and M.group_ok(rows, C, cus()), f"not a multi-trip shape on {cus()} compute units: {rows} rows, {plan}"
    maps, two = QT.threshold_geometry()
    B = next(n for n in (3, 5, 7, 1) if rows % n == 0)
    k = rows // B
    real = torch.stack([two[(i + 1) % 2] for i in range(B)])          # image 0 is the padded one
    S = real.shape[1]
    g = torch.Generator().manual_seed(C)
    idx = torch.randint(0, S, (B, k), generator=g)
    _, h = view(rows, C, 16, 8)
    h.relu_()
    W, b = bf(0.1 * torch.randn(4, C, device=DEV)), bf(0.1 * torch.randn(4, device=DEV))
    pmask = (~real).to(torch.uint8).to(DEV)
    shapes = torch.tensor(maps, dtype=torch.int64, device=DEV)
    hw = shapes[:, 0] * shapes[:, 1]
    lsi = torch.cumsum(hw, 0) - hw
    idx_dev = idx.to(DEV)
    what = f"tail rows {rows} = {B} x {k} C {C} trips {trips}"

    def run():
        ext = torch.full((B, len(maps), 2), -7, dtype=torch.int32, device=DEV)
        coords = torch.full((rows, 4), NAN, dtype=torch.float32, device=DEV)
        ref = torch.full((rows, 4), NAN, dtype=torch.float32, device=DEV)
        valid = torch.full((rows,), 9, dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib().vllm_query_select_tail_f32(P(h), h.stride(0), P(W), P(b), P(idx_dev), P(pmask), P(shapes), P(lsi), B, S, len(maps), k,
                                                         C, P(ext), P(coords), P(ref), P(valid), stream()), "vllm_query_select_tail_f32")
        torch.cuda.synchronize()
        return ext, coords, ref, valid
    ext, coords, ref, valid = run()
    flags = QT.torch_valid_flags(~real.to(DEV), maps).cpu()
    assert torch.equal(valid.cpu().bool().view(B, k), torch.gather(flags, 1, idx)), f"{what}: validity flags differ from torch's fp32 statements"
    logit, _ = QI.closed_form_proposals(real, maps)
    logit = torch.gather(logit, 1, idx[..., None].expand(-1, -1, 4)).view(rows, 4).to(DEV)
    filled = torch.gather(~flags | ~real, 1, idx).view(rows).to(DEV)
    rows_per_trip = plan["nwaves"] * plan["rows_per_group"]
    for t in range(trips):
        f = filled[t * rows_per_trip:(t + 1) * rows_per_trip]
        assert f.any() and (~f).any(), f"{what}: trip {t} lacks filled or finite rows"
    assert torch.equal(torch.isinf(coords), filled[:, None].expand(-1, 4)) and (coords[filled] > 0).all(), f"{what}: +inf exactly at filled rows"
    assert (ref[filled] == 1.0).all(), f"{what}: sigmoid(+inf) is 1.0"
    W64, b64 = W.double(), b.double()
    worst = worst_ref = 0.0
    for a, e in M.ref_slices(rows, C):
        fin = ~filled[a:e]
        h64 = h[a:e].double()
        z = (h64 @ W64.T + b64)[fin] + logit[a:e][fin]
        p = torch.sigmoid(logit[a:e][fin])
        bound = 2.0 ** -17 * (h64.abs() @ W64.abs().T + b64.abs())[fin] + 2.0 ** -22 / (p * (1 - p)) + 2.0 ** -20
        assert torch.isfinite(coords[a:e][fin]).all(), what
        worst = max(worst, ((coords[a:e][fin].double() - z).abs() / bound).max().item())
        worst_ref = max(worst_ref, ((ref[a:e][fin].double() - torch.sigmoid(z)).abs() / (0.25 * bound + 2.0 ** -22)).max().item())
    print(f"{what}: coords max err / bound {worst:.3f}; reference points err / bound {worst_ref:.3f}")
    assert worst <= 1.0 and worst_ref <= 1.0, what
    for x, y in zip(run(), (ext, coords, ref, valid)):
        assert torch.equal(QT.bits(x), QT.bits(y)), f"{what}: two runs differ"


# ---- refpoint_embed_kernel -----------------------------------------------------------------------------------------------------------
def test_refpoint_embed_past_one_chunk_per_thread():
    """P = 128, L = 4; rows = 5 Lq with Lq two fifths of a trip's rows, so the image index (and with it the valid ratios) changes inside
    every trip."""
    case = require(M.refpoint_case(cus()))
    s = case.sizes
    B, Lq, Lv, Pf, rows = s["B"], s["Lq"], s["L"], s["P"], s["rows"]
    assert Lq < s["rows_per_trip"] and rows * (Pf // 2) > 2 * s["rows_per_trip"] * (Pf // 2)
    g = torch.Generator(device=DEV).manual_seed(rows)
    ref = torch.rand(B, Lq, 4, generator=g, device=DEV)
    flat = ref.view(-1, 4)
    for r0 in [t * s["rows_per_trip"] for t in range(case.trips)] + [b * Lq for b in range(B)]:
        flat[r0] = torch.tensor([0.0, 0.5, 1.0, 0.5], device=DEV)
        flat[min(r0 + 1, rows - 1)] = torch.tensor([1.0, 0.0, 0.5, 1.0], device=DEV)
    vr = 1.0 - 0.5 * torch.rand(B, Lv, 2, generator=g, device=DEV)
    vr[0, 0] = 1.0                      # so that level 0 of image 0 keeps 0, 0.5 and 1 exactly
    dim_t = D.GroundingDinoDecoder._dim_t(Pf, torch.device(DEV))

    def run():
        parent = nan_bf16(rows, 4 * Pf + 24)
        sine = parent[:, 8:8 + 4 * Pf]
        rpi = torch.full((B, Lq, Lv, 4), NAN, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().vllm_refpoint_embed_bf16(P(ref), P(vr), P(dim_t), B, Lq, Lv, 4, Pf, P(rpi), P(sine), parent.stride(0), stream()),
                   "vllm_refpoint_embed_bf16")
        torch.cuda.synchronize()
        return rpi, sine, parent

    rpi, sine, parent = run()
    want_rpi = ref[:, :, None] * torch.cat([vr, vr], -1)[:, None]
    assert torch.equal(bits(rpi), bits(want_rpi)), "reference_points_input is not torch's fp32 product"
    assert torch.isnan(parent[:, :8]).all() and torch.isnan(parent[:, 8 + 4 * Pf:]).all(), "wrote outside the 4 P columns"
    lvl0 = want_rpi[:, :, 0].reshape(rows, 4)
    dt = dim_t.double()
    even = torch.arange(Pf, device=DEV) % 2 == 0
    worst = 0.0
    for a, e in M.ref_slices(rows, 4 * Pf):
        l0 = lvl0[a:e].double()
        truth = torch.cat([torch.where(even, v.sin(), v.cos()) for v in (l0[:, k, None] * (2 * math.pi) / dt for k in (1, 0, 2, 3))], -1)
        got = sine[a:e].double()
        assert torch.isfinite(got).all()
        worst = max(worst, (((got - truth).abs() - 2.0 ** -19).clamp_min(0) / bf16_ulp(truth)).max().item())
    print(f"refpoint rows {rows} = {B} x {Lq} L {Lv} P {Pf} trips {case.trips}: max excess {worst:.3f} bf16 ulp")
    assert worst <= 1.0
    assert torch.equal(sine[0, Pf:2 * Pf].double(), torch.where(even, 0.0, 1.0).double())   # sin(0) = 0, cos(0) = 1 in every feature of x = 0
    rpi2, sine2, _ = run()
    assert torch.equal(bits(sine), bits(sine2)) and torch.equal(bits(rpi), bits(rpi2)), "two runs differ"


# ---- add_bf16_kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["aligned", "misaligned"])
def test_add_bf16_past_one_step_per_thread(which):
    """aligned: 16-byte vectors for 3 trips and a scalar tail of 3 elements; off by one element: the element loop for 3 trips"""
    case = require(M.case(cus(), f"add_bf16_{which}"))
    n, lead = case.sizes["n"], case.sizes["lead"]
    assert n % 8 == 3 if which == "aligned" else lead == 1
    torch.manual_seed(n)
    a, b, parent = (torch.empty(n + 16, dtype=BF, device=DEV) for _ in range(3))
    for lo, hi in M.ref_slices(n + 16, 1):
        a[lo:hi] = bf(torch.randn(hi - lo, device=DEV) * 3)
        b[lo:hi] = bf(torch.randn(hi - lo, device=DEV))
    parent.fill_(NAN)
    a, b, out = a[lead:lead + n], b[lead:lead + n], parent[lead:lead + n]
    assert (a.data_ptr() % 16 == 0) == (which == "aligned")
    _lib.check(_lib.lib().vllm_add_bf16(P(a), P(b), P(out), n, stream()), "add_bf16")
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), (a + b).view(torch.int16))
    assert torch.isnan(parent[:lead]).all() and torch.isnan(parent[lead + n:]).all()


# ---- f32_to_bf16_kernel, f32_to_bf16_masked_kernel (both forms), bf16_to_f32_kernel --------------------------------------------------
TIES = (1.00390625, 1.01171875, -1.00390625, -1.01171875)   # half way between two bf16 numbers: to the even one


def test_f32_to_bf16_past_one_vector_per_thread():
    case = require(M.case(cus(), "f32_to_bf16"))
    n = case.sizes["n"]
    assert n % 4 == 3
    torch.manual_seed(0)
    x = torch.randn(n, device=DEV) * 100
    x[::7] = torch.tensor(TIES, device=DEV).repeat(M.ceil_div(M.ceil_div(n, 7), 4))[:M.ceil_div(n, 7)]
    parent = nan_bf16(n + 8)
    _lib.check(_lib.lib().vllm_f32_to_bf16(P(x), P(parent), n, stream()), "vllm_f32_to_bf16")
    torch.cuda.synchronize()
    assert torch.equal(parent[:n].view(torch.int16), x.to(BF).view(torch.int16)) and torch.isnan(parent[n:]).all()


@pytest.mark.parametrize("form", ["vector", "scalar"])
def test_masked_narrowing_past_one_step_per_thread(form):
    """masked rows in every trip, all of them NaN in the source: none gets through; a live NaN stays a NaN"""
    case = require(M.case(cus(), f"f32_to_bf16_masked_{form}"))
    rows, cols, per_trip = case.sizes["rows"], case.sizes["cols"], case.sizes["elems_per_trip"]
    assert (cols % 4 == 0) == (form == "vector")
    first = [t * per_trip // cols for t in range(case.trips + 1)]       # the row in which trip t begins (the last trip: inside the last row)
    assert first[case.trips - 1] == rows - 1 and first[case.trips] >= rows
    g = torch.Generator(device=DEV).manual_seed(rows + cols)
    src = torch.randn(rows, cols, generator=g, device=DEV).mul_(3)
    flat = src.view(-1)
    k = M.ceil_div(rows * cols, 7)
    flat[::7] = torch.tensor(TIES, device=DEV).repeat(M.ceil_div(k, 4))[:k]
    mask = torch.rand(rows, generator=g, device=DEV) < 0.3
    for t in range(case.trips - 1):
        mask[first[t] + 1] = True          # a masked row in every trip, whatever the draw
        mask[first[t] + 2] = False
    mask[-1] = True                        # (the last trip is the end of the last row)
    assert all(bool(mask[first[t]:min(first[t + 1] + 1, rows)].any()) for t in range(case.trips)) and case.trips >= 3
    src[mask] = NAN
    live = [first[t] + 2 for t in range(case.trips - 1)]
    src[live, cols - 1] = NAN
    want = src.to(BF)
    want_nan = torch.isnan(want)
    lib = _lib.lib()
    for m in (mask, None):
        parent = torch.full((rows * cols + 8,), 7.0, dtype=BF, device=DEV)
        dst = parent[:rows * cols].view(rows, cols)
        dm = None if m is None else m.to(torch.uint8)
        _lib.check(lib.vllm_f32_to_bf16_masked(P(src), P(dst), rows, cols, P(dm), stream()), "vllm_f32_to_bf16_masked")
        torch.cuda.synchronize()
        assert (parent[rows * cols:] == 7.0).all()
        assert bool(torch.isnan(dst[live, cols - 1]).all()), "a live NaN did not stay a NaN"
        for a, b in M.ref_slices(rows, cols):              # (a slice of rows at a time: no index tensors of the whole)
            d, wn = dst[a:b], want_nan[a:b]
            db, wb = d.view(torch.int16), want[a:b].view(torch.int16)
            keep = torch.ones(b - a, 1, dtype=torch.bool, device=DEV) if m is None else ~mask[a:b, None]
            assert bool((db.masked_fill(keep, 0) == 0).all()), "masked rows are not exact zeros"
            assert torch.equal(torch.isnan(d) & keep, wn & keep), "NaNs of the kept rows"
            ok = keep & ~wn
            assert torch.equal(db.masked_fill(~ok, 0), wb.masked_fill(~ok, 0)), "kept rows are not torch's round-to-nearest-even"


def test_widening_past_one_chunk_per_thread():
    case = require(M.case(cus(), "bf16_to_f32"))
    n = case.sizes["n"]
    assert n % 8 == 5
    g = torch.Generator(device=DEV).manual_seed(n)
    src = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int16, device=DEV)   # every bf16 pattern, NaNs and infinities included
    dst = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().vllm_bf16_to_f32(P(src), P(dst), n, stream()), "vllm_bf16_to_f32")
    torch.cuda.synchronize()
    got = dst.view(torch.int32)
    for a, b in M.ref_slices(n, 1):
        assert torch.equal(got[a:b], src[a:b].to(torch.int32) << 16), (a, b)
    assert (got[n:] == 0).all()


# ---- embed.hip: scatter_rows, copy_rows, copy_rows_masked, rows_segment_sum ----------------------------------------------------------
def guarded(rows, C, fill=None):
    """[1 + rows + 1, C]: the output between two guard rows of NaN"""
    buf = nan_bf16(rows + 2, C)
    if fill is not None:
        buf[1:-1] = fill
    return buf


def guards_untouched(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


def mover_case(kernel, C):
    case = require(M.case(cus(), kernel, C=C))
    assert case.sizes["rows"] == 3 * 16384 + 5
    return case, case.sizes["rows"], (case.trips - 1) * case.sizes["waves"] // (case.sizes["items"] // case.sizes["rows"])


@pytest.mark.parametrize("C", M.MOVER_C)
@pytest.mark.parametrize("entry", ["scatter_rows", "copy_rows"])
def test_row_movers_past_one_row_per_wave(entry, C):
    """a permutation into 11 more destination rows than there are sources; out-of-range and negative indices in the last trip (copy_rows:
    on both sides, and source rows read twice)"""
    case, n, last = mover_case(entry, C)
    L_ = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(C)
    dst_rows, src_rows = n + 11, n
    src = rand_rows(n, C, g)
    di = torch.randperm(dst_rows, generator=g, device=DEV)[:n]
    di[last], di[n - 2], di[n - 4] = -7, dst_rows + 4, -1
    si = torch.arange(n, device=DEV)
    if entry == "copy_rows":
        si = torch.randint(0, src_rows, (n,), generator=g, device=DEV)
        si[last + 2], si[n - 1] = src_rows, -2
    assert last >= 2 * 16384 and n - 4 > last
    dst0 = rand_rows(dst_rows, C, g)
    ok = (di >= 0) & (di < dst_rows) & (si >= 0) & (si < src_rows)
    want = dst0.clone()
    want[di[ok]] = src[si[ok]]
    assert int(ok.sum()) == n - (3 if entry == "scatter_rows" else 5)

    def run():
        buf = guarded(dst_rows, C, dst0)
        if entry == "scatter_rows":
            rc = L_.vllm_scatter_rows_bf16(P(src), P(di), P(buf[1:]), n, C, dst_rows, stream())
        else:
            rc = L_.vllm_copy_rows_bf16(P(src), P(si), P(buf[1:]), P(di), n, C, src_rows, dst_rows, stream())
        assert rc == 0, L_.vllm_last_error().decode()
        torch.cuda.synchronize()
        assert guards_untouched(buf)
        return buf

    first = run()
    assert torch.equal(bits(first[1:-1]), bits(want))
    del want
    assert torch.equal(bits(run()), bits(first)), "two runs differ"


@pytest.mark.parametrize("C", M.MOVER_C)
def test_masked_copy_past_one_row_per_wave(C):
    case, rows, last = mover_case("copy_rows_masked", C)
    g = torch.Generator(device=DEV).manual_seed(C + 1)
    base = rand_rows(rows, C, g)
    flag = (torch.rand(rows, generator=g, device=DEV) < 0.3).to(torch.uint8) * 3        # (any non-zero flag)
    for t in range(case.trips):
        flag[t * 16384], flag[t * 16384 + 1] = 3, 0
    flag[-1] = 1
    src = base.clone()
    src[flag != 0] = NAN                                                                 # a flagged row's values must not propagate
    want = base
    want[flag != 0] = 0
    outs = []
    for _ in range(2):
        buf = guarded(rows, C)
        assert _lib.lib().vllm_copy_rows_masked_bf16(P(src), P(flag), P(buf[1:]), rows, C, stream()) == 0
        torch.cuda.synchronize()
        assert guards_untouched(buf)
        outs.append(buf)
    assert torch.equal(bits(outs[0][1:-1]), bits(want)) and torch.equal(bits(outs[1]), bits(outs[0]))


@pytest.mark.parametrize("C", M.MOVER_C)
def test_segment_sum_past_one_row_per_wave(C):
    """segments of 0, 1 and 3 terms in turn (so in every trip); in the last trip one three-term segment has an index past src_rows and a
    negative one.  Empty segments are +0.0, one term is a bit-exact copy, three terms meet the bound of test_token_loops_train_gpu."""
    case, rows, last = mover_case("rows_segment_sum", C)
    src_rows = 4096
    g = torch.Generator(device=DEV).manual_seed(C + 2)
    src = rand_rows(src_rows, C, g)
    lens = torch.tensor([0, 1, 3], device=DEV).repeat(M.ceil_div(rows, 3))[:rows]
    seg_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), lens.cumsum(0)])
    n_idx = int(seg_ptr[-1])
    idx = torch.randint(0, src_rows, (n_idx,), generator=g, device=DEV)
    d_bad = rows - 1 - (rows - 1 - 2) % 3                       # the last segment of three terms
    assert int(lens[d_bad]) == 3 and d_bad >= last >= 2 * 16384
    idx[seg_ptr[d_bad]], idx[seg_ptr[d_bad] + 2] = src_rows + 5, -3
    valid = (idx >= 0) & (idx < src_rows)
    seg_of = torch.repeat_interleave(torch.arange(rows, device=DEV), lens)
    n = torch.zeros(rows, dtype=torch.int64, device=DEV).index_add_(0, seg_of, valid.to(torch.int64))
    assert int(n[d_bad]) == 1 and set(n.unique().tolist()) == {0, 1, 3}
    outs = []
    for _ in range(2):
        buf = guarded(rows, C)
        rc = _lib.lib().vllm_rows_segment_sum_bf16(P(src), src_rows, P(seg_ptr), P(idx), n_idx, P(buf[1:]), rows, C, stream())
        assert rc == 0, _lib.lib().vllm_last_error().decode()
        torch.cuda.synchronize()
        assert guards_untouched(buf)
        outs.append(buf)
    assert torch.equal(bits(outs[0]), bits(outs[1]))
    out = outs[0][1:-1]
    assert (bits(out[n == 0]) == 0).all()
    one = torch.zeros(rows, dtype=torch.int64, device=DEV).index_add_(0, seg_of[valid], idx[valid])   # n == 1: the index of the one term
    assert torch.equal(bits(out[n == 1]), bits(src[one[n == 1]]))
    worst = 0.0
    for a, b in M.ref_slices(rows, C):
        k0, k1 = int(seg_ptr[a]), int(seg_ptr[b])
        v = valid[k0:k1]
        terms = src[idx[k0:k1][v]].double()
        ref = torch.zeros(b - a, C, dtype=torch.float64, device=DEV).index_add_(0, seg_of[k0:k1][v] - a, terms)
        mag = torch.zeros(b - a, C, dtype=torch.float64, device=DEV).index_add_(0, seg_of[k0:k1][v] - a, terms.abs())
        err = (out[a:b].double() - ref).abs()
        worst = max(worst, ((err - 2.0 ** -23 * (n[a:b, None] - 1).clamp_min(0) * mag).clamp_min(0) / bf16_ulp(ref)).max().item())
    print(f"segment sum {rows} rows C {C} trips {case.trips}: max excess {worst:.3f} bf16 ulp")
    assert worst <= 1.0
