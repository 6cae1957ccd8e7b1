"""GPU: the training path of the four token loops around the LLM (``native_backward=True`` in visionllm_amd/splice.py) and the two row
kernels behind it (vllm_rows_segment_sum_bf16, vllm_copy_rows_masked_bf16).  Every gradient is compared with torch's fp64 autograd of
oracle/tokens.py on the same bf16-rounded tensors: bit-exact where a gradient row is a copy or an exactly representable sum, and within

    bf16_ulp(exact) + (n - 1) * 2^-23 * sum|terms|

where n terms are added: n - 1 fp32 roundings of at most 2^-24 of a partial sum that is at most sum|terms|, doubled for the second-order
terms, plus the one rounding to bf16.  Nothing in the bound is measured."""
import pytest
import torch

from bounds import P, assert_bound, rel_rms, stream
from conftest import load_golden
from oracle import tokens as T
from test_splice_train_gpu import offset_view
from visionllm_amd import _lib
from visionllm_amd import splice as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
BF = torch.bfloat16


def bf(x):
    return x.to(BF)


def bits(t):
    return t.contiguous().view(torch.int16)


def nan_rows(rows, C):
    """[1 + rows + 1, C] of NaN: the output with one guard row before and one after."""
    return torch.full((rows + 2, C), NAN, dtype=BF, device=DEV)


def guards_untouched(buf):
    return bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all())


# ---- 1: the kernels alone through the C ABI ------------------------------------------------------------------------------------------
DST_ROWS, SRC_ROWS = 37, 50


def segment_case(C, integer, seed=0):
    """37 destination rows: rows 0, 17, 36 empty (17 through a decreasing seg_ptr pair, so row 18 walks two of row 16's terms again);
    rows 1 and 2 one term each, the source rows that hold +-inf / -0.0; row 5 two terms, row 9 three, row 20 thirty-seven; row 12 three
    terms of which one index is past src_rows and one negative; row 35's end and row 36's pair lie beyond n_idx (clamped); every other
    row one term."""
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(-8, 9, (SRC_ROWS, C), generator=gen).float() if integer else torch.randn(SRC_ROWS, C, generator=gen)
    src[0, 0::4], src[0, 1::4], src[0, 2::4] = float("inf"), float("-inf"), -0.0
    src[1] = -0.0
    lens = {d: 1 for d in range(DST_ROWS)}
    lens.update({0: 0, 17: 0, 36: 0, 5: 2, 9: 3, 20: 37, 12: 3})
    seg_ptr, idx = [0], []
    for d in range(DST_ROWS):
        for _ in range(lens[d]):
            idx.append(int(torch.randint(2, SRC_ROWS, (1,), generator=gen)))
        seg_ptr.append(len(idx))
    idx[seg_ptr[1]], idx[seg_ptr[2]] = 0, 1                       # rows 1 and 2: the special source rows, alone in their segments
    idx[seg_ptr[12] + 1], idx[seg_ptr[12] + 2] = SRC_ROWS + 5, -3
    seg_ptr[18] -= 2                                              # (17, 18) decreasing: row 17 empty; row 18 = rows 15's and 16's terms and its own
    n_idx = len(idx)
    seg_ptr[36], seg_ptr[37] = n_idx + 7, n_idx + 9
    return bf(src), torch.tensor(seg_ptr), torch.tensor(idx)


def segment_reference(src, seg_ptr, src_idx):
    """The contract in a Python loop, fp64: -> (sums, sum of |terms|, number of valid terms) per destination row."""
    src = src.double()
    n_idx, rows = src_idx.numel(), seg_ptr.numel() - 1
    out, mag, n = torch.zeros(rows, src.shape[1], dtype=torch.float64), torch.zeros(rows, src.shape[1], dtype=torch.float64), [0] * rows
    for d in range(rows):
        lo, hi = (min(max(int(v), 0), n_idx) for v in (seg_ptr[d], seg_ptr[d + 1]))
        for k in range(lo, hi):
            r = int(src_idx[k])
            if 0 <= r < src.shape[0]:
                out[d] += src[r]
                mag[d] += src[r].abs()
                n[d] += 1
    return out, mag, torch.tensor(n)


def run_segment_sum(src, seg_ptr, src_idx, dst_rows, C, buf=None, expect=0, src_ptr=None, dst_ptr=None):
    buf = nan_rows(dst_rows, C) if buf is None else buf
    dst = buf[1:]
    rc = _lib.lib().vllm_rows_segment_sum_bf16(src_ptr or P(src), 0 if src is None else src.shape[0], P(seg_ptr), P(src_idx),
                                               0 if src_idx is None else src_idx.numel(), dst_ptr or P(dst), dst_rows, C, stream())
    assert rc == expect, (rc, _lib.lib().vllm_last_error().decode())
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("C", [8, 72, 520, 2056])   # one chunk; below a wave; one chunk past a 512-channel slab; the unrolled mover + a tail
def test_segment_sum_alone(C):
    for integer in (True, False):
        src, seg_ptr, idx = segment_case(C, integer)
        ref, mag, n = segment_reference(src, seg_ptr, idx)
        assert n.tolist()[:3] == [0, 1, 1] and n[5] == 2 and n[9] == 3 and n[12] == 1 and n[17] == 0 and n[18] == 3 and n[20] == 37 \
            and n[35] == 1 and n[36] == 0
        src_d, sp_d, idx_d = src.to(DEV), seg_ptr.to(DEV), idx.to(DEV)
        before = src_d.clone()
        buf = run_segment_sum(src_d, sp_d, idx_d, DST_ROWS, C)
        out = buf[1:-1].cpu()
        assert guards_untouched(buf) and torch.equal(bits(src_d), bits(before))
        for d in (0, 17, 36):
            assert torch.equal(bits(out[d]), torch.zeros(C, dtype=torch.int16)), d           # empty: +0.0 in every channel
        for d in range(DST_ROWS):
            if n[d] == 1:                                                                     # one term: the source row's bits
                lo = min(max(int(seg_ptr[d]), 0), idx.numel())
                r = next(int(idx[k]) for k in range(lo, idx.numel()) if 0 <= int(idx[k]) < SRC_ROWS)
                assert torch.equal(bits(out[d]), bits(src[r])), d
        finite = [d for d in range(DST_ROWS) if d not in (1, 2)]
        if integer:
            assert torch.equal(out[finite], bf(ref[finite]))
        else:
            assert_bound(out[finite], ref[finite], (n[finite][:, None] - 1).clamp_min(0) * mag[finite], f"segment sum C={C}", rel_mag=2.0 ** -23)
        assert torch.equal(bits(run_segment_sum(src_d, sp_d, idx_d, DST_ROWS, C)), bits(buf))  # the same bits on a second run


@pytest.mark.parametrize("C", [8, 72, 520, 2056])
def test_masked_copy_alone(C):
    rows = 11
    gen = torch.Generator().manual_seed(C)
    base = bf(torch.randn(rows, C, generator=gen))
    patterns = {"none": [0] * rows, "all": [1] * rows, "ends": [1] + [0] * (rows - 2) + [1], "alternating": [r & 1 for r in range(rows)]}
    for name, flags in patterns.items():
        src = base.clone()
        for r, f in enumerate(flags):
            if f:
                src[r, 0::2], src[r, 1::2] = NAN, float("inf") if r & 2 else float("-inf")   # a flagged row's values must not propagate
        src_d, flag_d = src.to(DEV), torch.tensor([3 * f for f in flags], dtype=torch.uint8, device=DEV)   # (any non-zero flag)
        outs = []
        for _ in range(2):
            buf = nan_rows(rows, C)
            assert _lib.lib().vllm_copy_rows_masked_bf16(P(src_d), P(flag_d), P(buf[1:]), rows, C, stream()) == 0
            torch.cuda.synchronize()
            outs.append(buf)
        out = outs[0][1:-1].cpu()
        assert guards_untouched(outs[0]) and torch.equal(bits(outs[0]), bits(outs[1])), name
        for r, f in enumerate(flags):
            want = torch.zeros(C, dtype=torch.int16) if f else bits(base[r])
            assert torch.equal(bits(out[r]), want), (name, r)


def test_refusals_write_nothing_and_empty_calls_are_accepted():
    C = 72
    L_ = _lib.lib()
    src, seg_ptr, idx = (t.to(DEV) for t in segment_case(C, True))
    err = lambda: L_.vllm_last_error().decode()   # noqa: E731
    odd_src = offset_view(src, 8, False)
    buf = nan_rows(DST_ROWS, C)
    for kwargs, text in (({"src": P(odd_src)}, "16-byte aligned"), ({"C": 12}, "multiple of 8"), ({"seg_ptr": None}, "null seg_ptr or dst"),
                         ({"src_idx": None}, "null src or src_idx")):
        a = {"src": P(src), "seg_ptr": P(seg_ptr), "src_idx": P(idx), "C": C, **kwargs}
        rc = L_.vllm_rows_segment_sum_bf16(a["src"], SRC_ROWS, a["seg_ptr"], a["src_idx"], idx.numel(), P(buf[1:]), DST_ROWS, a["C"], stream())
        assert rc == -1 and text in err(), (kwargs, err())
    assert L_.vllm_rows_segment_sum_bf16(P(src), SRC_ROWS, P(seg_ptr), P(idx), idx.numel(), P(offset_view(buf, 8, False)), 4, C, stream()) == -1
    assert "16-byte aligned" in err()
    assert L_.vllm_rows_segment_sum_bf16(None, SRC_ROWS, P(seg_ptr), P(idx), idx.numel(), P(buf[1:]), DST_ROWS, C, stream()) == -1
    assert "null src or src_idx" in err()
    assert L_.vllm_rows_segment_sum_bf16(P(src), SRC_ROWS, P(seg_ptr), P(idx), idx.numel(), None, DST_ROWS, C, stream()) == -1
    assert "null seg_ptr or dst" in err()
    flags = torch.zeros(DST_ROWS, dtype=torch.uint8, device=DEV)
    some = src[:DST_ROWS]
    for args, text in (((P(odd_src), P(flags), P(buf[1:]), DST_ROWS, C), "16-byte aligned"), ((P(some), P(flags), P(buf[1:]), DST_ROWS, 12), "multiple of 8"),
                       ((None, P(flags), P(buf[1:]), DST_ROWS, C), "null src"), ((P(some), None, P(buf[1:]), DST_ROWS, C), "null src"),
                       ((P(some), P(flags), None, DST_ROWS, C), "null src")):
        assert L_.vllm_copy_rows_masked_bf16(*args, stream()) == -1 and text in err(), (text, err())
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    # empty calls
    assert L_.vllm_rows_segment_sum_bf16(P(src), SRC_ROWS, P(seg_ptr), P(idx), idx.numel(), P(buf[1:]), 0, C, stream()) == 0
    assert L_.vllm_copy_rows_masked_bf16(P(some), P(flags), P(buf[1:]), 0, C, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    zeros = run_segment_sum(None, seg_ptr, None, DST_ROWS, C)       # n_idx == 0 with src == NULL: every row becomes zero
    assert guards_untouched(zeros) and torch.equal(bits(zeros[1:-1]), torch.zeros(DST_ROWS, C, dtype=torch.int16, device=DEV))


# ---- helpers for the function tests ----------------------------------------------------------------------------------------------------
def leaf64(t):
    return t.detach().cpu().double().requires_grad_(True)


def nonleaf(t):
    """-> (leaf on the device that requires grad, a non-leaf copy of it for the in-place functions)."""
    leaf = t.detach().clone().to(DEV).requires_grad_(True)
    return leaf, leaf * 1


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


# ---- 2: splice_region_tokens ---------------------------------------------------------------------------------------------------------------
REG = 77


def region_splice_case():
    torch.manual_seed(9)
    B, L, C = 3, 40, 128
    ids = torch.randint(100, 200, (B, L))
    ids[0, 3] = ids[0, 9] = REG
    ids[2, 1] = ids[2, 2] = ids[2, 30] = REG
    return ids, bf(torch.randn(B, L, C)), bf(torch.randn(5, C)), bf(torch.randn(B, L, C))


def region_splice_reference(ids, emb, feats, grad_out):
    e, f = leaf64(emb), leaf64(feats)
    T.region_splice(e, ids, REG, f).backward(grad_out.double())
    return bf(e.grad), bf(f.grad)


def region_splice_native(ids, emb, feats, grad_out, need=(True, True), feats_dtype=BF, retain=False):
    e = emb.to(DEV).requires_grad_(need[0])
    f = feats.to(DEV).to(feats_dtype).requires_grad_(need[1])
    x = e * 1 if need[0] else e.clone()
    out = S.splice_region_tokens(x, ids.to(DEV), REG, f, native_backward=True)
    assert out is x and out.grad_fn is not None
    out.backward(grad_out.to(DEV), retain_graph=retain)
    return e, f, out


def test_region_splice_gradients_vs_fp64_autograd():
    ids, emb, feats, grad_out = region_splice_case()
    ge, gf = region_splice_reference(ids, emb, feats, grad_out)
    e, f, out = region_splice_native(ids, emb, feats, grad_out)
    assert torch.equal(out.detach().cpu(), bf(T.region_splice(emb.float(), ids, REG, feats.float())))
    assert torch.equal(e.grad.cpu(), ge) and torch.equal(f.grad.cpu(), gf)
    assert bool((e.grad.cpu()[ids == REG] == 0).all()) and f.grad.dtype == BF
    e, f, _ = region_splice_native(ids, emb, feats, grad_out, need=(True, False))
    assert f.grad is None and torch.equal(e.grad.cpu(), ge)
    e, f, _ = region_splice_native(ids, emb, feats, grad_out, need=(False, True))
    assert e.grad is None and torch.equal(f.grad.cpu(), gf)
    e, f, _ = region_splice_native(ids, emb, feats, grad_out, feats_dtype=torch.float32)
    assert f.grad.dtype == torch.float32 and torch.equal(f.grad.cpu(), gf.float())
    leaf = emb.to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match="in-place"):
        S.splice_region_tokens(leaf, ids.to(DEV), REG, feats.to(DEV), native_backward=True)
    with torch.no_grad():                                               # no gradient needed: the plain path, no node
        plain = S.splice_region_tokens(emb.to(DEV), ids.to(DEV), REG, feats.to(DEV).requires_grad_(True), native_backward=True)
    assert plain.grad_fn is None
    assert S.splice_region_tokens(emb.to(DEV), ids.to(DEV), REG, feats.to(DEV), native_backward=True).grad_fn is None


# ---- 3: splice_emb_tokens ------------------------------------------------------------------------------------------------------------------
E0, NE, NG = 500, 8, 3
TOOLS = {450: "det", 451: "det", 453: "pose", 454: "gen"}


def emb_case(overlap=False):
    torch.manual_seed(3)
    B, L, C = 4, 120, 192
    ids = torch.randint(0, 400, (B, L))
    for b in range(B):
        for k, tid in enumerate(list(TOOLS)[: 1 + b]):
            p = 5 + 25 * k
            n = NG if TOOLS[tid] == "gen" else NE
            ids[b, p] = tid
            ids[b, p + 1: p + 1 + n] = E0 if TOOLS[tid] == "gen" else torch.arange(E0, E0 + n)
    if overlap:
        ids[1, 10] = 453                                # a pose block (rows 11..18) over the tail of sample 1's det block (rows 6..13)
    tabs = {"det": bf(torch.randn(NE, C)), "pose": bf(torch.randn(NE, C)), "gen": bf(torch.randn(NG, C))}
    return ids, bf(torch.randn(B, L, C)), tabs, bf(torch.randn(B, L, C))


def emb_reference(ids, emb, tabs, grad_out):
    """fp64 autograd of the oracle -> (ids, embeddings, grad embeddings, {table: (grad, sum |terms|, uses per row)})."""
    res = {}
    for what, g in (("grad", grad_out.double()), ("mag", grad_out.double().abs()), ("n", torch.ones_like(grad_out, dtype=torch.float64))):
        e = leaf64(emb)
        t64 = {k: leaf64(v) for k, v in tabs.items()}
        ids_out, out = T.emb_splice(ids, e, {tid: t64[k] for tid, k in TOOLS.items()}, E0, NE, NG, gen_tools=(454,))
        out.backward(g)
        res[what] = (e.grad, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in t64.items()})
    return ids_out, bf(out.detach()), bf(res["grad"][0]), {k: (res["grad"][1][k], res["mag"][1][k], res["n"][1][k]) for k in tabs}


def emb_native(ids, emb, tabs, grad_out, table_dtype=BF, retain=False):
    e, x = nonleaf(emb)
    t = {k: v.to(DEV).to(table_dtype).requires_grad_(True) for k, v in tabs.items()}
    ids_out, out = S.splice_emb_tokens(ids.to(DEV), x, {tid: t[k] for tid, k in TOOLS.items()}, E0, NE, NG, gen_tools=(454,), native_backward=True)
    assert out is x
    out.backward(grad_out.to(DEV), retain_graph=retain)
    return ids_out, out, e, t


@pytest.mark.parametrize("overlap", [False, True])
def test_emb_splice_gradients_vs_fp64_autograd(overlap):
    ids, emb, tabs, grad_out = emb_case(overlap)
    ids_ref, out_ref, ge, gt = emb_reference(ids, emb, tabs, grad_out)
    ids_out, out, e, t = emb_native(ids, emb, tabs, grad_out)
    assert torch.equal(ids_out.cpu(), ids_ref) and torch.equal(out.detach().cpu(), out_ref)      # the later tool wins in the forward
    assert torch.equal(e.grad.cpu(), ge)
    for k, (g64, mag, n) in gt.items():
        got = t[k].grad.cpu()                                                                    # det / seg share ONE table: one gradient
        assert got.dtype == BF and got.shape == g64.shape
        uses = n[:, 0]
        assert bool((n == uses[:, None]).all())
        once = uses == 1
        assert torch.equal(got[once], bf(g64[once]))
        if bool((~once).any()):
            assert_bound(got[~once], g64[~once], (uses[~once, None] - 1).clamp_min(0) * mag[~once], f"emb table {k}", rel_mag=2.0 ** -23)
    assert bool((gt["gen"][2] == 1).all()) and bool((gt["det"][2] >= 5).all())
    if overlap:
        assert gt["det"][2][:, 0].tolist() == [7.0] * 5 + [6.0] * 3 and bool((gt["pose"][2] == 3).all())
    # the forward is the default path's: the same ids and embeddings, bit for bit
    with torch.no_grad():
        ids_plain, out_plain = S.splice_emb_tokens(ids.to(DEV), emb.to(DEV).clone(), {tid: tabs[k].to(DEV) for tid, k in TOOLS.items()}, E0, NE,
                                                   NG, gen_tools=(454,))
    assert torch.equal(ids_plain, ids_out) and same_bits(out_plain, out.detach())


def test_emb_splice_fp32_tables_same_tool_overlap_and_the_plain_path():
    ids, emb, tabs, grad_out = emb_case()
    _, _, _, gt = emb_reference(ids, emb, tabs, grad_out)
    _, _, _, t32 = emb_native(ids, emb, tabs, grad_out, table_dtype=torch.float32)
    _, _, _, t16 = emb_native(ids, emb, tabs, grad_out)
    for k in tabs:                                                       # an fp32 parameter gets an fp32 gradient: the bf16 one, widened
        assert t32[k].grad.dtype == torch.float32 and torch.equal(t32[k].grad, t16[k].grad.float())
    close = ids.clone()
    close[0, 40], close[0, 45] = 450, 450                                # two det tokens closer than 8
    tables = {tid: tabs[k].to(DEV).requires_grad_(True) for tid, k in TOOLS.items()}
    with pytest.raises(RuntimeError, match="overlap"):
        S.splice_emb_tokens(close.to(DEV), emb.to(DEV).clone(), tables, E0, NE, NG, gen_tools=(454,), native_backward=True)
    with torch.no_grad():
        _, out = S.splice_emb_tokens(ids.to(DEV), emb.to(DEV).clone(), tables, E0, NE, NG, gen_tools=(454,), native_backward=True)
    assert out.grad_fn is None


# ---- 4: gather_emb_hidden_states -------------------------------------------------------------------------------------------------------------
def text_query_case():
    torch.manual_seed(5)
    B, L, C, ne, e0 = 6, 300, 256, 4, 900
    ids = torch.randint(0, 800, (B, L))
    for b in range(B):
        for k in range(b % 6):
            p = 10 + 40 * k + b
            ids[b, p:p + ne] = torch.arange(e0, e0 + ne)
    ids[0, 0] = e0                                       # sample 0: ONLY a stray token -- skipped by the reference (:783-786)
    return ids, bf(torch.randn(B, L, C)), ne, e0


def text_query_native(ids, hs, ne, e0, grad_out, retain=False):
    h = hs.to(DEV).requires_grad_(True)
    tq, masks = S.gather_emb_hidden_states(h, ids.to(DEV), e0, ne, native_backward=True)
    tq.backward(grad_out.to(DEV), retain_graph=retain)
    return h, tq, masks


def test_text_query_gradient_vs_fp64_autograd():
    ids, hs, ne, e0 = text_query_case()
    h64 = leaf64(hs)
    ref, ref_masks = T.text_query(h64, ids, e0, ne)
    grad_out = bf(torch.randn(ref.shape))
    ref.backward(grad_out.double())
    h, tq, masks = text_query_native(ids, hs, ne, e0, grad_out)
    assert tq.grad_fn is not None and torch.equal(tq.detach().cpu(), bf(ref.detach())) and torch.equal(masks.cpu(), ref_masks)
    assert torch.equal(h.grad.cpu(), bf(h64.grad))
    kept = (ids >= e0) & (ids <= e0 + ne - 1)
    kept[0] = False
    assert torch.equal(bits(h.grad.cpu()[~kept]), torch.zeros_like(bits(hs[~kept])))            # exactly zero, the stray token's row too
    assert bool((h.grad.cpu()[kept] != 0).any())
    hg = hs.to(DEV).requires_grad_(True)
    assert S.gather_emb_hidden_states(hg, torch.zeros_like(ids).to(DEV), e0, ne, native_backward=True) == (None, None)
    bad = ids.clone()
    bad[1, 0] = e0                                       # whole patches + a stray token: the reference's reshape fails
    with pytest.raises(RuntimeError, match="not a whole number of patches"):
        S.gather_emb_hidden_states(hg, bad.to(DEV), e0, ne, native_backward=True)
    plain, _ = S.gather_emb_hidden_states(hs.to(DEV), ids.to(DEV), e0, ne, native_backward=True)
    assert plain.grad_fn is None and same_bits(plain, tq.detach())


# ---- 5: gather_region_image_features ---------------------------------------------------------------------------------------------------------
def region_feature_cases():
    torch.manual_seed(9)
    split_sizes, num_regions = [5, 1, 3], [2, 0, 3]
    yield "anyres", [bf(torch.randn(sum(split_sizes), 1 + 16, 128)) for _ in range(4)], split_sizes, num_regions, None
    from test_oracle_tokens import _region_case
    g = load_golden("region_branch.npz")
    for tag in ("mmic", "pad"):
        hs, _, split_sizes, num_regions, num_splits = _region_case(g, tag)
        yield tag, [bf(h) for h in hs], split_sizes, num_regions, num_splits


def region_feature_reference(hs, split_sizes, num_regions, num_splits, grads):
    h64 = [leaf64(h) for h in hs]
    outs = T.region_features(h64, split_sizes, num_regions, num_splits=num_splits)
    torch.autograd.backward(outs, [g.double() for g in grads])
    return outs, [h.grad for h in h64]


def region_feature_native(hs, split_sizes, num_regions, num_splits, grads, need=None, retain=False):
    need = need or [True] * len(hs)
    h = [x.to(DEV).requires_grad_(r) for x, r in zip(hs, need)]
    outs = S.gather_region_image_features(h, split_sizes, num_regions, num_splits=num_splits, native_backward=True)
    torch.autograd.backward(outs, [g.to(DEV) for g in grads], retain_graph=retain)
    return h, outs


def test_region_feature_gradients_vs_fp64_autograd():
    for tag, hs, split_sizes, num_regions, num_splits in region_feature_cases():
        tiles = S.region_tile_index(split_sizes, num_regions, num_splits, n_images=hs[0].shape[0])
        shape = (len(tiles),) + tuple(hs[-1][:, 1:].shape[1:])
        gen = torch.Generator().manual_seed(1)
        for integer in (True, False):
            grads = [bf(torch.randint(-8, 9, shape, generator=gen).float() if integer else torch.randn(shape, generator=gen)) for _ in range(3)]
            outs_ref, g64 = region_feature_reference(hs, split_sizes, num_regions, num_splits, grads)
            _, mag = region_feature_reference(hs, split_sizes, num_regions, num_splits, [g.abs() for g in grads])
            _, n = region_feature_reference(hs, split_sizes, num_regions, num_splits, [torch.ones_like(g) for g in grads])
            h, outs = region_feature_native(hs, split_sizes, num_regions, num_splits, grads)
            assert all(torch.equal(o.detach().cpu(), bf(r.detach())) for o, r in zip(outs, outs_ref)), tag
            assert h[0].grad is None and g64[0] is None                                          # only the last three levels are read
            for lv in range(len(hs) - 3, len(hs)):
                got = h[lv].grad.cpu()
                unread = [t for t in range(hs[lv].shape[0]) if t not in tiles]
                assert torch.equal(bits(got[:, 0]), torch.zeros_like(bits(got[:, 0]))), (tag, lv)       # CLS rows
                assert torch.equal(bits(got[unread]), torch.zeros_like(bits(got[unread]))), (tag, lv)   # tiles no region reads
                if integer:
                    assert torch.equal(got, bf(g64[lv])), (tag, lv)
                else:
                    assert_bound(got, g64[lv], (n[lv] - 1).clamp_min(0) * mag[lv], f"region features {tag} level {lv}", rel_mag=2.0 ** -23)
            if tag == "anyres":                                                                  # tiles shared by 2 and by 3 regions
                assert n[1][4, 1:].unique().tolist() == [2.0] and n[1][8, 1:].unique().tolist() == [3.0]


def test_region_feature_levels_without_grad_and_one_tensor_for_all_levels():
    _, hs, split_sizes, num_regions, num_splits = next(region_feature_cases())
    shape = (sum(num_regions), 16, 128)
    gen = torch.Generator().manual_seed(2)
    grads = [bf(torch.randint(-8, 9, shape, generator=gen).float()) for _ in range(3)]
    h = [x.to(DEV).requires_grad_(r) for x, r in zip(hs, (True, True, False, True))]
    outs = S.gather_region_image_features(h, split_sizes, num_regions, native_backward=True)
    assert outs[0].grad_fn is not None and outs[1].grad_fn is None and outs[2].grad_fn is not None
    # the same tensor at all three levels: three gradients accumulate (integer-valued, so every partial sum is exact)
    one = hs[0].to(DEV).requires_grad_(True)
    outs = S.gather_region_image_features([one] * 3, split_sizes, num_regions, native_backward=True)
    torch.autograd.backward(outs, [g.to(DEV) for g in grads])
    o64 = leaf64(hs[0])
    torch.autograd.backward(T.region_features([o64] * 3, split_sizes, num_regions), [g.double() for g in grads])
    assert torch.equal(one.grad.cpu(), bf(o64.grad))


# ---- 6 and 7: offset views, a caller stream, a second backward through a retained graph ----------------------------------------------------
def test_offset_views_and_a_caller_stream():
    side = torch.cuda.Stream(device=DEV)
    off = 4                                                             # bytes: a storage offset of 2 elements
    ids, emb, feats, grad_out = region_splice_case()
    e0, f0, out0 = region_splice_native(ids, emb, feats, grad_out)
    eids, eemb, tabs, egrad = emb_case()
    _, eout0, ee0, et0 = emb_native(eids, eemb, tabs, egrad)
    tids, ths, ne, e0_id = text_query_case()
    tgrad = bf(torch.randn(6, 5, ne, 256))
    th0, tq0, _ = text_query_native(tids, ths, ne, e0_id, tgrad)
    _, rhs, split_sizes, num_regions, _ = next(region_feature_cases())
    rgrads = [bf(torch.randn(sum(num_regions), 16, 128)) for _ in range(3)]
    rh0, routs0 = region_feature_native(rhs, split_sizes, num_regions, None, rgrads)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        e = emb.to(DEV).requires_grad_(True)
        f = feats.to(DEV).requires_grad_(True)
        x = offset_view(e, off, True)
        assert x.data_ptr() % 16 != 0
        out = S.splice_region_tokens(x, ids.to(DEV), REG, offset_view(f, off, True), native_backward=True)
        assert out is x
        out.backward(offset_view(grad_out.to(DEV), off, False))
        assert same_bits(out.detach(), out0.detach()) and same_bits(e.grad, e0.grad) and same_bits(f.grad, f0.grad)

        ee = eemb.to(DEV).requires_grad_(True)
        t = {k: v.to(DEV).requires_grad_(True) for k, v in tabs.items()}
        x = offset_view(ee, off, True)
        _, out = S.splice_emb_tokens(eids.to(DEV), x, {tid: offset_view(t[k], off, True) if k == "pose" else t[k] for tid, k in TOOLS.items()}, E0,
                                     NE, NG, gen_tools=(454,), native_backward=True)
        out.backward(offset_view(egrad.to(DEV), off, False))
        assert same_bits(out.detach(), eout0.detach()) and same_bits(ee.grad, ee0.grad)
        assert all(same_bits(t[k].grad, et0[k].grad) for k in tabs)

        th = ths.to(DEV).requires_grad_(True)
        tq, _ = S.gather_emb_hidden_states(offset_view(th, off, True), tids.to(DEV), e0_id, ne, native_backward=True)
        tq.backward(offset_view(tgrad.to(DEV), off, False))
        assert same_bits(tq.detach(), tq0.detach()) and same_bits(th.grad, th0.grad)

        rh = [h.to(DEV).requires_grad_(True) for h in rhs]
        routs = S.gather_region_image_features([offset_view(h, off, True) for h in rh], split_sizes, num_regions, native_backward=True)
        torch.autograd.backward(routs, [offset_view(g.to(DEV), off, False) for g in rgrads])
        assert all(same_bits(a.detach(), b.detach()) for a, b in zip(routs, routs0))
        assert all(same_bits(rh[lv].grad, rh0[lv].grad) for lv in (1, 2, 3))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def test_a_second_backward_through_a_retained_graph_gives_the_same_bits():
    def twice(leaves, outs, grads):
        torch.autograd.backward(outs, grads, retain_graph=True)
        first = [x.grad.clone() for x in leaves]
        for x in leaves:
            x.grad = None
        torch.autograd.backward(outs, grads)
        assert all(same_bits(a, x.grad) for a, x in zip(first, leaves))

    ids, emb, feats, grad_out = region_splice_case()
    e, x = nonleaf(emb)
    f = feats.to(DEV).requires_grad_(True)
    twice([e, f], [S.splice_region_tokens(x, ids.to(DEV), REG, f, native_backward=True)], [grad_out.to(DEV)])
    eids, eemb, tabs, egrad = emb_case()
    e, x = nonleaf(eemb)
    t = {k: v.to(DEV).requires_grad_(True) for k, v in tabs.items()}
    _, out = S.splice_emb_tokens(eids.to(DEV), x, {tid: t[k] for tid, k in TOOLS.items()}, E0, NE, NG, gen_tools=(454,), native_backward=True)
    twice([e, *t.values()], [out], [egrad.to(DEV)])
    tids, ths, ne, e0_id = text_query_case()
    h = ths.to(DEV).requires_grad_(True)
    tq, _ = S.gather_emb_hidden_states(h, tids.to(DEV), e0_id, ne, native_backward=True)
    twice([h], [tq], [bf(torch.randn(tq.shape)).to(DEV)])
    _, rhs, split_sizes, num_regions, _ = next(region_feature_cases())
    rh = [x.to(DEV).requires_grad_(True) for x in rhs[1:]]
    routs = S.gather_region_image_features(rh, split_sizes, num_regions, native_backward=True)
    twice(rh, routs, [bf(torch.randn(o.shape)).to(DEV) for o in routs])


# ---- 8: end to end: tower levels -> region features -> region encoder -> <region> slots -> loss ----------------------------------------------
def test_end_to_end_region_branch_against_the_composed_chain(monkeypatch):
    """RegionEncoder with native_branch between the two region token loops, all with native_backward=True, against the same modules with
    the switch off and torch indexing in place of the two functions -- each measured against an fp64 CPU run of the composed chain with
    the same (replayed) sample points.  The tolerance is tests/test_region_stem_gpu.py's for the module against its composed form:
    native's relative rms error at most 1.25 x the composed chain's, per output, per parameter and per hidden-state leaf."""
    import test_region_stem_gpu as RS
    from visionllm_amd import region_encoder as A
    images, masks, _, _ = RS._module_inputs()                          # 3 regions of 56 x 84
    split_sizes, num_regions = [2, 1], [2, 1]                          # regions 0, 1 read tile 1, region 2 reads tile 2, tile 0 is unread
    tiles = S.region_tile_index(split_sizes, num_regions)
    gen = torch.Generator().manual_seed(11)
    hidden = [bf(torch.randn(3, 1 + 24, RS.EMB, generator=gen)) for _ in range(3)]
    B, L = 2, 12
    ids = torch.randint(100, 200, (B, L), generator=gen)
    ids[0, 2] = ids[0, 7] = ids[1, 5] = REG
    emb = bf(torch.randn(B, L, RS.OUT, generator=gen))

    def step(enc, native, device, dtype):
        enc.zero_grad(set_to_none=True)
        hid = [t.to(device).to(dtype).requires_grad_(True) for t in hidden]
        e = emb.to(device).to(dtype).requires_grad_(True)
        ids_d = ids.to(device)
        torch.manual_seed(1)
        if native:
            feats = S.gather_region_image_features(hid, split_sizes, num_regions, native_backward=True)
            x = S.splice_region_tokens(e * 1, ids_d, REG, enc(images, masks, feats), native_backward=True)
        else:
            feats = [h[tiles][:, 1:] for h in hid]
            x = e * 1
            x[ids_d == REG] = enc(images.to(device).to(dtype), masks.to(device).to(dtype), feats).to(dtype)
        (x if dtype == torch.float64 else x.float()).pow(2).sum().backward()
        res = {"out": x.detach(), "emb": e.grad}
        res.update({f"level{i}": h.grad for i, h in enumerate(hid)})
        res.update({k: p.grad for k, p in enc.named_parameters()})
        assert all(v is not None for v in res.values()), [k for k, v in res.items() if v is None]
        return {k: v.detach().clone() for k, v in res.items()}

    enc = RS._encoder(native=True)
    recorded, real = [], A.rand_sample

    def record(x, divisor, max_len):
        recorded.append(real(x, divisor, max_len))
        return recorded[-1]

    monkeypatch.setattr(A, "rand_sample", record)
    native = step(enc, True, DEV, BF)
    points = list(recorded)

    def replay_on(device):
        it = iter(points)
        return lambda x, divisor, max_len: next(it).to(device)

    off = RS._encoder(native=False)
    off.load_state_dict(enc.state_dict())
    monkeypatch.setattr(A, "rand_sample", replay_on(DEV))
    composed = step(off, False, DEV, BF)
    twin = RS.TR._TwinEncoder(hidden_dim=RS.HID, embed_dim=RS.EMB, out_dim=RS.OUT, patch_size=14, mask_pool_type="grid_sample")
    twin.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    twin = twin.double().train()
    twin.num_points = RS.NPTS
    monkeypatch.setattr(A, "rand_sample", replay_on("cpu"))
    ref = step(twin, False, "cpu", torch.float64)
    assert sorted(native) == sorted(ref) == sorted(composed) and len(ref) == 12 + 5
    worse = []
    for k in sorted(ref):
        assert native[k].dtype == BF and native[k].shape == ref[k].shape and bool(torch.isfinite(native[k].float()).all()), k
        en, eo = rel_rms(native[k].cpu(), ref[k]), rel_rms(composed[k].cpu(), ref[k])
        print(f"region branch {k}: native {en:.4g}  composed {eo:.4g}  ratio {en / max(eo, 1e-300):.3f}")
        if not en <= 1.25 * eo:
            worse.append((k, en, eo))
    assert not worse, worse
    for i in range(3):                                                 # CLS rows and the unread tile: exactly zero
        assert bool((native[f"level{i}"][:, 0] == 0).all()) and bool((native[f"level{i}"][0] == 0).all())
