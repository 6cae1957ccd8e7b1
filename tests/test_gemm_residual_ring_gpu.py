"""Persistent GEMM, residual epilogue without LayerScale: the residual tile rides the operand ring as two virtual K tiles and is added by
MFMAs against an identity fragment (gemm256p.hip, RING; option "gemm_res_ring").  y = (x W^T + res) + b with one rounding; the epilogue
route (option 0) computes (x W^T + b) + res: the same terms in another fp32 order.

Shapes: at least 256 tiles each (the persistent schedule needs as many tiles as CUs), K as short as the schedule takes -- every case
runs in well under a second.  Bounds: the ones test_gemm256_persistent_residual / test_gemm_folded_norm use; nothing here is measured
from the kernel under test."""
import functools
import math

import pytest
import torch

from bounds import P, assert_bound, stream
from visionllm_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 7.0

#        M      N     K   tile   pad
CASES = [
    (16500, 1024, 128, 0x300, 0),     # nk = 2 (virtual K tile 0 is requested from the tile's K tile 0), 192-row tiles
    (16700, 1024, 192, 0x200, 64),    # odd nk (stage parity across the seam), strided X / W / Y / res with ldr != ldx
    (70001, 256, 128, 0x200, 0),      # one column tile, ragged last row tile
    (20000, 1096, 128, 0x200, 16),    # last column tile 72 wide (its last 32-column group reaches into the padding), no statistics
]
IDS = [f"M{c[0]}_N{c[1]}_K{c[2]}_{c[3]:#x}_pad{c[4]}" for c in CASES]


def bf(t):
    return t.to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


def gemm(c, x, w, b, res, ring, y=None, ldr=None):
    """One launch of the residual GEMM on the persistent schedule (asserted) with the ring route on / off -> the whole output buffer."""
    M, N, K, force, pad = c
    L = _lib.lib()
    if y is None:
        y = torch.full((M + 300, N + pad), CANARY, dtype=torch.bfloat16, device=DEV)   # canary rows (a whole tile's worth) and columns
    before = L.vllm_gemm_persistent_launches()
    old = _lib.set_option("gemm_res_ring", ring)
    try:
        _lib.check(L.vllm_gemm_bf16(P(x), P(w), P(b) if b is not None else None, P(y), M, N, K, K + pad, K + pad, N + pad, 3 | force, None,
                                    P(res), N + pad if ldr is None else ldr, 0, stream()))
    finally:
        _lib.set_option("gemm_res_ring", old)
    torch.cuda.synchronize()
    assert L.vllm_gemm_persistent_launches() - before == 1, "the persistent schedule was not taken"
    return y


@functools.lru_cache(maxsize=None)
def clean(i):
    """Random operands of case i, the ring route's output and the fp64 reference of the first, middle and last 300 rows (computed once)."""
    M, N, K, force, pad = c = CASES[i]
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    x = bf(torch.randn(M, K + pad, device=DEV, generator=g))
    w = bf(torch.randn(N, K + pad, device=DEV, generator=g) / math.sqrt(K))
    b = bf(torch.randn(N, device=DEV, generator=g))
    res = bf(torch.randn(M, N + pad, device=DEV, generator=g))
    y = gemm(c, x, w, b, res, 1)
    ye = gemm(c, x, w, b, res, 0)
    rows = torch.cat([torch.arange(0, 300), torch.arange(M // 2, M // 2 + 300), torch.arange(M - 300, M)]).to(DEV)
    z = x[rows, :K].double() @ w[:, :K].double().t() + b.double() + res[rows, :N].double()
    mag = x[rows, :K].double().abs() @ w[:, :K].double().abs().t() + b.double().abs() + res[rows, :N].double().abs()
    return dict(x=x, w=w, b=b, res=res, y=y, ye=ye, rows=rows, z=z, mag=mag)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_mapping_exact(i):
    """W = 0, bias = 0: the output IS the residual, bit for bit -- a swapped lane, k step, slot or column group fails here."""
    M, N, K, force, pad = c = CASES[i]
    g = torch.Generator(device=DEV).manual_seed(i)
    x = bf(torch.randn(M, K + pad, device=DEV, generator=g))
    w = torch.zeros(N, K + pad, dtype=torch.bfloat16, device=DEV)
    b = torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    # nonzero finite bf16 values over 41 binades, every significand, both signs (normal numbers only)
    shape = (M, N + pad)
    e = torch.randint(-20, 21, shape, device=DEV, generator=g).double()
    m = 1.0 + torch.randint(0, 128, shape, device=DEV, generator=g).double() / 128.0
    sgn = torch.randint(0, 2, shape, device=DEV, generator=g).double() * 2.0 - 1.0
    res = (sgn * m * torch.pow(2.0, e)).to(torch.bfloat16)
    assert torch.isfinite(res.float()).all() and (res != 0).all()
    spoiled = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    if pad:
        # "nothing beyond column N of a row is read": what follows a row's N elements in memory is NaN -- the row's padding, and the
        # first 8 columns of the next row, which lie inside the reach of the row's last 32-column group when N + pad is short of it
        # (N = 1096, row stride 1112: the group 1088 .. 1119).  A NaN that came in would spoil the group (0 x NaN).  The rows whose
        # own first columns are NaN may have their first group spoiled, by the contract: those 32 elements are left out.
        res[:, N:] = float("nan")
        for r in (101, M // 2 + 1, M - 1):
            res[r, :8] = float("nan")
            spoiled[r, :32] = True
    y0 = gemm(c, x, w, b, res, 1)
    y1 = gemm(c, x, w, b, res, 1)
    assert torch.equal(bits(y0), bits(y1)), "ring route: run-to-run difference"
    assert (y0[M:] == CANARY).all() and (y0[:, N:] == CANARY).all(), "wrote outside the output block"
    bad = (bits(y0[:M, :N]) != bits(res[:, :N])) & ~spoiled
    assert not bad.any(), f"{int(bad.sum())} elements are not their residual's bits; first at {bad.nonzero()[0].tolist()}"
    if pad:
        assert torch.isnan(y0[:M, :N][spoiled].float()).all(), "the ring route was not taken: 0 x NaN must spoil a NaN's 32-column group"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_accuracy_both_routes(i):
    """Random operands against fp64 (first, middle and last 300 rows): the ring route and the epilogue route meet the same bound and
    differ in fewer than 5 % of the elements (fp32-ulp flips at bf16 ties: the cap the existing test puts on persistent against
    tile-wise, which differ the same way)."""
    M, N, K, force, pad = c = CASES[i]
    d = clean(i)
    y = d["y"]
    assert (y[M:] == CANARY).all() and (y[:, N:] == CANARY).all(), "wrote outside the output block"
    assert torch.equal(bits(y), bits(gemm(c, d["x"], d["w"], d["b"], d["res"], 1))), "ring route: run-to-run difference"
    ye = d["ye"]
    assert (ye[M:] == CANARY).all() and (ye[:, N:] == CANARY).all(), "epilogue route wrote outside the output block"
    assert_bound(y[d["rows"], :N], d["z"], d["mag"], f"ring route {IDS[i]}")
    assert_bound(ye[d["rows"], :N], d["z"], d["mag"], f"epilogue route {IDS[i]}")
    share = (y[:M, :N] != ye[:M, :N]).float().mean().item()
    print(f"{IDS[i]}: the routes differ in {share:.5f} of the elements")
    assert share < 0.05


@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_statistics(i, rms):
    """Folded norm, producer side, on the ring route: {mean, M2} ({sum of squares, -}) per row and 256-column tile against the same
    moments recomputed in fp64 from the stored bf16 output, at test_gemm_folded_norm's tolerances."""
    M, N, K, force, pad = CASES[i]
    L = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(100 + i + rms)
    x = bf(torch.randn(M, K + pad, device=DEV, generator=g))
    w = bf(torch.randn(N, K + pad, device=DEV, generator=g) / math.sqrt(K))
    b = bf(torch.randn(N, device=DEV, generator=g) + 0.5)
    res = bf(torch.randn(M, N + pad, device=DEV, generator=g) * 2.0 + 0.75)
    res[:, 7] += 40.0                                    # an outlier channel, as residual streams have
    nt = N // 256
    outs = []
    before = L.vllm_gemm_persistent_launches()
    for _ in range(2):
        h = torch.full((M + 300, N + pad), CANARY, dtype=torch.bfloat16, device=DEV)
        stats = torch.full((M, nt, 2), float("nan"), dtype=torch.float32, device=DEV)
        _lib.check(L.vllm_gemm_bf16_ln(P(x), P(w), P(b), P(h), M, N, K, K + pad, K + pad, N + pad, 3 | force, None, P(res), N + pad,
                                       P(stats), None, 0, rms, 1e-5, None, None, stream()))
        outs.append((h, stats))
    torch.cuda.synchronize()
    assert L.vllm_gemm_persistent_launches() - before == 2, "the persistent schedule was not taken"
    (h, stats), (h2, stats2) = outs
    assert torch.equal(bits(h), bits(h2)) and torch.equal(stats, stats2), "run-to-run difference"
    assert (h[M:] == CANARY).all() and (h[:, N:] == CANARY).all(), "wrote outside the output block"
    rows = torch.cat([torch.arange(0, 300), torch.arange(M - 300, M)]).to(DEV)
    z = x[rows, :K].double() @ w[:, :K].double().t() + b.double() + res[rows, :N].double()
    mag = x[rows, :K].double().abs() @ w[:, :K].double().abs().t() + b.double().abs() + res[rows, :N].double().abs()
    assert_bound(h[rows, :N], z, mag, f"ring route with statistics {IDS[i]} rms={rms}")
    hd = h[:M, :N].double()
    for tcol in range(nt):
        blk = hd[:, tcol * 256:(tcol + 1) * 256]
        if rms:
            torch.testing.assert_close(stats[:, tcol, 0].double(), (blk * blk).sum(1), rtol=2e-6, atol=1e-6)
        else:
            torch.testing.assert_close(stats[:, tcol, 0].double(), blk.mean(1), rtol=2e-6, atol=2e-6)
            torch.testing.assert_close(stats[:, tcol, 1].double(), ((blk - blk.mean(1, keepdim=True)) ** 2).sum(1), rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_in_place(i):
    """res == Y: a tile's residual has been consumed by the matrix pipe before the tile's first store goes out."""
    M, N, K, force, pad = c = CASES[i]
    d = clean(i)
    y = torch.full((M + 300, N + pad), CANARY, dtype=torch.bfloat16, device=DEV)
    y[:M] = d["res"]
    gemm(c, d["x"], d["w"], d["b"], y, 1, y=y)
    assert torch.equal(bits(y[:M, :N]), bits(d["y"][:M, :N])), "in place differs from out of place"
    assert (y[M:] == CANARY).all() and torch.equal(bits(y[:M, N:]), bits(d["res"][:, N:])), "wrote outside the output block"


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_nonfinite_containment(i):
    """0 x Inf is NaN in the identity product: a non-finite residual element may spoil its row's aligned 32-column group (the documented
    contract), and nothing else -- every other output equals the clean run bit for bit.  The same two elements tell the routes apart:
    with the option on the groups' other elements ARE NaN, with it off only the two elements themselves change."""
    M, N, K, force, pad = c = CASES[i]
    d = clean(i)
    res = d["res"].clone()
    spots = [(200, 5, float("inf")), (M - 1, N - 1, float("nan"))]   # inside the first tiles; last row of the ragged row tile, last column
    allowed = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    for r, col, v in spots:
        res[r, col] = v
        allowed[r, (col // 32) * 32:min(N, (col // 32) * 32 + 32)] = True
    own = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    for r, col, _ in spots:
        own[r, col] = True
    y = gemm(c, d["x"], d["w"], d["b"], res, 1)
    for r, col, _ in spots:
        assert not torch.isfinite(y[r, col].float()), "the non-finite element itself must come out non-finite"
    diff = (bits(y[:M, :N]) != bits(d["y"][:M, :N])) & ~allowed
    assert not diff.any(), f"{int(diff.sum())} outputs outside the 32-column groups changed; first at {diff.nonzero()[0].tolist()}"
    assert (y[M:] == CANARY).all() and (y[:, N:] == CANARY).all(), "wrote outside the output block"
    # which kernel ran: on the matrix pipe the group's other elements are 0 x Inf / 0 x NaN = NaN; the epilogue route adds element
    # by element, so there only the two elements themselves differ from its clean run
    assert torch.isnan(y[:M, :N][allowed & ~own].float()).all(), "option 1 did not take the ring route: the groups' other elements are not NaN"
    ye = gemm(c, d["x"], d["w"], d["b"], res, 0)
    for r, col, _ in spots:
        assert not torch.isfinite(ye[r, col].float()), "epilogue route: the non-finite element itself must come out non-finite"
    diff = (bits(ye[:M, :N]) != bits(d["ye"][:M, :N])) & ~own
    assert not diff.any(), f"option 0 did not take the epilogue route: {int(diff.sum())} other outputs changed; first at {diff.nonzero()[0].tolist()}"
    assert (ye[M:] == CANARY).all() and (ye[:, N:] == CANARY).all(), "epilogue route wrote outside the output block"


@pytest.mark.parametrize("ring", [1, 0])
def test_statistics_wide_ragged(ring):
    """Wide statistics (RMSNorm, a row of other than four column tiles: [M][16] sums of squares) with a ragged last column tile, on
    both routes: slot s against the sum of squares of the stored bf16 values of column tile s in fp64, test_gemm_folded_norm's
    tolerance; the last tile is 72 wide (its pieces beyond N count nothing), slots >= 5 stay as the caller cleared them."""
    M, N, K, force, pad = CASES[3]
    L = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(300)
    x = bf(torch.randn(M, K + pad, device=DEV, generator=g))
    w = bf(torch.randn(N, K + pad, device=DEV, generator=g) / math.sqrt(K))
    b = bf(torch.randn(N, device=DEV, generator=g) + 0.5)
    res = bf(torch.randn(M, N + pad, device=DEV, generator=g) * 2.0 + 0.75)
    res[:, N:] = 1000.0                                  # what lies behind a row must not be counted
    nt = (N + 255) // 256
    assert nt == 5 and N % 256 == 72
    h = torch.full((M + 300, N + pad), CANARY, dtype=torch.bfloat16, device=DEV)
    stats = torch.zeros(M, 16, dtype=torch.float32, device=DEV)
    before = L.vllm_gemm_persistent_launches()
    old = _lib.set_option("gemm_res_ring", ring)
    try:
        _lib.check(L.vllm_gemm_bf16_ln(P(x), P(w), P(b), P(h), M, N, K, K + pad, K + pad, N + pad, 3 | force, None, P(res), N + pad,
                                       P(stats), None, nt, 1, 1e-5, None, None, stream()))
    finally:
        _lib.set_option("gemm_res_ring", old)
    torch.cuda.synchronize()
    assert L.vllm_gemm_persistent_launches() - before == 1, "the persistent schedule was not taken"
    assert (h[M:] == CANARY).all() and (h[:, N:] == CANARY).all(), "wrote outside the output block"
    rows = torch.cat([torch.arange(0, 300), torch.arange(M - 300, M)]).to(DEV)
    z = x[rows, :K].double() @ w[:, :K].double().t() + b.double() + res[rows, :N].double()
    mag = x[rows, :K].double().abs() @ w[:, :K].double().abs().t() + b.double().abs() + res[rows, :N].double().abs()
    assert_bound(h[rows, :N], z, mag, f"wide statistics, ring={ring}")
    hd = h[:M, :N].double()
    for tcol in range(nt):
        blk = hd[:, tcol * 256:min(N, (tcol + 1) * 256)]
        torch.testing.assert_close(stats[:, tcol].double(), (blk * blk).sum(1), rtol=2e-6, atol=1e-6)
    assert (stats[:, nt:] == 0).all(), "a slot beyond the row's column tiles was written"


def test_residual_rows_not_16_byte_aligned_keep_the_epilogue_route():
    """ldr = 4 (mod 8): the residual's rows are 8-byte aligned.  The epilogue's register loads take that; the ring's 16-byte LDS-DMA
    reads, like those of X and W, want 16-byte aligned rows -- such a call stays on the persistent schedule and on the epilogue route,
    whatever the option says: same bits as with the option off, and an Inf stays in its own element."""
    M, N, K, force, pad = c = CASES[0]
    d = clean(0)
    ldr = N + 4
    res = torch.zeros(M, ldr, dtype=torch.bfloat16, device=DEV)
    res[:, :N] = d["res"][:, :N]
    res[:, N:] = float("nan")
    y1 = gemm(c, d["x"], d["w"], d["b"], res, 1, ldr=ldr)
    y0 = gemm(c, d["x"], d["w"], d["b"], res, 0, ldr=ldr)
    assert torch.equal(bits(y1), bits(y0)) and torch.equal(bits(y1), bits(d["ye"])), "not the epilogue route's bits"
    res[200, 5] = float("inf")
    y = gemm(c, d["x"], d["w"], d["b"], res, 1, ldr=ldr)
    diff = bits(y[:M, :N]) != bits(d["ye"][:M, :N])
    assert diff[200, 5] and int(diff.sum()) == 1, "an Inf spread beyond its own element: the ring route was taken"
