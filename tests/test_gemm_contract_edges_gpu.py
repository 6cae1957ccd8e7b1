"""The vllm_gemm_bf16* entries at the minimums include/vllm_hip.h documents: N % 4 == 0 (not 8), ldy % 4 == 0, ldr % 4 == 0, Y / bias /
scale / res / pre 8-byte (not 16-byte) aligned, M below one MFMA fragment, N below one tile -- on every kernel behind the entry (forced
128 x 128, 8-phase with 256- / 192-row tiles, 8-phase on the 32x32x16 instruction, automatic) and under every public epilogue.  There the
128 x 128 and the tile-wise 8-phase kernels leave their row-wise LDS epilogue and store 8-byte pairs straight from the accumulator
layout, the residual no longer enters as the accumulators' initial value, and the persistent schedule's 16-byte stores land on rows
that are only 8-byte aligned.

The reference is fp64 on the bf16-rounded operands, never another route of the library.  Bounds are the project's own (bounds.py, the
GEMM tests of test_vit_gpu.py): bf16 outputs 1 bf16 ulp(ref) + 2^-17 sum|terms| (2^-16 for LayerScale + residual on the tile-wise
8-phase kernels, as test_gemm256_persistent_residual: the res / ls * ls round trip), fp32 outputs 2^-17 sum|terms| and no rounding
term, GELU-backward the factor 1.2 on the magnitude (test_gelu_bwd_epilogue_against_fp64).  Every output buffer is filled with a NaN
of a bit pattern no arithmetic produces (a canary the result cannot take, a NaN the kernel wrote included), with ldy - N padding columns
and 16 (persistent shapes: 300) rows behind M: every element of the block must come out finite, everything else must keep the canary's
bits.  What lies behind K in a row of X / W and behind N in a row of res / the position table is NaN too: read, it would spoil the
result.

No call here hands in a pointer below the contract: every offset is 8 bytes (bf16 operands) or 0."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from bounds import P, assert_bound, stream
from test_bridge_train_gpu import gelu_grad64
from visionllm_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CANARY = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5}   # NaNs with a payload: neither the default NaN nor one made from it
PATCH = 7                    # patches per image of the embed epilogue: several images (and CLS slots) from M = 15 on, a partial last image
ROUTES = [0x100, 0x200, 0x300, 0x800, 0]
ROUTE_IDS = [f"{r:#x}" if r else "auto" for r in ROUTES]
#        name -> epilogue number (the residual-save forms go through vllm_gemm_bf16_residual_save)
EPI = {"bias": 0, "gelu": 1, "quick_gelu": 2, "residual": 3, "residual_ls": 3, "embed": 4, "f32": 5, "f32_mask": 5, "gelu_bwd": 6,
       "save": 3, "save_ls": 3}
# every M in {1, 15, 17, 129, 193, 257} (below one fragment, one row past each tile height), every N in {4, 12, 68, 132, 260} (N = 4
# mod 8; below one fragment, one 128-wide and one 256-wide tile) and both K at least twice
SMALL = [(1, 4, 64), (15, 12, 192), (17, 68, 64), (129, 132, 192), (193, 260, 64), (257, 4, 192),
         (1, 260, 192), (15, 132, 64), (17, 260, 192), (129, 12, 64), (193, 68, 192), (257, 132, 64)]
ROWS8 = [(300, 256, 128), (1100, 1024, 128)]


def bf(t):
    return t.to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def canaries(n, dtype):
    return torch.full((n,), CANARY[dtype], dtype=torch.int16 if dtype == torch.bfloat16 else torch.int32, device=DEV).view(dtype)


def intact(t):
    return bool((bits(t) == CANARY[t.dtype]).all())


def placed(t, off, ld=None):
    """`t` (1-D, or 2-D with row stride `ld`) as a view `off` elements into a fresh NaN-filled allocation; row padding is NaN."""
    rows, cols = (1, t.numel()) if t.dim() == 1 else t.shape
    ld = cols if ld is None else ld
    flat = torch.full((off + rows * ld,), NAN, dtype=t.dtype, device=DEV)
    v = flat[off:].view(rows, ld)
    v[:, :cols] = t.view(rows, cols)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16 and (off * t.element_size()) % 8 == 0
    return v[0, :cols] if t.dim() == 1 else v


def eight_phase(route, M, N):
    return route in (0x200, 0x300, 0x800) or (route == 0 and M >= 1024 and N >= 1024)


def res_as_initial_value(route, M, N):
    """The kernels on which a 16-byte aligned residual with ldr % 8 == 0 (and N % 8 == 0) enters as the accumulators' initial value."""
    return route in (0x200, 0x300) or (route == 0 and M >= 1024 and N >= 1024)


def operands(M, N, K, epi, off, ldr, seed):
    """Random operands of one case; the VALUES depend on (M, N, K, epi, seed) only, not on `off` (elements bias / scale / res start into
    their allocations) or `ldr`."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    o = SimpleNamespace(M=M, N=N, K=K, epi=epi, ldx=K + 8, ldr=ldr, P=0, scale=None, res=None, arg=None, mask=None)
    o.x = placed(bf(rn(M, K)), 0, o.ldx)
    o.w = placed(bf(rn(N, K) / math.sqrt(K)), 0, o.ldx)
    o.bias = None if epi == "gelu_bwd" else placed(bf(rn(N)), off)
    if epi.endswith("_ls"):
        o.scale = placed(bf(0.1 * (1.0 + 0.1 * rn(N))), off)
    if epi in ("residual", "residual_ls", "save", "save_ls", "gelu_bwd"):
        o.res = o.arg = placed(bf(rn(M, N)), off, ldr)
    elif epi == "embed":
        o.res = o.arg = placed(bf(rn(PATCH + 1, N)), off, ldr)
        o.P = PATCH
    elif epi == "f32_mask":
        o.mask = o.arg = (torch.arange(M, device=DEV) % 3 == 0).to(torch.uint8)   # row 0 masked, row 1 live
    m = torch.arange(M, device=DEV)
    o.orow = m // PATCH * (PATCH + 1) + 1 + m % PATCH if epi == "embed" else m    # output row of GEMM row m
    o.rows_out = int(o.orow[-1]) + 1
    return o


def reference(o, rows=None):
    """fp64 reference and sum|terms| of GEMM rows `rows` (all) -> (ref, mag, pre_ref, pre_mag); the last two for the save forms."""
    rows = torch.arange(o.M, device=DEV) if rows is None else rows
    N, K = o.N, o.K
    x, w = o.x[rows, :K].double(), o.w[:, :K].double()
    acc, amag = x @ w.t(), x.abs() @ w.abs().t()
    b = o.bias.double() if o.bias is not None else torch.zeros(N, dtype=torch.float64, device=DEV)
    z, mag = acc + b, amag + b.abs()
    if o.epi == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0))), mag, None, None
    if o.epi == "quick_gelu":
        return z * torch.sigmoid(1.702 * z), mag, None, None
    if o.epi in ("residual", "residual_ls", "save", "save_ls"):
        ls = o.scale.double() if o.scale is not None else torch.ones(N, dtype=torch.float64, device=DEV)
        r = o.res[rows, :N].double()
        return r + z * ls, r.abs() + mag * ls.abs(), z, mag
    if o.epi == "embed":
        t = o.res[1 + rows % PATCH, :N].double()
        return z + t, mag + t.abs(), None, None
    if o.epi == "gelu_bwd":
        return acc * gelu_grad64(o.res[rows, :N]), amag * 1.2, None, None
    return z, mag, None, None   # bias, f32, f32_mask


def out_buffer(o, ldy, off, behind=16):
    """Canary-filled output of `rows_out + behind` rows, starting `off` elements into its allocation -> (allocation, [rows, ldy] view)."""
    dtype = torch.float32 if o.epi.startswith("f32") else torch.bfloat16
    rows = o.rows_out + behind
    flat = canaries(off + rows * ldy, dtype)
    v = flat[off:].view(rows, ldy)
    assert v.data_ptr() % 16 == (off * flat.element_size()) % 16
    return flat, v


def launch(o, route, y, pre=None, extra=0):
    L = _lib.lib()
    ldy = y.stride(0)
    if o.epi.startswith("save"):
        assert pre.stride(0) == ldy
        rc = L.vllm_gemm_bf16_residual_save(P(o.x), P(o.w), P(o.bias), P(y), P(pre), o.M, o.N, o.K, o.ldx, o.ldx, ldy, 3 | route, P(o.scale),
                                            P(o.res), o.ldr, stream())
    else:
        rc = L.vllm_gemm_bf16(P(o.x), P(o.w), P(o.bias), P(y), o.M, o.N, o.K, o.ldx, o.ldx, ldy, EPI[o.epi] | route | extra, P(o.scale),
                              P(o.arg), o.ldr if o.res is not None else 0, o.P, stream())
    _lib.check(rc, f"{o.epi} route {route:#x} M{o.M} N{o.N} K{o.K} ldy{ldy}")


def assert_block_only(o, flat, y, what):
    """Every element of the block (the scattered rows of the embed epilogue) is written, everything else is the canary it was."""
    written = torch.zeros(y.shape, dtype=torch.bool, device=DEV)
    written[o.orow, :o.N] = True
    assert torch.isfinite(y[written].float()).all(), f"{what}: an element of the block was not written"
    assert intact(y[~written]), f"{what}: wrote outside the block (padding columns, rows behind M, CLS rows)"
    head = flat.numel() - y.numel()
    assert intact(flat[:head]), f"{what}: wrote in front of Y"


def run_and_check(o, route, ldy, off, ref, what, behind=16):
    """One launch into fresh canary-filled buffers, canaries and the fp64 bound -> (Y view, pre view or None)."""
    flat, y = out_buffer(o, ldy, off, behind)
    pflat, pre = out_buffer(o, ldy, off, behind) if o.epi.startswith("save") else (None, None)
    launch(o, route, y, pre)
    torch.cuda.synchronize()
    assert_block_only(o, flat, y, what)
    z, mag, pz, pmag = ref
    out = y[o.orow, :o.N]
    if o.epi.startswith("f32"):
        live = torch.ones(o.M, dtype=torch.bool, device=DEV) if o.mask is None else o.mask == 0
        assert (out[~live] == 0).all(), f"{what}: a masked row is not exactly zero"
        ratio = ((out[live].double() - z[live]).abs() / (2.0 ** -17 * mag[live])).max().item() if live.any() else 0.0
        print(f"{what}: fp32 max |out - ref| / (2^-17 sum|terms|) = {ratio:.3f}")
        assert ratio <= 1.0, f"{what}: {ratio:.3f} of the fp32 bound"
    else:
        scaled = o.scale is not None and eight_phase(route, o.M, o.N)
        assert_bound(out, z, mag, what, 2.0 ** -16 if scaled else 2.0 ** -17)
    if pre is not None:
        assert_block_only(o, pflat, pre, what + " pre")
        assert_bound(pre[:o.M, :o.N], pz, pmag, what + " pre")
    return y, pre


# ---- small cases: N = 4 (mod 8), ldy = N + 4, ldr = N + 12, every bf16 pointer 8 bytes into its allocation -----------------------------
@pytest.mark.parametrize("epi", list(EPI))
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_small_shapes_at_the_contract_minimum(route, epi):
    for i, (M, N, K) in enumerate(SMALL):
        o = operands(M, N, K, epi, 4, N + 12, seed=1000 * i + M + N + K)
        off = 0 if epi.startswith("f32") else 4          # fp32 output: 16-byte aligned base, ldy = N + 4 floats
        run_and_check(o, route, N + 4, off, reference(o), f"{epi} {route:#x} {M}x{N}x{K}")


# ---- N % 8 == 0 with rows that are only 8-byte aligned: same bits as with 16-byte aligned rows -----------------------------------------
@pytest.mark.parametrize("epi", list(EPI))
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_rows_8_byte_aligned_give_the_bits_of_16_byte_aligned_rows(route, epi):
    """ldy = N + 4 (and ldr = N + 4) against ldy = N + 8 (ldr = N + 8) on the same values: the direct and the row-wise LDS epilogue run
    the same epi_value arithmetic, so the block is the same bit for bit.  The exception is the residual (and residual-save) epilogue on
    the 8-phase kernels with 256- / 192-row tiles (forced, or automatic from 1024 x 1024 on): there ldr % 8 decides whether the
    residual enters as the accumulators' initial value, another fp32 summation order.  Those two meet the bound each; and with ldr
    held fixed, ldy alone changes no bit there either (ldr = N + 4: residual read in the epilogue; ldr = N + 8: initial value,
    stored through LDS and straight from the accumulators)."""
    residual = epi in ("residual", "residual_ls", "save", "save_ls")
    for i, (M, N, K) in enumerate(ROWS8):
        seed = 77 + i
        o4, o8 = operands(M, N, K, epi, 0, N + 4, seed), operands(M, N, K, epi, 0, N + 8, seed)
        assert torch.equal(bits(o4.x), bits(o8.x)) and (o4.res is None or torch.equal(bits(o4.res[:, :N]), bits(o8.res[:, :N])))
        ref = reference(o4)
        what = f"{epi} {route:#x} {M}x{N}x{K}"
        y44, p44 = run_and_check(o4, route, N + 4, 0, ref, what + " ldy+4 ldr+4")
        y88, p88 = run_and_check(o8, route, N + 8, 0, ref, what + " ldy+8 ldr+8")
        pairs = [(y44, p44, y88, p88)]
        if residual and res_as_initial_value(route, M, N):
            y84, p84 = run_and_check(o4, route, N + 8, 0, ref, what + " ldy+8 ldr+4")
            y48, p48 = run_and_check(o8, route, N + 4, 0, ref, what + " ldy+4 ldr+8")
            pairs = [(y44, p44, y84, p84), (y48, p48, y88, p88)]
        for ya, pa, yb, pb in pairs:
            assert torch.equal(bits(ya[o4.orow, :N]), bits(yb[o4.orow, :N])), f"{what}: the row stride of Y changes the result"
            if pa is not None:
                assert torch.equal(bits(pa[:M, :N]), bits(pb[:M, :N])), f"{what}: the row stride of Y changes pre"


# ---- the persistent schedule with ldy = 4 (mod 8): 16-byte stores to rows that are 8-byte aligned ---------------------------------------
PERSIST = [(70001, 256, 128, 0x200), (16500, 1024, 128, 0x300)]
PERSIST_IDS = [f"M{c[0]}_N{c[1]}_K{c[2]}_{c[3]:#x}" for c in PERSIST]
#            name -> (epilogue, LayerScale, gemm_res_ring, ldr - N)
PCASES = {"bias": (0, False, 1, 0), "quick_gelu": (2, False, 1, 0), "residual_ls": (3, True, 1, 4), "residual_ring": (3, False, 1, 8),
          "residual_epilogue": (3, False, 0, 8)}


@functools.lru_cache(maxsize=None)
def persistent_operands(i):
    """Operands of persistent shape i (16-byte aligned, as the schedule requires) and the fp64 pieces of the first, middle and last 300
    rows, computed once and left unchanged."""
    M, N, K, force = PERSIST[i]
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    d = SimpleNamespace(x=placed(bf(rn(M, K)), 0, K + 8), w=placed(bf(rn(N, K) / math.sqrt(K)), 0, K + 8), b=bf(rn(N)),
                        ls=bf(0.1 + 0.05 * rn(N)))
    res = bf(rn(M, N))
    d.res = {4: placed(res, 0, N + 4), 8: placed(res, 0, N + 8)}
    d.rows = torch.cat([torch.arange(0, 300), torch.arange(M // 2, M // 2 + 300), torch.arange(M - 300, M)]).to(DEV)
    x, w = d.x[d.rows, :K].double(), d.w[:, :K].double()
    d.z = x @ w.t() + d.b.double()
    d.mag = x.abs() @ w.abs().t() + d.b.double().abs()
    d.r = res[d.rows].double()
    return d


def persistent_launch(i, name, extra=0):
    """One call at persistent shape i with ldy = N + 4 into a canary-filled [M + 300, N + 4] buffer -> (buffer, rise of the counter)."""
    M, N, K, force = PERSIST[i]
    epi, scaled, ring, rpad = PCASES[name]
    d = persistent_operands(i)
    L = _lib.lib()
    y = canaries((M + 300) * (N + 4), torch.bfloat16).view(M + 300, N + 4)
    res = d.res[rpad] if epi == 3 else None
    before = L.vllm_gemm_persistent_launches()
    old = _lib.set_option("gemm_res_ring", ring)
    try:
        _lib.check(L.vllm_gemm_bf16(P(d.x), P(d.w), P(d.b), P(y), M, N, K, K + 8, K + 8, N + 4, epi | force | extra, P(d.ls) if scaled else None,
                                    P(res), N + rpad if epi == 3 else 0, 0, stream()))
    finally:
        _lib.set_option("gemm_res_ring", old)
    torch.cuda.synchronize()
    return y, L.vllm_gemm_persistent_launches() - before


@pytest.mark.parametrize("name", list(PCASES))
@pytest.mark.parametrize("i", range(len(PERSIST)), ids=PERSIST_IDS)
def test_persistent_schedule_rows_8_byte_aligned(i, name):
    M, N, K, force = PERSIST[i]
    epi, scaled, ring, rpad = PCASES[name]
    d = persistent_operands(i)
    y, rise = persistent_launch(i, name)
    assert rise == 1, "the persistent schedule was not taken"
    assert torch.isfinite(y[:M, :N].float()).all(), "an element of the block was not written"
    assert intact(y[M:]) and intact(y[:, N:]), "wrote outside the output block"
    z, mag = d.z, d.mag
    if epi == 2:
        z = z * torch.sigmoid(1.702 * z)
    elif epi == 3:
        ls = d.ls.double() if scaled else torch.ones(N, dtype=torch.float64, device=DEV)
        z, mag = d.r + z * ls, d.r.abs() + mag * ls.abs()
    assert_bound(y[d.rows, :N], z, mag, f"persistent {name} {PERSIST_IDS[i]} ldy = N + 4")
    if epi != 3:
        yt, rise = persistent_launch(i, name, extra=0x1000)
        assert rise == 0, "VLLM_GEMM_FORCE_TILEWISE did not keep the call off the persistent schedule"
        assert torch.equal(bits(y), bits(yt)), "persistent schedule differs from one workgroup per tile"


def test_persistent_schedule_leaves_N_1028_to_the_tilewise_kernel():
    """N = 1028 (4 mod 8) at M = 16500: the persistent schedule's 16-byte pieces cannot end at N; the call must stay off it (counter
    unchanged), and the tile-wise kernel's direct epilogue meets the bound.  X is the shape's; the weight and the bias are this test's."""
    i, N = 1, 1028
    M, N0, K, force = PERSIST[i]
    d = persistent_operands(i)
    g = torch.Generator(device=DEV).manual_seed(5)
    w = placed(bf(torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)), 0, K + 8)
    b = bf(torch.randn(N, device=DEV, generator=g))
    L = _lib.lib()
    y = canaries((M + 300) * (N + 4), torch.bfloat16).view(M + 300, N + 4)
    before = L.vllm_gemm_persistent_launches()
    _lib.check(L.vllm_gemm_bf16(P(d.x), P(w), P(b), P(y), M, N, K, K + 8, K + 8, N + 4, 0 | force, None, None, 0, 0, stream()))
    torch.cuda.synchronize()
    assert L.vllm_gemm_persistent_launches() == before, "the persistent schedule took N % 8 != 0"
    assert torch.isfinite(y[:M, :N].float()).all(), "an element of the block was not written"
    assert intact(y[M:]) and intact(y[:, N:]), "wrote outside the output block"
    x, wd = d.x[d.rows, :K].double(), w[:, :K].double()
    assert_bound(y[d.rows, :N], x @ wd.t() + b.double(), x.abs() @ wd.abs().t() + b.double().abs(), "tile-wise N = 1028, ldy = N + 4")
