"""Shapes of test_multitrip_rows_gpu.py: for every row-walking kernel the smallest row / element count at which, on a device with
``cus`` compute units, some thread goes round its loop at least 3 times, the last trip is ragged and the last block's work is ragged too.
Pure Python: the launch arithmetic of the kernels' hosts is RESTATED here (the file and the statement are named at each function), so
test_multitrip_inputs_cpu.py can check the shapes for several parts without a GPU, and the GPU tests can assert the same precondition
against the device they run on before they launch.

  walker                       a "trip"                                             restated from
  norm.hip backward kernels    one row of a virtual block's range of `rpb` rows     rb_plan (norm.hip)
  add_layernorm, box_refine,   one row group of a wave (2 rows at C <= 256, else 1)  row_group_plan (row_groups.hpp)
  qs_tail
  refpoint_embed, add_bf16     one 16-byte chunk (or element) of a thread           refpoint_embed_launch / add_launch
  f32 <-> bf16 conversions     one vector / element / chunk of a thread             cvt_launch, stream_grid (msda_layer*.hip)
  row movers, segment sum      one row (or row slab) of a wave                      grid_for (embed.hip)

Every case is a ``Case``: the sizes the test passes, ``trips`` (loop trips of the busiest walker), ``ragged`` (the last trip does not
fill every walker AND the last block is not full), and ``bytes``, the device memory the GPU test of that case holds at once (operands,
outputs of both runs, workspace, and the fp64 temporaries of a reference that is evaluated ``REF_ELEMS`` elements at a time)."""
import collections

CU_COUNTS = (64, 104, 228, 256, 304)
MIN_TRIPS = 3
MEM_LIMIT = 256 << 20
REF_ELEMS = 1 << 18          # elements per slice of an fp64 reference
REF_TEMPS = 20               # fp64 tensors of one slice alive at once, at most (rms_bwd_ref / ln_bwd_ref with their magnitudes)

NORM_C = (8, 200, 512, 576, 1024, 1088, 2048, 2112, 4096, 4160, 8192)
NORM_C_LN = (64, 192, 512, 576, 1024, 1088, 2048, 2112, 4096, 4160, 8192)     # vllm_layernorm_backward_res_bf16: C % 64 == 0
ALN_C = (64, 256, 320, 512)
REFINE_C = (64, 256, 512)
MOVER_C = (8, 520)
MOVER_WAVES = 4096 * 4       # grid_for: at most 4096 blocks of 4 waves
REFPOINT_P, REFPOINT_L, REFPOINT_B = 128, 4, 5

Case = collections.namedtuple("Case", "kernel sizes trips ragged bytes")


def ceil_div(a, b):
    return -(-a // b)


def ref_bytes(cols):
    """the fp64 temporaries of one reference slice of whole rows"""
    rows = max(1, REF_ELEMS // cols)
    return REF_TEMPS * rows * cols * 8


def ref_slices(rows, cols):
    """[(r0, r1)] of at most REF_ELEMS elements each"""
    step = max(1, REF_ELEMS // cols)
    return [(r, min(r + step, rows)) for r in range(0, rows, step)]


# ---- norm.hip: rb_plan ---------------------------------------------------------------------------------------------------------------
def rb_plan(rows, C, cus):
    """rb_plan(rows, C) of norm.hip -> dict(tpr, maxch, rg, rpb, nbv, grid)"""
    nchunk = C // 8
    tpr = 64 if nchunk <= 64 else 128 if nchunk <= 128 else 256
    per = ceil_div(nchunk, tpr)
    maxch = 1 if per <= 1 else 2 if per <= 2 else 4
    rg = 256 // tpr
    b = max(1, min(rows, 2 * cus * rg))
    rpb = ceil_div(rows, b)
    nbv = ceil_div(rows, rpb) if rpb > 0 else 1
    return dict(tpr=tpr, maxch=maxch, rg=rg, rpb=rpb, nbv=nbv, grid=ceil_div(nbv, rg))


def norm_ok(rows, nbv):
    """the precondition the GPU tests assert on the plan read back from the workspace query: every range is walked for at least 3 rows
    and the last range ends early"""
    rpb = ceil_div(rows, nbv)
    return rpb >= MIN_TRIPS and rows % rpb != 0


def norm_rows(C, cus):
    """4 cus (256 / TPR) + 3 rows: rpb = 3 and a last range of fewer than 3 rows -- unless cus (256 / TPR) is a multiple of 3 (228 CUs),
    where that count divides by 3: then the next count that does not."""
    rg = rb_plan(1, C, cus)["rg"]
    rows = 4 * cus * rg + 3
    while not norm_ok(rows, rb_plan(rows, C, cus)["nbv"]):
        rows += 1
    return rows


def norm_case(kernel, C, cus):
    rows = norm_rows(C, cus)
    p = rb_plan(rows, C, cus)
    sums = 2 if kernel == "ln_res_bwd" else 1
    # x, grad_y, grad_res and three outputs (two runs and the in-place copy) with padded rows, the partial sums, the reference slices
    mem = 6 * rows * (C + 24) * 2 + sums * p["nbv"] * C * 4 + ref_bytes(C)
    sizes = dict(rows=rows, C=C, last_range=rows - (p["nbv"] - 1) * p["rpb"], empty_vbs=p["grid"] * p["rg"] - p["nbv"], **p)
    return Case(kernel, sizes, ceil_div(rows, p["nbv"]), norm_ok(rows, p["nbv"]), mem)


def norm_g2_case(C, cus):
    """the G = 2 call on a [rows, 3C] slab: the slab, its gradient, the two out-of-place results and the saved v block"""
    rows = norm_rows(C, cus)
    p = rb_plan(rows, C, cus)
    mem = rows * (2 * (3 * C + 8) + 3 * C) * 2 + 2 * p["nbv"] * C * 4 + ref_bytes(C)
    return Case("rms_bwd_g2", dict(rows=rows, C=C, **p), ceil_div(rows, p["nbv"]), norm_ok(rows, p["nbv"]), mem)


def colsum_chain(rows, nbv):
    """the longest chain of fp32 additions behind one column sum: rpb rows in a range's registers, ceil(nbv / 8) partials in a slice of
    colsum_reduce_kernel, its 8 slices"""
    return ceil_div(rows, nbv) + ceil_div(nbv, 8) + 8


# ---- add_layernorm_kernel / box_refine_kernel / qs_tail_kernel: row groups over waves ------------------------------------------------
def group_plan(rows, C, cus):
    """row_group_plan(rows, C) of csrc/row_groups.hpp, the one launch geometry of the four row-group kernels (the workgroups it returns
    times the four waves of ROWG_THREADS) -> dict(G, rows_per_group, ngroups, nwaves)"""
    G = 32 if C <= 256 else 64
    rpg = 64 // G
    ngroups = ceil_div(rows, rpg)
    blocks = min(ceil_div(ngroups, 4), cus * 8)
    return dict(G=G, rows_per_group=rpg, ngroups=ngroups, nwaves=blocks * 4)


def group_ok(rows, C, cus):
    p = group_plan(rows, C, cus)
    last = p["ngroups"] % p["nwaves"]
    return (ceil_div(p["ngroups"], p["nwaves"]) >= MIN_TRIPS and last != 0 and last % 4 != 0 and rows % 2 == 1)


def group_rows(C, cus):
    """3 * 32 cus + 5 row groups and an odd row count (C <= 256: the last half-wave has no row)"""
    rpg = group_plan(1, C, cus)["rows_per_group"]
    return (3 * 32 * cus + 5) * rpg - (rpg - 1)


def group_case(kernel, C, cus):
    rows = group_rows(C, cus)
    p = group_plan(rows, C, cus)
    if kernel == "add_layernorm":   # x, res, pos, y, y_pos and the copy of x the in-place call rewrites (vllm_add_bf16 runs on slices)
        mem = rows * ((C + 16) + (C + 24) + (C + 8) + (C + 40) + (C + 8) + (C + 16)) * 2 + ref_bytes(C)
    else:                           # h, ref and three outputs
        mem = rows * (C + 16) * 2 + 4 * rows * 16 + ref_bytes(C)
    return Case(kernel, dict(rows=rows, C=C, **p), ceil_div(p["ngroups"], p["nwaves"]), group_ok(rows, C, cus), mem)


# ---- grid-stride loops over items ----------------------------------------------------------------------------------------------------
def stride_trips(items, cap_blocks):
    threads = min(ceil_div(max(items, 1), 256), cap_blocks) * 256
    return ceil_div(items, threads)


def stride_ok(items, cap_blocks):
    threads = min(ceil_div(max(items, 1), 256), cap_blocks) * 256
    return ceil_div(items, threads) >= MIN_TRIPS and items % threads != 0 and items % 256 != 0


def stride_rows(unit, cap_blocks, multiple_of=1):
    """the smallest row count (a multiple of `multiple_of`) whose rows * unit items pass stride_ok"""
    rows = ceil_div(2 * cap_blocks * 256 + 1, unit)
    rows = ceil_div(rows, multiple_of) * multiple_of
    while not stride_ok(rows * unit, cap_blocks):
        rows += multiple_of
    return rows


def refpoint_case(cus):
    """refpoint_embed_launch: rows P / 2 chunks over at most 8 cus blocks.  rows = B Lq with B = 5, so Lq is 2/5 of a trip's rows and the
    image index changes inside every trip."""
    P, L, B = REFPOINT_P, REFPOINT_L, REFPOINT_B
    rows = stride_rows(P // 2, cus * 8, multiple_of=B)
    items = rows * (P // 2)
    rows_per_trip = cus * 8 * 256 // (P // 2)
    mem = rows * (16 + L * 16 + (4 * P + 24) * 2) * 2 + ref_bytes(4 * P)
    sizes = dict(rows=rows, B=B, Lq=rows // B, L=L, P=P, items=items, rows_per_trip=rows_per_trip)
    return Case("refpoint_embed", sizes, stride_trips(items, cus * 8), stride_ok(items, cus * 8) and rows // B < rows_per_trip, mem)


def add_cases(cus):
    """add_launch: n / 8 chunks (all three operands 16-byte aligned) or n elements over at most 16 cus blocks; the aligned case ends in
    a scalar tail of 3 elements"""
    cap = cus * 16
    n8 = stride_rows(1, cap)
    aligned = Case("add_bf16_aligned", dict(n=8 * n8 + 3, items=n8, lead=0), stride_trips(n8, cap), stride_ok(n8, cap), 4 * (8 * n8 + 19) * 2)
    n = stride_rows(1, cap)
    return [aligned, Case("add_bf16_misaligned", dict(n=n, items=n, lead=1), stride_trips(n, cap), stride_ok(n, cap), 4 * (n + 16) * 2)]


def convert_cases():
    """cvt_launch (4096 blocks over float4 vectors, a tail of n % 4 elements in one thread) and stream_grid (8192 blocks over float4
    vectors / elements / 8-element chunks); none depends on the device.  The masked forms take rows of `cols`: 100 (25 vectors a row, the
    vector form) and 37 (the element form).  The checks run on slices, one fp32 / int32 temporary of REF_ELEMS * 8 elements at a time."""
    check = 3 * REF_ELEMS * 8 * 4
    n4 = stride_rows(1, 4096)
    out = [Case("f32_to_bf16", dict(n=4 * n4 + 3, items=n4), stride_trips(n4, 4096), stride_ok(n4, 4096), (4 * n4 + 3) * 6 + check)]
    for name, cols, unit in (("f32_to_bf16_masked_vector", 100, 25), ("f32_to_bf16_masked_scalar", 37, 37)):
        rows = stride_rows(unit, 8192)
        items = rows * unit
        out.append(Case(name, dict(rows=rows, cols=cols, items=items, elems_per_trip=8192 * 256 * (cols // unit)), stride_trips(items, 8192),
                        stride_ok(items, 8192), rows * cols * 6 + rows + check))
    n8 = stride_rows(1, 8192)
    out.append(Case("bf16_to_f32", dict(n=8 * n8 + 5, items=n8), stride_trips(n8, 8192), stride_ok(n8, 8192), (8 * n8 + 13) * 6 + check))
    return out


def mover_ok(items):
    waves = min(ceil_div(items * 64, 256), 4096) * 4
    last = items % waves
    return ceil_div(items, waves) >= MIN_TRIPS and last != 0 and last % 4 != 0


def mover_cases():
    """grid_for(rows * 64): a row (the segment sum: a slab of 512 channels of a row) per wave, at most 4096 blocks.  3 * 16384 + 5 rows."""
    rows = 3 * MOVER_WAVES + 5
    out = []
    for kernel in ("scatter_rows", "copy_rows", "copy_rows_masked", "rows_segment_sum"):
        for C in MOVER_C:
            items = rows * ceil_div(C // 8, 64) if kernel == "rows_segment_sum" else rows
            waves = min(ceil_div(items * 64, 256), 4096) * 4
            # source, guarded output of two runs, the expected rows, indices; the segment sum also its reference slices
            mem = 4 * (rows + 2) * C * 2 + 4 * rows * 8 + (ref_bytes(C) if kernel == "rows_segment_sum" else 0)
            out.append(Case(kernel, dict(rows=rows, C=C, items=items, waves=waves), ceil_div(items, waves), mover_ok(items), mem))
    return out


def cases(cus):
    """every case of test_multitrip_rows_gpu.py on a device with `cus` compute units"""
    out = [norm_case("rms_bwd", C, cus) for C in NORM_C] + [norm_case("ln_res_bwd", C, cus) for C in NORM_C_LN]
    out += [norm_case("ls_bwd", C, cus) for C in NORM_C] + [norm_g2_case(C, cus) for C in NORM_C]
    out += [group_case("add_layernorm", C, cus) for C in ALN_C] + [group_case("box_refine", C, cus) for C in REFINE_C]
    out.append(refpoint_case(cus))
    return out + add_cases(cus) + convert_cases() + mover_cases()


def case(cus, kernel, **sizes):
    """the one case of `kernel` whose sizes include `sizes`"""
    found = [c for c in cases(cus) if c.kernel == kernel and all(c.sizes.get(k) == v for k, v in sizes.items())]
    assert len(found) == 1, (kernel, sizes, len(found))
    return found[0]
