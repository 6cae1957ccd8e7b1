"""CPU: the shapes of test_multitrip_rows_gpu.py (multitrip_inputs.py) cannot be vacuous on any part the project may meet: for 64, 104,
228, 256 and 304 compute units every case reaches at least 3 loop trips in some thread with a ragged last trip and a ragged last block,
by the launch arithmetic restated there, and holds less than 256 MB of device memory."""
import pytest

import multitrip_inputs as M


@pytest.mark.parametrize("cus", M.CU_COUNTS)
def test_every_shape_reaches_three_ragged_trips_within_the_memory_limit(cus):
    cases = M.cases(cus)
    assert len(cases) == 4 * 11 + 4 + 3 + 1 + 2 + 4 + 8
    for c in cases:
        assert c.trips >= M.MIN_TRIPS, c
        assert c.ragged, c
        assert 0 < c.bytes < M.MEM_LIMIT, (c, c.bytes >> 20)


@pytest.mark.parametrize("cus", M.CU_COUNTS)
def test_norm_shapes_by_the_plan_itself(cus):
    """independent of norm_ok: walk the ranges the plan hands out"""
    for C in sorted(set(M.NORM_C + M.NORM_C_LN)):
        rows = M.norm_rows(C, cus)
        p = M.rb_plan(rows, C, cus)
        assert p["tpr"] * p["maxch"] * 8 >= C and p["rg"] * p["tpr"] == 256
        ranges = [(vb * p["rpb"], min(vb * p["rpb"] + p["rpb"], rows)) for vb in range(p["grid"] * p["rg"])]
        assert ranges[0][1] - ranges[0][0] >= 3                                     # a full range: at least 3 trips
        live = [r for r in ranges if r[0] < rows]
        assert len(live) == p["nbv"] and sum(b - a for a, b in live) == rows
        assert 0 < live[-1][1] - live[-1][0] < p["rpb"]                             # the last range ends early
        assert rows >= 4 * cus * p["rg"] + 3 and rows - (4 * cus * p["rg"] + 3) < 3  # the issue's count, or the next ragged one
        assert p["nbv"] <= 2 * cus * p["rg"]


def test_the_counts_on_256_compute_units():
    c = M.case(256, "rms_bwd", C=200)
    assert (c.sizes["rows"], c.sizes["rpb"], c.sizes["nbv"], c.sizes["last_range"], c.sizes["empty_vbs"], c.trips) == (4099, 3, 1367, 1, 1, 3)
    assert M.colsum_chain(4099, 1367) == 3 + 171 + 8
    assert [M.case(256, "ls_bwd", C=C).sizes["rows"] for C in (512, 1024, 2048, 8192)] == [4099, 2051, 1027, 1027]
    assert {C: M.case(256, "ln_res_bwd", C=C).sizes["maxch"] for C in (2048, 2112, 4096, 4160, 8192)} == {2048: 1, 2112: 2, 4096: 2, 4160: 4, 8192: 4}
    a = M.case(256, "add_layernorm", C=256)
    assert (a.sizes["ngroups"], a.sizes["rows"], a.sizes["nwaves"], a.trips) == (24581, 49161, 8192, 4)
    b = M.case(256, "box_refine", C=512)
    assert (b.sizes["ngroups"], b.sizes["rows"], b.trips) == (24581, 24581, 4)
    r = M.case(256, "refpoint_embed")
    assert r.sizes["rows"] == 16385 and r.sizes["Lq"] == 3277 and r.sizes["rows_per_trip"] == 8192 and r.trips == 3
    assert M.case(256, "add_bf16_aligned").sizes["n"] % 8 == 3 and M.case(256, "add_bf16_aligned").sizes["items"] == 2 * 4096 * 256 + 1
    assert M.case(256, "f32_to_bf16").sizes["items"] == 2 * 1048576 + 1
    assert M.case(256, "bf16_to_f32").sizes["items"] == 2 * 2097152 + 1
    for k in ("scatter_rows", "copy_rows", "copy_rows_masked", "rows_segment_sum"):
        assert M.case(256, k, C=8).sizes["rows"] == 3 * 16384 + 5 and M.case(256, k, C=8).trips == 4
    assert M.case(256, "rows_segment_sum", C=520).trips == 7


def test_228_compute_units_need_the_next_count():
    """4 * 228 * 4 + 3 = 3651 rows divide by rpb = 3: no range would end early"""
    assert not M.norm_ok(3651, M.rb_plan(3651, 200, 228)["nbv"])
    assert M.norm_rows(200, 228) == 3652


def test_one_trip_shapes_fail_the_precondition():
    """the checks are not vacuous themselves: the kernel-alone tests' shapes fail them"""
    assert not M.norm_ok(300, M.rb_plan(300, 128, 256)["nbv"])
    assert not M.norm_ok(4098, M.rb_plan(4098, 200, 256)["nbv"])      # 3 trips, but every range full
    assert not M.group_ok(257, 256, 256) and not M.group_ok(49160, 256, 256)
    assert not M.stride_ok(4099, 4096) and not M.stride_ok(3 * 4096 * 256, 4096)
    assert not M.mover_ok(37) and not M.mover_ok(3 * 16384)


def test_reference_slices_cover_the_rows_once():
    for rows, cols in ((4099, 200), (1027, 8192), (49161, 64), (1, 8)):
        s = M.ref_slices(rows, cols)
        assert s[0][0] == 0 and s[-1][1] == rows and all(a[1] == b[0] for a, b in zip(s, s[1:]))
        assert all((b - a) * cols <= max(M.REF_ELEMS, cols) for a, b in s)
