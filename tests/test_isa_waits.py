"""CPU: inline-asm loads are waited for before anything touches their destination registers (tests/isa_waits.py).

The compiler does not know an `asm volatile("ds_read_b128 ...")` is a load: it takes the outputs for ready when the statement
ends.  If it copies, spills, reads or reuses such a register before the kernel's own `s_waitcnt`, the kernel computes with data
that has not arrived -- rare wrong tiles that parity tests and race screens only see when the data happens to arrive late.
Synthetic assembly pins each rule of the analyser; then every file under visionllm_amd/csrc is compiled to device assembly with
the Makefile's flags and every kernel instantiation must come out clean, compiler-emitted loads included."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

import isa_waits as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visionllm_amd", "csrc")


def kernel(body, inline=()):
    """One kernel around `body` (lines of assembly); the 0-based line indices in `inline` are wrapped as inline-asm blocks."""
    out = ["\t.globl\tk", "\t.type\tk,@function", "k:"]
    for i, ln in enumerate(body):
        if i in inline:
            out += ["\t;;#ASMSTART", ln, "\t;;#ASMEND"]
        else:
            out.append(ln if ln.endswith(":") else "\t" + ln)
    out += ["\ts_endpgm", ".Lfunc_end0:", "\t.size\tk, .Lfunc_end0-k"]
    return "\n".join(out) + "\n"


def findings(body, inline=()):
    return W.analyse(kernel(body, inline)).findings


def reads(n, first=16):
    return [f"ds_read_b128 v[{first + 4 * i}:{first + 4 * i + 3}], v100" for i in range(n)]


# ---- one rule per test: each has a snippet that passes and one that fails ----------------------------------------------------

def test_read_of_a_pending_destination():
    assert findings(["ds_read_b128 v[0:3], v4", "v_add_f32_e32 v5, v1, v6"], inline={0})
    assert not findings(["ds_read_b128 v[0:3], v4", "s_waitcnt lgkmcnt(0)", "v_add_f32_e32 v5, v1, v6"], inline={0})
    f = findings(["ds_read_b128 v[0:3], v4", "v_add_f32_e32 v5, v1, v6"], inline={0})[0]
    assert f.issuer_inline and "ds_read_b128" in f.issuer_text and "v_add_f32" in f.text and f.kernel == "k"


def test_write_of_a_pending_destination():
    assert findings(["ds_read_b128 v[0:3], v4", "v_mov_b32_e32 v2, 0"])
    assert not findings(["ds_read_b128 v[0:3], v4", "v_mov_b32_e32 v5, 0"])
    assert not findings(["ds_read_b128 v[0:3], v4", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v2, 0"])


def test_spill_of_a_pending_destination():
    assert findings(["ds_read_b128 v[0:3], v4", "scratch_store_dword off, v3, s33 offset:8"])
    assert not findings(["ds_read_b128 v[0:3], v4", "s_waitcnt lgkmcnt(0)", "scratch_store_dword off, v3, s33 offset:8"])


def test_partial_overlap_and_agpr_ranges():
    assert findings(["global_load_dwordx4 v[8:11], v[0:1], off", "v_mov_b32_e32 v12, v10"])
    assert not findings(["global_load_dwordx4 v[8:11], v[0:1], off", "v_mov_b32_e32 v12, v7"])
    assert findings(["global_load_dwordx4 v[8:11], v[0:1], off", "v_pk_fma_f32 v[12:13], v[10:11], v[2:3], v[4:5]"])
    assert findings(["global_load_dwordx4 a[0:3], v[4:5], off", "v_accvgpr_read_b32 v0, a2"])
    assert not findings(["global_load_dwordx4 a[0:3], v[4:5], off", "v_accvgpr_read_b32 v0, a4"])
    assert not findings(["global_load_dwordx4 a[0:3], v[4:5], off", "v_mov_b32_e32 v0, v2"])      # a2 is not v2
    assert findings(["s_load_dwordx2 s[4:5], s[0:1], 0x0", "s_mov_b32 s6, s5"])


def test_counted_wait_with_eight_younger_lds_reads_retires():
    body = ["ds_read_b128 v[0:3], v4"] + reads(8) + ["s_waitcnt lgkmcnt(8)", "v_mov_b32_e32 v200, v0"]
    assert not findings(body)
    body = ["ds_read_b128 v[0:3], v4"] + reads(7) + ["s_waitcnt lgkmcnt(8)", "v_mov_b32_e32 v200, v0"]
    assert findings(body)
    # ... and the eight younger ones are still in flight after it
    body = ["ds_read_b128 v[0:3], v4"] + reads(8) + ["s_waitcnt lgkmcnt(8)", "v_mov_b32_e32 v200, v16"]
    assert findings(body)


def test_counted_wait_needs_eight_younger_reads_on_every_path():
    def body(skip_path_reads):
        return (["ds_read_b128 v[0:3], v4"] + reads(7) + ["s_cbranch_scc1 .LBB0_2"] + reads(1, first=60) + [".LBB0_2:"]
                + reads(skip_path_reads, first=80) + ["s_waitcnt lgkmcnt(8)", "v_mov_b32_e32 v200, v0"])
    assert findings(body(0))          # the taken branch skips the eighth read
    assert not findings(body(1))      # eight on the taken path, nine on the other


def test_younger_smem_does_not_retire_lds():
    for smem in ("s_load_dword s8, s[0:1], 0x0", "s_memtime s[8:9]", "s_memrealtime s[8:9]"):
        body = ["ds_read_b128 v[0:3], v4"] + reads(7) + [smem, "s_waitcnt lgkmcnt(8)", "v_mov_b32_e32 v200, v0"]
        assert findings(body), smem
        body = ["ds_read_b128 v[0:3], v4"] + reads(8) + [smem, "s_waitcnt lgkmcnt(8)", "v_mov_b32_e32 v200, v0"]
        assert not findings(body), smem
    # an SMEM result itself is ready only at lgkmcnt(0), however many LDS ops follow it
    body = ["s_memtime s[8:9]"] + reads(4) + ["s_waitcnt lgkmcnt(1)", "s_mov_b32 s10, s8"]
    assert findings(body)
    assert not findings(["s_memtime s[8:9]"] + reads(4) + ["s_waitcnt lgkmcnt(0)", "s_mov_b32 s10, s8"])


def test_vmcnt_counts_loads_stores_and_lds_dma_in_order():
    younger = ["global_store_dword v[12:13], v20, off", "global_load_lds_dwordx4 v[12:13], off",
               "buffer_load_dword v21, s[8:11], 0 offen lds", "buffer_store_dword v22, v23, s[8:11], 0 offen",
               "global_atomic_add_f32 v[12:13], v24, off"]
    head = ["global_load_dwordx4 v[0:3], v[10:11], off"]
    assert not findings(head + younger + ["s_waitcnt vmcnt(5)", "v_mov_b32_e32 v30, v0"])
    assert findings(head + younger + ["s_waitcnt vmcnt(6)", "v_mov_b32_e32 v30, v0"])
    # vmcnt does not retire LDS reads, lgkmcnt does not retire vector-memory loads
    assert findings(head + ["s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v30, v0"])
    assert findings(["ds_read_b32 v0, v4", "s_waitcnt vmcnt(0)", "v_mov_b32_e32 v30, v0"])
    # an LDS-DMA load names its address, not a destination: reading that register is fine
    assert not findings(["buffer_load_dword v21, s[8:11], 0 offen lds", "v_mov_b32_e32 v30, v21"])


def test_returning_atomics_are_loads():
    assert findings(["global_atomic_add_f32 v5, v[12:13], v24, off sc0", "v_mov_b32_e32 v30, v5"])
    assert not findings(["global_atomic_add_f32 v[12:13], v24, off", "v_mov_b32_e32 v30, v24"])
    assert findings(["ds_add_rtn_u32 v5, v1, v2", "v_mov_b32_e32 v30, v5"])


def test_flat_retires_only_when_both_counters_reach_zero():
    head = ["flat_load_dword v0, v[2:3]"]
    assert findings(head + ["s_waitcnt vmcnt(0)", "v_mov_b32_e32 v30, v0"])
    assert findings(head + ["s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v30, v0"])
    assert not findings(head + ["s_waitcnt vmcnt(0) lgkmcnt(0)", "v_mov_b32_e32 v30, v0"])
    assert not findings(head + ["s_waitcnt vmcnt(0)", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v30, v0"])
    assert findings(head + ["global_load_dword v9, v[2:3], off", "s_waitcnt vmcnt(1) lgkmcnt(0)", "v_mov_b32_e32 v30, v0"])
    # a younger flat op is out of order: it does not retire an older in-order load
    assert findings(["global_load_dword v9, v[2:3], off", "flat_load_dword v0, v[2:3]", "s_waitcnt vmcnt(1)",
                     "v_mov_b32_e32 v30, v9"])


def two_deep_loop(exit_wait):
    """Sets A (v[0:3]) and B (v[4:7]): each iteration waits for A, consumes it, re-issues it, then the same for B; the
    loop's back edge carries both sets in flight."""
    return (["ds_read_b128 v[0:3], v40", "ds_read_b128 v[4:7], v41",
             ".LBB0_1:",
             "s_waitcnt lgkmcnt(1)", "v_add_f32_e32 v50, v0, v50", "ds_read_b128 v[0:3], v40",
             "s_waitcnt lgkmcnt(1)", "v_add_f32_e32 v50, v4, v50", "ds_read_b128 v[4:7], v41",
             "s_add_u32 s0, s0, -1", "s_cmp_lg_u32 s0, 0", "s_cbranch_scc1 .LBB0_1"]
            + (["s_waitcnt lgkmcnt(0)"] if exit_wait else []) + ["v_add_f32_e32 v50, v0, v50"])


def test_two_deep_loop_released_in_the_next_iteration():
    assert not findings(two_deep_loop(True), inline={0, 1, 3, 5, 6, 8})
    f = findings(two_deep_loop(False), inline={0, 1, 3, 5, 6, 8})
    assert f and all("v0" in x.text for x in f)
    # a loop whose top waits for the WRONG set (lgkmcnt(2): nothing retired) is caught on the back edge
    body = two_deep_loop(True)
    body[3] = "s_waitcnt lgkmcnt(2)"
    assert findings(body)


def test_both_successors_of_a_conditional_branch():
    taken_bad = ["ds_read_b128 v[0:3], v4", "s_cbranch_scc1 .LBB0_1", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v9, v0",
                 "s_endpgm", ".LBB0_1:", "v_mov_b32_e32 v9, v0"]
    fall_bad = ["ds_read_b128 v[0:3], v4", "s_cbranch_scc1 .LBB0_1", "v_mov_b32_e32 v9, v0", "s_endpgm", ".LBB0_1:",
                "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v9, v0"]
    assert [f.text for f in findings(taken_bad)] == ["v_mov_b32_e32 v9, v0"]
    assert [f.text for f in findings(fall_bad)] == ["v_mov_b32_e32 v9, v0"]
    good = ["ds_read_b128 v[0:3], v4", "s_cbranch_execz .LBB0_1", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v9, v0",
            "s_branch .LBB0_2", ".LBB0_1:", "s_waitcnt lgkmcnt(0)", ".LBB0_2:", "v_mov_b32_e32 v9, v0"]
    assert not findings(good)
    # s_branch is unconditional: the code after it is reached only through its label
    assert not findings(["ds_read_b128 v[0:3], v4", "s_branch .LBB0_1", "v_mov_b32_e32 v9, v0", ".LBB0_1:",
                         "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v9, v0"])


def test_endpgm_ends_the_path():
    body = ["s_cbranch_scc1 .LBB0_1", "ds_read_b128 v[0:3], v4", "s_endpgm", ".LBB0_1:", "v_mov_b32_e32 v9, v0"]
    assert not findings(body)
    body[2] = "s_nop 0"
    assert findings(body)


def test_in_order_vector_loads_may_overwrite_each_other():
    """Two vector-memory loads return in issue order: the younger may target an older one's destination without a wait (the
    compiler relies on this).  Any other writer, or a read, must wait."""
    assert not findings(["global_load_dword v0, v[2:3], off", "global_load_dword v0, v[2:3], off offset:4",
                         "s_waitcnt vmcnt(0)", "v_mov_b32_e32 v9, v0"])
    assert findings(["ds_read_b32 v0, v4", "global_load_dword v0, v[2:3], off"])
    assert findings(["global_load_dword v2, v[2:3], off", "global_load_dword v0, v[2:3], off"])    # reads v2


def test_wait_forms():
    assert W.parse_wait("vmcnt(3) lgkmcnt(0)") == {W.VM: 3, W.LGKM: 0}
    assert W.parse_wait("lgkmcnt(8)") == {W.LGKM: 8}
    assert W.parse_wait("0") == {W.VM: 0, W.LGKM: 0}
    assert W.parse_wait("0xc07f") == {W.VM: 63, W.LGKM: 0}
    assert W.regs_of("v[8:11], v12, a[0:1], s[4:5] sc0 offset:16") == (
        frozenset(range(8, 13)) | {1024, 1025, 2052, 2053})


# ---- the shipped kernels ------------------------------------------------------------------------------------------------------

def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


def makefile_flags():
    """HIPFLAGS (with ARCH = gfx950, no EXTRA) and the per-file FLAGS_<name> of visionllm_amd/csrc/Makefile."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    base = re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, flags=re.M).group(1)
    base = base.replace("$(ARCH)", "gfx950").replace("$(EXTRA)", "").split()
    per = {m.group(1): m.group(2).split() for m in re.finditer(r"^FLAGS_(\w+)\s*=\s*(.*)$", text, flags=re.M)}
    return base, per


@pytest.fixture(scope="module")
def shipped(tmp_path_factory):
    """{file stem: (assembly text, Report)} for every visionllm_amd/csrc/*.hip (device code only, nothing is loaded or run)."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    out_dir = tmp_path_factory.mktemp("isa")
    base, per = makefile_flags()
    assert "--offload-arch=gfx950" in base and "-O3" in base
    names = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))

    def compile_one(name):
        out = out_dir / (name + ".s")
        subprocess.run([hipcc] + base + per.get(name, []) + ["-S", "--cuda-device-only", name + ".hip", "-o", str(out)],
                       check=True, cwd=CSRC, capture_output=True, timeout=900)
        text = out.read_text()
        return name, text, W.analyse(text)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        res = list(pool.map(compile_one, names))
    return {n: (t, r) for n, t, r in res}


def test_shipped_kernels_wait_for_every_load(shipped):
    total = W.Report()
    for name, (_, rep) in shipped.items():
        total.merge(rep)
    lines = [f"{f.kernel}: line {f.line} `{f.text}` touches a destination of line {f.issuer_line} `{f.issuer_text}`"
             f" ({'inline asm' if f.issuer_inline else 'compiler'}) before it is waited for" for f in total.findings]
    assert not lines, "\n".join(lines[:40])
    print(f"\nisa_waits: {total.kernels} kernels, {len(total.inline_load_groups)} inline-asm load groups "
          f"({total.inline_loads} loads, {len(total.split_groups)} released in another asm block), "
          f"{len(total.counted_waits)} counted waits retiring inline-asm loads, {total.compiler_loads} compiler-emitted loads")
    assert total.kernels >= 200 and total.compiler_loads >= 10000


def test_phase_clock_builds_of_msda9_and_dcnv3_are_analysed(shipped):
    """The PROF instantiations put s_memtime inside counted sections: they are compiled and analysed like the others.  Generations 4
    and 6 of the MSDA forward have no clock build: one kernel each, without s_memtime."""
    for name in ("msda_tiled9", "dcnv3_pipe"):
        text, rep = shipped[name]
        fns = W.split_functions(text)
        assert rep.kernels == len(fns) >= 2, name
        assert any(any(x.mnem == "s_memtime" for x in fn.instrs) for fn in fns), name
        assert any(not any(x.mnem == "s_memtime" for x in fn.instrs) for fn in fns), name
    for name in ("msda_tiled4", "msda_tiled6"):
        text, rep = shipped[name]
        fns = W.split_functions(text)
        assert rep.kernels == len(fns) == 1, name
        assert not any(x.mnem == "s_memtime" for x in fns[0].instrs), name


@pytest.mark.parametrize("name", ["msda_tiled9", "dcnv3_pipe", "gemm_skinny", "gemm256p"])
def test_split_inline_load_groups_are_tracked(shipped, name):
    """Floors: a parser regression must not pass by tracking nothing."""
    _, rep = shipped[name]
    assert rep.split_groups, f"{name}: no inline-asm load group issued in one asm block and released in another"
    if name != "gemm256p":
        assert rep.counted_waits, f"{name}: no nonzero counted wait observed retiring inline-asm loads"


def _first_split_read_group(text, rep):
    groups = sorted((lines[0], lines) for key, lines in rep.inline_load_groups.items() if key in rep.split_groups
                    and len(lines) == 8 and all("ds_read_b128" in text.splitlines()[ln - 1] for ln in lines))
    assert groups
    return groups[0][1]


@pytest.mark.parametrize("name", ["msda_tiled9", "dcnv3_pipe"])
def test_mutation_copy_of_an_in_flight_register_is_flagged(shipped, name):
    text, rep = shipped[name]
    assert not rep.findings
    lines = text.splitlines()
    group = _first_split_read_group(text, rep)
    dst = re.search(r"ds_read_b128\s+v\[(\d+):", lines[group[0] - 1]).group(1)
    end = group[-1]                                 # 1-based line of the group's last read; the ;;#ASMEND follows
    assert lines[end].strip() == ";;#ASMEND"
    mutated = lines[:end + 1] + [f"\tv_mov_b32_e32 v255, v{dst}"] + lines[end + 1:]
    found = W.analyse("\n".join(mutated)).findings
    assert any(f.line == end + 2 and f.issuer_inline for f in found), found[:4]


@pytest.mark.parametrize("name", ["msda_tiled9", "dcnv3_pipe"])
def test_mutation_weaker_counted_wait_is_flagged(shipped, name):
    text, rep = shipped[name]
    lines = text.splitlines()
    at = min(ln for k, ln in rep.counted_waits if "lgkmcnt(8)" in lines[ln - 1])
    mutated = list(lines)
    mutated[at - 1] = lines[at - 1].replace("lgkmcnt(8)", "lgkmcnt(9)")
    found = W.analyse("\n".join(mutated)).findings
    assert found and all(f.issuer_inline for f in found), found[:4]
