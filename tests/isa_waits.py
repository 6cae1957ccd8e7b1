"""Static check of gfx950 device assembly: is every load's destination waited for before anything touches it?

Inline-asm loads (`asm volatile("ds_read_b128 ...")`) are invisible to the compiler's wait insertion: it treats their outputs as
ready when the statement ends, and only the kernel's own `s_waitcnt` makes them so.  This module reads the `.s` text that
`hipcc -S --cuda-device-only` writes, follows each kernel's control-flow graph, and reports every instruction that names a
register of a load that may still be in flight on some path.  Compiler-emitted loads go through the same analysis: the compiler
inserts its waits by the same rules, so they must come out clean too, which validates the counter model on real code.

Counter model (gfx950):
  vmcnt    vector-memory loads, stores, atomics and LDS-DMA, retired in issue order;
  lgkmcnt  LDS operations (ds_*, returning or not) in issue order; SMEM and s_memtime / s_memrealtime also count but return
           out of order, so they never help retire an LDS op, and an SMEM op retires only at lgkmcnt(0);
  flat_*   counts on both counters, out of order: retired once vmcnt(0) and lgkmcnt(0) have both been seen.
`s_waitcnt vmcnt(N)` retires an in-order op once at least N younger ops of its counter were issued after it on every path.

Plain Python, no dependencies.  `analyse(text)` returns a Report.
"""
import re
from collections import namedtuple

VM, LGKM, SMEM, FLAT = "vm", "lgkm", "smem", "flat"
CAP = {VM: 63, LGKM: 15}           # counter widths on gfx9 (6-bit vmcnt, 4-bit lgkmcnt)
_FLAT_VM, _FLAT_LGKM = 1, 2

Finding = namedtuple("Finding", "kernel line text issuer_line issuer_text issuer_inline")
Instr = namedtuple("Instr", "line text mnem ops regs inline block")

_LABEL = re.compile(r"^([.\w$]+):")
_REG_RANGE = re.compile(r"(?<![\w.$])([vas])\[(\d+):(\d+)\]")
_REG_ONE = re.compile(r"(?<![\w.$])([vas])(\d+)(?![\w$])")
_REG_BASE = {"v": 0, "a": 1024, "s": 2048}
_WAIT_FIELD = re.compile(r"(vmcnt|lgkmcnt|expcnt)\((\d+)\)")


def regs_of(ops):
    """Register ids named in an operand string: v0..v511 -> 0.., a0.. -> 1024.., s0.. -> 2048.."""
    out = set()
    for k, lo, hi in _REG_RANGE.findall(ops):
        out.update(range(_REG_BASE[k] + int(lo), _REG_BASE[k] + int(hi) + 1))
    for k, n in _REG_ONE.findall(_REG_RANGE.sub(" ", ops)):
        out.add(_REG_BASE[k] + int(n))
    return frozenset(out)


def first_operand_regs(ops):
    return regs_of(ops.split(",", 1)[0])


def classify(mnem, ops):
    """(counter, returns_data) of a memory instruction, or None.  counter is VM / LGKM / SMEM / FLAT."""
    if mnem.startswith("ds_"):
        if mnem.startswith(("ds_nop", "ds_gws", "ds_append", "ds_consume")):
            return (LGKM, mnem.startswith(("ds_append", "ds_consume")))
        returns = (mnem.startswith(("ds_read", "ds_bpermute", "ds_permute", "ds_swizzle")) or "_rtn" in mnem
                   or mnem.startswith(("ds_wrxchg", "ds_cmpst_rtn")))
        return (LGKM, returns)
    if mnem.startswith(("buffer_", "global_", "scratch_")):
        lds_dma = "_lds_" in mnem or re.search(r"(?:^|\s)lds(?:\s|$)", ops) is not None
        if lds_dma:
            return (VM, False)
        if "_load" in mnem:
            return (VM, True)
        if "_atomic" in mnem:       # returning form: sc0 (glc before gfx940)
            return (VM, re.search(r"(?:^|\s)(sc0|glc)(?:\s|$)", ops) is not None)
        return (VM, False)          # stores, wbl2 / inv
    if mnem.startswith("flat_"):
        returns = "_load" in mnem or ("_atomic" in mnem and re.search(r"(?:^|\s)(sc0|glc)(?:\s|$)", ops) is not None)
        return (FLAT, returns)
    if mnem.startswith(("s_load", "s_buffer_load", "s_scratch_load")) or mnem in ("s_memtime", "s_memrealtime"):
        return (SMEM, True)
    if mnem.startswith(("s_store", "s_buffer_store", "s_scratch_store", "s_atomic", "s_buffer_atomic", "s_dcache")):
        return (SMEM, False)
    return None


def parse_wait(ops):
    """{counter: N} of an s_waitcnt; counters it does not name are not waited for."""
    ops = ops.strip()
    if re.fullmatch(r"(0x[0-9a-fA-F]+|\d+)", ops):
        v = int(ops, 0)
        return {VM: (v & 0xF) | ((v >> 14) & 0x3) << 4, LGKM: (v >> 8) & 0xF}
    return {(VM if k == "vmcnt" else LGKM): int(n) for k, n in _WAIT_FIELD.findall(ops) if k != "expcnt"}


class Function:
    def __init__(self, name):
        self.name = name
        self.instrs = []                 # Instr
        self.labels = {}                 # label -> index of the next instruction
        self.blocks = []                 # (start, end) instruction index ranges
        self.succ = []                   # block -> [block]


def split_functions(text):
    """Functions of an assembly file: from the `name:` line of each `.type name,@function` to its `.Lfunc_end`."""
    funcs = re.findall(r"^\s*\.type\s+([\w.$]+),\s*@function", text, flags=re.M)
    want = set(funcs)
    out, cur, inline, block_no = [], None, False, 0
    for lineno, raw in enumerate(text.splitlines(), 1):
        s = raw.strip()
        if cur is None:
            m = _LABEL.match(raw)
            if m and m.group(1) in want:
                cur = Function(m.group(1))
            continue
        if raw.startswith(".Lfunc_end"):
            out.append(cur)
            cur = None
            continue
        if s.startswith(";;#ASMSTART"):
            inline, block_no = True, block_no + 1
            continue
        if s.startswith(";;#ASMEND"):
            inline = False
            continue
        m = _LABEL.match(raw)
        if m:
            cur.labels[m.group(1)] = len(cur.instrs)
            s = raw[m.end():].strip()
        s = re.split(r";|//", s, 1)[0].strip()
        if not s or s.startswith("."):
            continue
        mnem, _, ops = s.partition(" ")
        ops = ops.strip()
        cur.instrs.append(Instr(lineno, s, mnem, ops, regs_of(ops), inline, block_no if inline else 0))
    return out


def build_cfg(fn):
    ins = fn.instrs
    starts = {0} | {i for i in fn.labels.values() if i < len(ins)}
    for i, x in enumerate(ins):
        if x.mnem.startswith(("s_branch", "s_cbranch_", "s_setpc", "s_swappc", "s_endpgm")) and i + 1 < len(ins):
            starts.add(i + 1)
    starts = sorted(starts)
    index = {s: b for b, s in enumerate(starts)}
    fn.blocks = [(s, starts[b + 1] if b + 1 < len(starts) else len(ins)) for b, s in enumerate(starts)]
    fn.succ = []
    for b, (s, e) in enumerate(fn.blocks):
        last = ins[e - 1] if e > s else None
        nxt = [b + 1] if b + 1 < len(fn.blocks) else []
        if last is None:
            fn.succ.append(nxt)
            continue
        target = last.ops.split(",")[0].strip() if last.ops else ""
        tgt = [index[fn.labels[target]]] if target in fn.labels and fn.labels[target] in index else []
        if last.mnem.startswith("s_branch"):
            fn.succ.append(tgt)
        elif last.mnem.startswith("s_cbranch_"):
            fn.succ.append(sorted(set(tgt + nxt)))
        elif last.mnem.startswith(("s_endpgm", "s_setpc")):
            fn.succ.append([])
        else:                             # s_swappc: a call returns to the next instruction
            fn.succ.append(nxt)


class Report:
    def __init__(self):
        self.kernels = 0
        self.findings = []                # Finding
        self.inline_load_groups = {}      # (kernel, asm block) that issues loads -> [line of each load]
        self.split_groups = set()         # (kernel, asm block of the loads) retired by a wait outside that block
        self.counted_waits = set()        # (kernel, line of a wait with N > 0 that retired an inline-asm load)
        self.compiler_loads = 0
        self.inline_loads = 0

    def merge(self, other):
        self.kernels += other.kernels
        self.findings += other.findings
        for k in ("inline_load_groups", "split_groups", "counted_waits"):
            getattr(self, k).update(getattr(other, k))
        self.compiler_loads += other.compiler_loads
        self.inline_loads += other.inline_loads


class _Analysis:
    """Forward dataflow over one function.  A state maps the index of an issuing memory instruction to its pending-ness:
    for VM / LGKM ops the minimum number of younger same-counter in-order ops over all paths (capped at the counter width),
    for SMEM None, for FLAT a bit mask of the counters whose zero has not been seen yet."""

    def __init__(self, fn, report):
        self.fn, self.rep = fn, report
        self.kind = {}
        for i, x in enumerate(fn.instrs):
            c = classify(x.mnem, x.ops)
            if c:
                self.kind[i] = c

    def join(self, a, b):
        out = dict(a)
        for k, v in b.items():
            if k not in out:
                out[k] = v
            else:
                cnt = self.kind[k][0]
                out[k] = (out[k] | v) if cnt == FLAT else None if cnt == SMEM else min(out[k], v)
        return out

    def step(self, i, x, st, findings):
        """Apply instruction i to state st (in place).  With findings (a list) also check its operands."""
        fn, kind = self.fn, self.kind
        if x.mnem == "s_waitcnt":
            w = parse_wait(x.ops)
            for k in list(st):
                cnt = kind[k][0]
                if cnt == FLAT:
                    m = st[k]
                    if w.get(VM) == 0:
                        m &= ~_FLAT_VM
                    if w.get(LGKM) == 0:
                        m &= ~_FLAT_LGKM
                    done = m == 0
                    if not done:
                        st[k] = m
                elif cnt == SMEM:
                    done = w.get(LGKM) == 0
                else:
                    n = w.get(cnt)
                    done = n is not None and st[k] >= n
                if done:
                    del st[k]
                    src = fn.instrs[k]
                    if src.inline and kind[k][1]:
                        if x.inline and src.block != x.block:
                            self.rep.split_groups.add((fn.name, src.block))
                        n = w.get(cnt if cnt in (VM, LGKM) else LGKM, 0)
                        if n > 0:
                            self.rep.counted_waits.add((fn.name, x.line))
            return
        if x.mnem.startswith("s_nop"):
            return
        if findings is not None and st and x.regs:
            c = kind.get(i)
            for k in st:
                src = fn.instrs[k]
                if not kind[k][1]:
                    continue
                dst = first_operand_regs(src.ops)
                if dst & x.regs:
                    # two vector-memory loads of one counter return in order: the younger one may overwrite an older one's
                    # destination without a wait (the compiler relies on this); reading it, or any other writer, may not
                    if (c and c[0] == VM and c[1] and kind[k][0] == VM and not (dst & (x.regs - first_operand_regs(x.ops)))):
                        continue
                    findings.append(Finding(fn.name, x.line, x.text, src.line, src.text, src.inline))
        c = kind.get(i)
        if c is None:
            return
        cnt, returns = c
        if cnt in (VM, LGKM):
            cap = CAP[cnt]
            for k in st:
                if kind[k][0] == cnt and st[k] < cap:
                    st[k] += 1
        if returns:
            st[i] = None if cnt == SMEM else (_FLAT_VM | _FLAT_LGKM) if cnt == FLAT else 0

    def run(self):
        fn = self.fn
        nb = len(fn.blocks)
        if nb == 0:
            return []
        state_in = [None] * nb
        state_in[0] = {}
        work, queued = [0], {0}
        while work:
            b = work.pop()
            queued.discard(b)
            st = dict(state_in[b])
            s, e = fn.blocks[b]
            for i in range(s, e):
                self.step(i, fn.instrs[i], st, None)
            for t in fn.succ[b]:
                new = st if state_in[t] is None else self.join(state_in[t], st)
                if new != state_in[t]:
                    state_in[t] = new
                    if t not in queued:
                        queued.add(t)
                        work.append(t)
        findings = []
        for b in range(nb):
            if state_in[b] is None:
                continue                   # unreachable
            st = dict(state_in[b])
            s, e = fn.blocks[b]
            for i in range(s, e):
                self.step(i, fn.instrs[i], st, findings)
        return findings


def analyse(text):
    """Analyse every function of one assembly file."""
    rep = Report()
    for fn in split_functions(text):
        build_cfg(fn)
        rep.kernels += 1
        a = _Analysis(fn, rep)
        for i, (cnt, returns) in a.kind.items():
            if returns:
                x = fn.instrs[i]
                if x.inline:
                    rep.inline_loads += 1
                    rep.inline_load_groups.setdefault((fn.name, x.block), []).append(x.line)
                else:
                    rep.compiler_loads += 1
        seen = set()
        for f in a.run():
            if (f.line, f.issuer_line) not in seen:
                seen.add((f.line, f.issuer_line))
                rep.findings.append(f)
    return rep
