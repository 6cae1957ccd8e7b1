"""A caller workspace with guard bytes around it and a chosen content (test_workspace_contract_gpu.py).

The header's contract for every workspace-taking entry: given exactly the bytes its size query answers, aligned as the header says and
no better, a call stays inside them and does not care what was in them.  ``guarded`` builds such a workspace inside one uint8 device
tensor the test owns,

    [front guard 4096 B][skew][nbytes of workspace][back guard]

so that a stray store lands in memory of the test's own and is seen.  Guards and skew bytes hold 0xA5, the workspace bytes hold ``fill``:
    0x00  the clean baseline
    0xFF  every bf16 / fp16 / fp32 word a NaN, every flag non-zero, every int32 -1
    0x3F  finite, plausible values (0.75 in bf16, 1.75 in fp16, 0.747 in fp32), for code that would ``select`` a NaN away
``skew`` is 0 or the least alignment the header promises for the entry (16; 8 for the point-sample backward; 4 for the splice's int32
words): the front guard is a multiple of 256 bytes and the allocator's blocks start 256-byte aligned, so the workspace pointer is then
aligned to ``skew`` and to nothing larger.  Nothing here touches torch.cuda at import."""
import torch

GUARD = 0xA5
FRONT = 4096
HOSTILE = 0xFF    # NaN in every floating type, non-zero flags, -1 ints
PLAUSIBLE = 0x3F
MIB = 1 << 20


def back_guard_bytes(widest_row_bytes=0):
    """max(1 MiB, 256 x the widest row the case writes): a whole stray 256-row tile lands inside the guard, not only a stray element."""
    return max(MIB, 256 * int(widest_row_bytes))


def guarded(nbytes, fill, skew=0, widest_row_bytes=0, device="cuda:0"):
    """-> (ptr, nbytes, check).  ``ptr`` is the integer device address of the ``nbytes`` workspace bytes (pass it as a c_void_p), ``check()``
    synchronises and asserts that every guard byte is still 0xA5.  ``check.buffer`` is the whole tensor (it keeps the memory alive) and
    ``check.workspace`` the uint8 view of the workspace bytes, for a test that refills them between two calls."""
    assert skew in (0, 4, 8, 16) and nbytes >= 0
    back = back_guard_bytes(widest_row_bytes)
    buf = torch.full((FRONT + skew + nbytes + back,), GUARD, dtype=torch.uint8, device=device)
    lo, hi = FRONT + skew, FRONT + skew + nbytes
    buf[lo:hi] = fill
    assert buf.data_ptr() % 256 == 0
    ptr = buf.data_ptr() + lo
    assert skew == 0 or (ptr % skew == 0 and ptr % (2 * skew) != 0)

    def check():
        torch.cuda.synchronize()
        front, behind = buf[:lo] != GUARD, buf[hi:] != GUARD
        if bool(behind.any()):
            off = int(behind.nonzero()[0])
            raise AssertionError(f"workspace overrun: byte {off} behind the workspace's end ({nbytes} bytes, skew {skew}) was written "
                                 f"({int(behind.sum())} guard bytes changed)")
        if bool(front.any()):
            off = int(front.nonzero()[-1])
            raise AssertionError(f"workspace underrun: byte {lo - off} in front of the workspace's start was written "
                                 f"({int(front.sum())} guard bytes changed)")

    check.buffer = buf
    check.workspace = buf[lo:hi]
    return ptr, nbytes, check
