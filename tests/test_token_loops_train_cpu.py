"""Host side of the token loops' training path: the two row kernels are declared and exported and refuse bad arguments without a device
(a refused call launches nothing); the default path of the four functions still refuses inputs that require grad; the pure-torch
bookkeeping (owner map, CSR lists) agrees with a brute-force Python loop."""
import ctypes
import random

import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import splice as S

SEG, MASKED = "vllm_rows_segment_sum_bf16", "vllm_copy_rows_masked_bf16"
V, LONG, INT = ctypes.c_void_p, ctypes.c_long, ctypes.c_int


def _err():
    return _lib.lib().vllm_last_error().decode()


def test_the_two_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    for name in (SEG, MASKED):
        assert name in protos and hasattr(_lib.lib(), name), name
    assert protos[SEG] == (INT, [V, LONG, V, V, LONG, V, LONG, INT, V])
    assert protos[MASKED] == (INT, [V, V, V, LONG, INT, V])
    src = open(_lib.HEADER).read()
    for name, cites in ((SEG, ("432-527", "775-787", "644-681")), (MASKED, ("688-698", "432-527"))):
        doc = src[src.index("Backward of those four loops"):src.index("int " + name)]
        assert all(c in doc for c in cites), name            # each cites the reference statements whose autograd it replaces


def _host_pointers():
    buf = (ctypes.c_uint16 * 512)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return buf, ctypes.c_void_p(base), ctypes.c_void_p(base + 8)


def test_segment_sum_refusals_need_no_device():
    fn = getattr(_lib.lib(), SEG)
    keep, p, odd = _host_pointers()
    assert fn(p, 4, p, p, 4, p, 2, 12, None) == -1 and "C must be a positive multiple of 8" in _err()
    assert fn(p, 4, p, p, 4, p, 2, 0, None) == -1 and "C must be a positive multiple of 8" in _err()
    assert fn(p, 4, p, p, 4, p, 2, -8, None) == -1 and "C must be a positive multiple of 8" in _err()
    for sizes in ((-1, 4, 2), (4, -1, 2), (4, 4, -2)):
        assert fn(p, sizes[0], p, p, sizes[1], p, sizes[2], 8, None) == -1 and "must not be negative" in _err()
    assert fn(odd, 4, p, p, 4, p, 2, 8, None) == -1 and "16-byte aligned" in _err()
    assert fn(p, 4, p, p, 4, odd, 2, 8, None) == -1 and "16-byte aligned" in _err()
    assert fn(p, 4, None, p, 4, p, 2, 8, None) == -1 and "null seg_ptr or dst" in _err()
    assert fn(p, 4, p, p, 4, None, 2, 8, None) == -1 and "null seg_ptr or dst" in _err()
    assert fn(None, 4, p, p, 4, p, 2, 8, None) == -1 and "null src or src_idx" in _err()
    assert fn(p, 4, p, None, 4, p, 2, 8, None) == -1 and "null src or src_idx" in _err()
    assert fn(None, 0, None, None, 0, None, 0, 8, None) == 0                       # dst_rows == 0: accepted, nothing launched
    assert fn(p, 4, p, p, 4, p, 0, 8, None) == 0


def test_masked_copy_refusals_need_no_device():
    fn = getattr(_lib.lib(), MASKED)
    keep, p, odd = _host_pointers()
    assert fn(p, p, p, 2, 12, None) == -1 and "C must be a positive multiple of 8" in _err()
    assert fn(p, p, p, 2, 0, None) == -1 and "C must be a positive multiple of 8" in _err()
    assert fn(p, p, p, -2, 8, None) == -1 and "must not be negative" in _err()
    assert fn(odd, p, p, 2, 8, None) == -1 and "16-byte aligned" in _err()
    assert fn(p, p, odd, 2, 8, None) == -1 and "16-byte aligned" in _err()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert fn(*args, 2, 8, None) == -1 and "null src, zero_row or dst" in _err()
    assert fn(None, None, None, 0, 8, None) == 0                                   # rows == 0: accepted, nothing launched


def test_the_default_path_still_refuses_to_cut_gradients():
    C = 16
    emb = torch.zeros(1, 8, C, dtype=torch.bfloat16)
    ids = torch.tensor([[5, 1, 2, 3, 4, 9, 9, 9]])
    grad = lambda *shape: torch.zeros(*shape, dtype=torch.bfloat16, requires_grad=True)   # noqa: E731
    with pytest.raises(RuntimeError, match="forward-only"):
        S.splice_emb_tokens(ids, emb.clone(), {5: grad(2, C)}, 100, 2)
    with pytest.raises(RuntimeError, match="forward-only"):
        S.splice_emb_tokens(ids, emb.clone(), {5: grad(2, C)}, 100, 2, native_backward=False)
    with pytest.raises(RuntimeError, match="forward-only"):
        S.gather_emb_hidden_states(grad(1, 8, C), ids, 1, 2, native_backward=False)
    with pytest.raises(RuntimeError, match="forward-only"):
        S.splice_region_tokens(emb.clone(), ids, 9, grad(3, C), native_backward=False)
    with pytest.raises(RuntimeError, match="forward-only"):
        S.gather_region_image_features([grad(2, 5, C)] * 3, [2], [1], native_backward=False)


def _check_csr(seg_ptr, src_idx, want):
    """``want``: per destination row, the list of its source rows in order."""
    assert seg_ptr.dtype == src_idx.dtype == torch.int64 and seg_ptr.numel() == len(want) + 1 and int(seg_ptr[0]) == 0
    sp, si = seg_ptr.tolist(), src_idx.tolist()
    assert [si[sp[d]:sp[d + 1]] for d in range(len(want))] == want


def test_segments_keep_the_order_of_the_terms():
    keys = torch.tensor([3, 0, 3, 5, 0, 3])
    rows = torch.tensor([10, 11, 12, 13, 14, 15])
    _check_csr(*S._segments(keys, rows, 7), [[11, 14], [], [], [10, 12, 15], [], [13], []])
    _check_csr(*S._segments(keys[:0], rows[:0], 3), [[], [], []])


@pytest.mark.parametrize("seed", range(4))
def test_owner_map_and_its_segments_against_a_python_loop(seed):
    """Random ids with three tools (the first two share a table, the last has no token at all: an empty tool); seed 0 also plants a
    second tool's block inside the first tool's (the later tool wins the rows they share)."""
    rnd = random.Random(seed)
    B, L, NE, NG = 3, 60, 4, 2
    ids = torch.tensor([[rnd.randrange(0, 50) for _ in range(L)] for _ in range(B)])
    tools = [(90, NE, 0), (91, NE, 0), (92, NG, NE), (93, NE, NE + NG)]                  # (tool id, rows, first global table row)
    for b in range(B):
        for k, (tid, n, _) in enumerate(tools[:3]):
            if rnd.random() < 0.8:
                ids[b, 3 + 12 * k + rnd.randrange(0, 5)] = tid
    if seed == 0:
        ids[0, 3:40] = 1
        ids[0, 5], ids[0, 7] = 90, 92                                                    # 92's block (8, 9) lies inside 90's (6..9)
    writes = []
    for tid, n, base in tools:
        pos = torch.nonzero(ids == tid, as_tuple=False)
        if pos.numel():
            writes.append((*S._emb_block_rows(pos, L, n), base))
    owner = S._emb_owner_map(B * L, writes)
    want = [-1] * (B * L)
    for tid, n, base in tools:                                                           # the reference's order: tool by tool
        for b in range(B):
            for p in range(L):
                if int(ids[b, p]) == tid:
                    for j in range(n):
                        want[b * L + p + 1 + j] = base + j
    assert owner.dtype == torch.int32 and owner.tolist() == want
    if seed == 0:
        assert want[6:10] == [0, 1, NE, NE + 1]
    n_rows = 2 * NE + NG
    zero_row, seg_ptr, src_idx = S._emb_segments(owner, n_rows)
    assert zero_row.dtype == torch.uint8 and zero_row.tolist() == [int(w >= 0) for w in want]
    _check_csr(seg_ptr, src_idx, [[i for i, w in enumerate(want) if w == r] for r in range(n_rows)])
    assert int(seg_ptr[NE + NG]) == int(seg_ptr[-1])                                     # the empty tool's rows: empty segments


def test_region_segments_against_a_python_loop():
    tiles = S.region_tile_index([5, 1, 3], [2, 0, 3])                                    # regions 0, 1 read tile 4; 2, 3, 4 read tile 8
    n_tiles, S1 = 9, 1 + 3
    T = S1 - 1
    want = [[] for _ in range(n_tiles * S1)]
    for r, tile in enumerate(tiles):
        for t in range(T):
            want[tile * S1 + 1 + t].append(r * T + t)
    _check_csr(*S._region_segments(torch.tensor(tiles), n_tiles, S1), want)
    assert want[4 * S1] == [] and want[4 * S1 + 1] == [0, 3] and want[8 * S1 + 3] == [8, 11, 14]
