"""Host side of the visual-token splice's native backward: the entry point is declared, documented and exported, refuses bad sizes
without a device (a refused call launches nothing), and the Python wrapper still rejects CPU tensors before anything else."""
import ctypes
import re

import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd.splice import splice_visual_tokens

NAME = "vllm_splice_visual_tokens_backward_bf16"


def _err():
    return _lib.lib().vllm_last_error().decode()


def test_backward_entry_point_is_declared_and_exported():
    protos = _lib.parse_header()
    assert NAME in protos and hasattr(_lib.lib(), NAME)
    restype, argtypes = protos[NAME]
    assert restype is ctypes.c_int and len(argtypes) == 10
    assert argtypes[:2] == [ctypes.c_void_p] * 2 and argtypes[2:7] == [ctypes.c_int] * 5 and argtypes[7:] == [ctypes.c_void_p] * 3
    assert _lib.header_abi_version() == 2


def test_header_comment_carries_the_alignment_line_and_the_departure():
    src = open(_lib.HEADER).read()
    m = re.search(r"/\* Alignment: ([^*]*)\*/\s*int\s+" + NAME + r"\s*\(", src)
    assert m, "no 'Alignment:' line directly above the declaration"
    assert all(w in m.group(1) for w in ("grad_out", "grad_inputs_embeds", "grad_image_features", "16 bytes"))
    doc = src[src.index("Backward of that splice"):m.start()]
    assert "Deliberate departure" in doc and "written completely" in doc


def test_bad_sizes_are_refused_without_a_device():
    fn = getattr(_lib.lib(), NAME)
    buf = (ctypes.c_uint16 * 256)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)
    assert fn(p, p, 1, 4, 1, 2, 12, p, p, None) == -1 and "C must be a positive multiple of 8" in _err()      # C % 8 != 0
    assert fn(p, p, 1, 4, 1, 2, 0, p, p, None) == -1 and "bad sizes" in _err()
    assert fn(p, p, -1, 4, 1, 2, 8, p, p, None) == -1 and "bad sizes" in _err()
    assert fn(p, p, 1, -4, 1, 2, 8, p, p, None) == -1 and "bad sizes" in _err()
    assert fn(p, p, 1, 4, -1, 2, 8, p, p, None) == -1 and "bad sizes" in _err()
    assert fn(p, p, 1, 4, 1, -2, 8, p, p, None) == -1 and "bad sizes" in _err()
    assert fn(p, p, 4097, 4, 1, 2, 8, p, p, None) == -1 and "too many samples" in _err()                       # the forward's limits
    assert fn(p, p, 2, 1 << 30, 1, 2, 8, p, p, None) == -1 and "too many samples" in _err()
    for args in ((odd, p, p), (p, odd, p), (p, p, odd)):
        assert fn(p, args[0], 1, 4, 1, 2, 8, args[1], args[2], None) == -1 and "16-byte aligned" in _err()
    assert fn(None, p, 1, 4, 1, 2, 8, p, p, None) == -1 and "null workspace" in _err()
    assert fn(p, None, 1, 4, 1, 2, 8, p, p, None) == -1 and "null grad_out" in _err()
    assert fn(None, None, 0, 4, 0, 2, 8, None, None, None) == 0                                                # empty sizes
    assert fn(None, None, 1, 4, 1, 2, 8, None, None, None) == 0                                                # no output asked for


@pytest.mark.parametrize("requires_grad", [False, True])
def test_cpu_tensors_are_still_refused(requires_grad):
    emb = torch.zeros(1, 4, 8, dtype=torch.bfloat16)
    feats = torch.zeros(1, 2, 8, dtype=torch.bfloat16, requires_grad=requires_grad)
    x = (emb.clone().requires_grad_(True) * 1) if requires_grad else emb
    with pytest.raises(RuntimeError, match="splice_visual_tokens: inputs_embeds must be a contiguous bf16 CUDA tensor"):
        splice_visual_tokens(x, torch.zeros(1, 4, dtype=torch.int64), 7, feats)
