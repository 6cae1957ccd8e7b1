"""Host side of the attention backward: the bounds of attn_train_inputs.py are ones a faithful implementation meets (the CPU
emulation of the algorithm's rounding points stays inside them on every case), the helper's closed-form expressions are torch's fp64
autograd, the workspace query answers without a device, the entry points are declared and exported, and the hook still refuses a
CPU tensor -- requiring grad or not -- with the message it always had."""
import ctypes

import pytest
import torch

import attn_train_inputs as ati
from visionllm_amd import _lib
from visionllm_amd.flash_attention import FlashAttention

NAMES = ("vllm_attn_fwd_train_qkvpacked_bf16", "vllm_attn_fwd_train_qkvpacked_f16", "vllm_attn_bwd_workspace_bytes",
         "vllm_attn_bwd_qkvpacked_bf16", "vllm_attn_bwd_qkvpacked_f16")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 2, 5, 33, 65, 257])
@pytest.mark.parametrize("name", ati.CASES)
def test_emulation_of_the_rounding_points_is_inside_the_bounds(name, S, D, dtype):
    qkv, dout = ati.case(name, 1, S, 2, D, dtype)
    scale = D ** -0.5
    ref, bound, lse = ati.grad_bounds(qkv, dout, scale, dtype)
    out, lse_e, dqkv = ati.emulate(qkv, dout, scale, dtype)
    assert torch.isfinite(dqkv).all()
    worst, at = ati.worst_factor(dqkv, ref, bound)
    print(f"{name} S{S} D{D} {dtype}: gradient {worst:.3f} of the bound, lse {float((lse_e - lse).abs().max()) / ati.lse_bound(dtype):.3f}")
    assert worst <= 1.0, f"emulation at {worst:.2f} x the gradient bound (element {at})"
    assert float((lse_e - lse).abs().max()) <= ati.lse_bound(dtype)


@pytest.mark.parametrize("name", ati.CASES)
def test_closed_form_is_the_fp64_autograd_of_naive_attn(name):
    S, D = 65, 64
    qkv, dout = ati.case(name, 2, S, 2, D, torch.bfloat16)
    out, g = ati.autograd_grads(qkv, dout, D ** -0.5, torch.float64)
    c = ati.closed_form(qkv, dout, D ** -0.5)
    assert torch.allclose(c["out"], out, rtol=1e-12, atol=1e-13)
    assert torch.allclose(c["dqkv"], g, rtol=1e-10, atol=1e-12)
    # delta two ways: sum_d dO O = sum_j p_ij dP_ij
    do = dout.double().permute(0, 2, 1, 3)
    v = qkv.double()[:, :, 2].permute(0, 2, 1, 3)
    assert torch.allclose(c["delta"], (c["p"] * (do @ v.transpose(-2, -1))).sum(-1), rtol=1e-10, atol=1e-12)
    assert float(c["dS"].sum(-1).abs().max()) < 1e-10      # rows of dS sum to zero


def test_case_fixtures_do_what_they_say():
    D, S = 64, 129
    for name, check in (("key0_dominant", lambda p: float(p[..., 0].min()) > 0.5), ("key0_far_below", lambda p: float(p[..., 0].max()) < 1e-3),
                        ("near_one_hot", lambda p: float(p.max(-1).values.min()) > 0.99),
                        ("spiked_key", lambda p: float(p[..., S // 2].min()) > 0.5)):
        qkv, dout = ati.case(name, 1, S, 2, D, torch.bfloat16)
        assert check(ati.closed_form(qkv, dout, D ** -0.5)["p"]), name


def test_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    L = _lib.lib()
    for n in NAMES:
        assert n in protos and hasattr(L, n), n
    assert protos["vllm_attn_bwd_workspace_bytes"] == (ctypes.c_long, [ctypes.c_int] * 4)
    r, a = protos["vllm_attn_bwd_qkvpacked_bf16"]
    assert r is ctypes.c_int and a == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 2 + \
        [ctypes.c_long, ctypes.c_void_p]
    r, a = protos["vllm_attn_fwd_train_qkvpacked_f16"]
    assert a == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p]
    assert _lib.header_abi_version() == 2


def test_workspace_query_answers_on_the_host():
    L = _lib.lib()
    prev = 0
    for B in (0, 1, 2, 7, 40):
        n = L.vllm_attn_bwd_workspace_bytes(B, 577, 16, 64)
        assert n >= B * 16 * 577 * 4 and n >= prev       # at least the delta buffer [B, H, S] fp32; non-decreasing in B
        prev = n
    assert L.vllm_attn_bwd_workspace_bytes(40, 1025, 25, 128) >= 40 * 25 * 1025 * 4
    assert L.vllm_attn_bwd_workspace_bytes(1, 577, 16, 32) < 0
    assert L.vllm_attn_bwd_workspace_bytes(1, 577, 16, 96) < 0


def test_refused_backward_calls_need_no_device():
    L = _lib.lib()
    buf = (ctypes.c_uint16 * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 8)
    need = L.vllm_attn_bwd_workspace_bytes(1, 4, 1, 64)
    fn = L.vllm_attn_bwd_qkvpacked_bf16
    assert fn(p, p, p, p, 1, 4, 1, 32, 0.125, p, p, 1 << 20, None) == -1 and "head_dim" in L.vllm_last_error().decode()
    assert fn(p, p, p, p, 1, 4, 1, 64, 0.125, p, p, need - 1, None) == -1 and "workspace" in L.vllm_last_error().decode()
    assert fn(p, p, p, p, 1, 0, 1, 64, 0.125, p, p, need, None) == -1
    for i in (0, 1, 3, 9, 10):
        args = [p, p, p, p, 1, 4, 1, 64, 0.125, p, p, need, None]
        args[i] = odd
        assert fn(*args) == -1 and "16-byte aligned" in L.vllm_last_error().decode(), i
    assert fn(None, None, None, None, 0, 4, 1, 64, 0.125, None, None, 0, None) == 0       # B = 0 is accepted
    assert L.vllm_attn_fwd_train_qkvpacked_bf16(p, p, None, 1, 4, 1, 64, 0.125, None) == -1
    assert L.vllm_attn_fwd_train_qkvpacked_bf16(p, p, ctypes.c_void_p(base + 2), 1, 4, 1, 64, 0.125, None) == -1 and \
        "lse must be 4-byte aligned" in L.vllm_last_error().decode()


@pytest.mark.parametrize("requires_grad", [False, True])
def test_hook_refuses_a_cpu_tensor_with_the_same_message(requires_grad):
    qkv = torch.zeros(1, 4, 3, 1, 64, dtype=torch.bfloat16, requires_grad=requires_grad)
    with pytest.raises(RuntimeError, match=r"native FlashAttention: qkv must be a bf16 / fp16 CUDA tensor \[B, S, 3, H, D\]"):
        FlashAttention()(qkv)
    with pytest.raises(NotImplementedError):
        FlashAttention()(qkv, causal=True)
    m = FlashAttention(attention_dropout=0.1).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        m(qkv)


def test_backward_lane_swaps_read_both_results(tmp_path):
    """The scan of tests/test_capi.py::test_attention_lane_swaps_read_both_results on attn_bwd.hip: delta's two halves are combined with
    v_permlane32_swap (halves_sum), whose two results this toolchain has been seen to fold into one in small kernels."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "visionllm_amd", "csrc", "attn_bwd.hip")
    out = tmp_path / "attn_bwd.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(root, "include"), "-S",
                    "--cuda-device-only", src, "-o", str(out)], check=True, cwd=os.path.dirname(src), capture_output=True, timeout=900)
    text = out.read_text()
    lines = [ln for ln in text.splitlines() if ln.strip() and not ln.strip().startswith(";")]
    swaps = 0
    for i, ln in enumerate(lines):
        m = re.search(r"v_permlane32_swap_b32\S*\s+(v\d+), (v\d+)", ln)
        if not m:
            continue
        swaps += 1
        second, verdict = m.group(2), None
        for nxt in lines[i + 1:i + 40]:
            ops = nxt.split(None, 1)
            if len(ops) < 2 or not ops[0].startswith(("v_", "ds_", "global_", "buffer_", "scratch_")):
                continue
            dst, _, srcs = ops[1].partition(",")
            if re.search(r"\b" + second + r"\b", srcs):
                verdict = "read"
                break
            if re.fullmatch(second, dst.strip()):
                verdict = "overwritten"
                break
        assert verdict == "read", f"second result of the swap at instruction {i} ({ln.strip()}) is {verdict}"
    assert swaps > 0
    # no scratch, and no float atomics on any output
    assert not re.search(r"\.private_segment_fixed_size:\s*[1-9]", text)
    assert "atomic" not in "\n".join(lines)
