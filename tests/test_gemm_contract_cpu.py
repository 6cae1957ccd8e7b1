"""CPU: the vllm_gemm_bf16* entries refuse what include/vllm_hip.h's contract excludes BEFORE any launch.

Only refused calls are made (and M == 0, which returns before the gates), with fake non-null pointers: the gates look at values and
dereference nothing, so nothing touches a device.  Every case starts from a call that meets the contract, changes what the case is
about, and asserts VLLM_EINVAL with THAT requirement named in vllm_last_error() (so no other gate fired first).  The cases run on
every entry that has the argument: vllm_gemm_bf16, _sk (NULL scratch), _ln (no folded norm unless the case is about one) and
_residual_save."""
import ctypes

import pytest

from visionllm_amd import _lib

OK, EINVAL = 0, -1
PTR = 1 << 20          # 256-byte aligned, non-null
ENTRIES = ("gemm", "sk", "ln", "save")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def call(entry, **kw):
    """One call of `entry` that meets the contract (64 x 64 x 64, every pointer aligned) with the arguments in `kw` replaced."""
    L = _lib.lib()
    a = dict(X=PTR, W=PTR, bias=PTR, Y=PTR, pre=PTR, M=64, N=64, K=64, ldx=64, ldw=64, ldy=64, epi=3 if entry == "save" else 0, scale=0,
             res=PTR if entry == "save" else 0, ldr=64, P=0, ln_out=0)
    assert set(kw) <= set(a), kw
    a.update(kw)
    head = (vp(a["X"]), vp(a["W"]), vp(a["bias"]), vp(a["Y"]))
    dims = (a["M"], a["N"], a["K"], a["ldx"], a["ldw"], a["ldy"], a["epi"], vp(a["scale"]), vp(a["res"]), a["ldr"])
    if entry == "gemm":
        return L.vllm_gemm_bf16(*head, *dims, a["P"], None)
    if entry == "sk":
        return L.vllm_gemm_bf16_sk(*head, *dims, a["P"], None, 0, None)
    if entry == "ln":
        return L.vllm_gemm_bf16_ln(*head, *dims, vp(a["ln_out"]), None, 0, 0, 1e-6, None, None, None)
    return L.vllm_gemm_bf16_residual_save(*head, vp(a["pre"]), *dims, None)


# (id, entries, changed arguments, substring of the message)
ALL, NOT_SAVE, WITH_P = ENTRIES, ("gemm", "sk", "ln"), ("gemm", "sk")
CASES = [
    ("N_not_multiple_of_4", ALL, dict(N=66, ldy=68), "N=66 must be a multiple of 4"),
    ("K_not_multiple_of_64", ALL, dict(K=100, ldx=104, ldw=104), "K=100 must be a multiple of 64"),
    ("ldx_not_multiple_of_8", ALL, dict(ldx=68), "row strides"),
    ("ldw_not_multiple_of_8", ALL, dict(ldw=68), "row strides"),
    ("ldy_not_multiple_of_4", ALL, dict(ldy=66), "row strides"),
    ("X_8_byte_aligned", ALL, dict(X=PTR + 8), "X and W must be 16-byte aligned"),
    ("W_8_byte_aligned", ALL, dict(W=PTR + 8), "X and W must be 16-byte aligned"),
    ("Y_4_byte_aligned", ALL, dict(Y=PTR + 4), "Y 8-byte aligned"),
    ("Y_8_byte_aligned_fp32_output", NOT_SAVE, dict(Y=PTR + 8, epi=5), "16-byte for fp32 output"),
    ("bias_4_byte_aligned", ALL, dict(bias=PTR + 4), "bias and scale must be 8-byte aligned"),
    ("scale_4_byte_aligned", ALL, dict(epi=3, res=PTR, scale=PTR + 4), "bias and scale must be 8-byte aligned"),
    ("residual_without_res", NOT_SAVE, dict(epi=3, res=0), "residual epilogue needs res"),
    ("residual_save_without_res", ("save",), dict(res=0), "null pointer"),
    ("residual_ldr_not_multiple_of_4", ALL, dict(epi=3, res=PTR, ldr=66), "ldr a multiple of 4"),
    ("residual_res_4_byte_aligned", ALL, dict(epi=3, res=PTR + 4), "residual epilogue needs res (8-byte aligned"),
    ("embed_without_table", WITH_P, dict(epi=4, res=0, P=7), "embed epilogue needs the position table"),
    ("embed_P_zero", WITH_P, dict(epi=4, res=PTR, P=0), "embed epilogue needs the position table"),
    ("embed_P_negative", WITH_P, dict(epi=4, res=PTR, P=-3), "embed epilogue needs the position table"),
    ("embed_ldr_not_multiple_of_4", WITH_P, dict(epi=4, res=PTR, P=7, ldr=66), "ldr a multiple of 4"),
    ("embed_table_4_byte_aligned", WITH_P, dict(epi=4, res=PTR + 4, P=7), "position table (8-byte aligned"),
    ("gelu_bwd_with_bias", NOT_SAVE, dict(epi=6, res=PTR), "GELU-backward epilogue needs"),
    ("gelu_bwd_res_4_byte_aligned", NOT_SAVE, dict(epi=6, bias=0, res=PTR + 4), "GELU-backward epilogue needs"),
    ("gelu_bwd_without_res", NOT_SAVE, dict(epi=6, bias=0, res=0), "GELU-backward epilogue needs"),
    ("residual_save_null_pre", ("save",), dict(pre=0), "null pointer"),
    ("residual_save_pre_4_byte_aligned", ("save",), dict(pre=PTR + 4), "8-byte aligned pre-activation"),
    ("residual_save_other_epilogue", ("save",), dict(epi=0), "the epilogue is VLLM_EPI_RESIDUAL"),
    ("four_wave_variant_not_built", NOT_SAVE, dict(epi=0 | 0x400), "not built"),
    ("four_wave_variant_not_built_residual", ALL, dict(epi=3 | 0x400, res=PTR), "not built"),
    ("unknown_epilogue_7", NOT_SAVE, dict(epi=7), "unknown epilogue 7"),
    ("unknown_epilogue_99_forced_8_phase", NOT_SAVE, dict(epi=99 | 0x200), "unknown epilogue 99"),
    ("folded_norm_N_not_multiple_of_8", ("ln",), dict(N=68, ldy=72, ln_out=PTR, epi=3, res=PTR, ldr=72), "N, ldy multiples of 8"),
    ("negative_M", ALL, dict(M=-1), "bad dims"),
    ("zero_N", ALL, dict(N=0), "bad dims"),
]
PARAMS = [pytest.param(e, kw, msg, id=f"{e}-{name}") for name, entries, kw, msg in CASES for e in entries]


@pytest.mark.parametrize("entry,kw,msg", PARAMS)
def test_refused_before_any_launch(entry, kw, msg):
    rc = call(entry, **kw)
    err = _lib.lib().vllm_last_error().decode()
    assert rc == EINVAL and msg in err, (rc, err)


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_rows_is_ok_and_does_nothing(entry):
    """M == 0 returns VLLM_OK whatever else the call says (the orchestrators pass empty batches through): nothing is read, nothing is
    launched -- fake pointers, and arguments the gates behind it would refuse."""
    assert call(entry, M=0) == OK
    assert call(entry, M=0, K=100) == OK
