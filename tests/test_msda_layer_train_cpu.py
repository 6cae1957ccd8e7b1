"""CPU: what the deformable-attention layer's training entries promise without a GPU -- the host-only size queries, the ctypes mirror,
the predicate -- and the yardstick of the GPU tests tied to the reference's own run (msda_layer_train_inputs.py)."""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import msda_layer_train_inputs as T
from conftest import load_golden
from oracle import msda as O
from visionllm_amd import _lib
from visionllm_amd import ms_deform_attn as A

PTR = 1 << 20


def _desc(C=256, M=8, L=4, P=4, ref_dim=2, weights=True):
    d = _lib.VllmMsdaLayerDesc()
    d.d_model, d.n_heads, d.n_levels, d.n_points, d.ref_dim = C, M, L, P, ref_dim
    if weights:
        for n in T.LINEARS:
            setattr(d, n + "_w", PTR)
            setattr(d, n + "_b", PTR)
    return d


QUERIES = ("vllm_msda_layer_saved_bytes", "vllm_msda_layer_forward_train_workspace_bytes", "vllm_msda_layer_backward_workspace_bytes")


@pytest.mark.parametrize("name", QUERIES)
def test_size_queries_are_host_only_monotonic_and_refuse_bad_descriptors(name):
    L = _lib.lib()
    fn = getattr(L, name)
    d = _desc()
    base = fn(ctypes.byref(d), 2, 300, 1000)
    assert base > 0 and base % 256 == 0
    assert fn(ctypes.byref(d), 0, 0, 0) >= 0
    for big in ((3, 300, 1000), (2, 301, 1000), (2, 300, 1001), (2, 3000, 1000), (2, 300, 10000), (8, 300, 1000)):
        if name == "vllm_msda_layer_forward_train_workspace_bytes" and big[:2] == (2, 300):
            assert fn(ctypes.byref(d), *big) == base      # (the fp32 operator output: query rows only)
        else:
            assert fn(ctypes.byref(d), *big) >= base, big
    assert fn(ctypes.byref(d), 8, 300, 1000) > base and fn(ctypes.byref(d), 2, 3000, 1000) > base
    if name != "vllm_msda_layer_forward_train_workspace_bytes":
        assert fn(ctypes.byref(d), 2, 300, 10000) > base
    assert fn(None, 2, 300, 1000) < 0
    for bad in (_desc(C=250), _desc(M=7), _desc(ref_dim=3), _desc(L=0), _desc(P=0), _desc(weights=False)):
        assert fn(ctypes.byref(bad), 2, 300, 1000) < 0
    assert fn(ctypes.byref(d), -1, 300, 1000) < 0 and fn(ctypes.byref(d), 2, -1, 1000) < 0 and fn(ctypes.byref(d), 2, 300, -1) < 0


def test_saved_bytes_is_the_four_tensors_of_the_header():
    """value fp32 [B S, C], locations fp32 [R, 2 M L P], weights fp32 [R, M L P], operator output bf16 [R, C]; pieces of 256 bytes"""
    a256 = lambda x: (x + 255) & ~255
    for (Bn, Lq, S), (C, M, L, P) in (((2, 50, 252), (256, 8, 3, 4)), ((1, 900, 12240), (256, 8, 4, 4)), ((3, 7, 11), (64, 2, 1, 8))):
        d = _desc(C=C, M=M, L=L, P=P)
        R, MLP = Bn * Lq, M * L * P
        want = a256(Bn * S * C * 4) + a256(R * MLP * 8) + a256(R * MLP * 4) + a256(R * C * 2)
        assert _lib.lib().vllm_msda_layer_saved_bytes(ctypes.byref(d), Bn, Lq, S) == want


def test_backward_workspace_holds_the_concatenated_query_linears():
    """M L P = 96 (the 3-level pixel decoder): 288 columns padded to 320, so the stacked weight and its gradient are [320, C]"""
    assert T.npad(8, 3, 4) == 320 and T.npad(4, 2, 4) == 128 and T.npad(8, 4, 4) == 384 and T.npad(8, 4, 8) == 768
    d = _desc(L=3)
    need = _lib.lib().vllm_msda_layer_backward_workspace_bytes(ctypes.byref(d), 2, 50, 252)
    R, C, N, VS, MLP = 100, 256, 320, 504, 96
    least = N * C * 2 * 3 + R * C * 4 + VS * C * 4 + R * MLP * 12 + R * N * 2 + N * 2 + VS * C * 2
    assert need >= least


def test_refused_calls_return_einval_before_any_device_work():
    """fake pointers: the gates look at values only.  A short / misaligned / NULL workspace or saved memory, a misaligned operand, a bias
    gradient without its weight's."""
    L = _lib.lib()
    p = ctypes.c_void_p(PTR)
    d = _desc(L=3)
    dims = (2, 50, 252)
    ns, nf, nb = (getattr(L, q)(ctypes.byref(d), *dims) for q in QUERIES)
    g = _lib.VllmMsdaLayerGrads(**{n: PTR for n, _ in _lib.VllmMsdaLayerGrads._fields_})
    v16 = ctypes.c_int(7)

    def fwd(saved=PTR, nsaved=ns, ws=PTR, nws=nf, query=PTR, desc=d):
        return L.vllm_msda_layer_forward_train(ctypes.byref(desc), ctypes.c_void_p(query), p, p, None, p, p, *dims, p, ctypes.c_void_p(saved),
                                               nsaved, ctypes.byref(v16), ctypes.c_void_p(ws) if ws else None, nws, None)

    def bwd(saved=PTR, nsaved=ns, ws=PTR, nws=nb, gout=PTR, grads=g, v=0, desc=d):
        return L.vllm_msda_layer_backward(ctypes.byref(desc), p, p, p, None, p, p, *dims, ctypes.c_void_p(saved), nsaved, v,
                                          ctypes.c_void_p(gout), p, p, ctypes.byref(grads), ctypes.c_void_p(ws) if ws else None, nws, None)

    for call in (fwd, bwd):
        need = nf if call is fwd else nb
        for kw, word in ((dict(nws=need - 1), "workspace"), (dict(ws=PTR + 8), "workspace"), (dict(ws=0), "workspace"),
                         (dict(nsaved=ns - 1), "saved"), (dict(saved=PTR + 8), "saved"), (dict(desc=_desc(C=96)), "d_model")):
            assert call(**kw) == -1, kw
            assert word in L.vllm_last_error().decode(), (kw, L.vllm_last_error())
    assert fwd(query=PTR + 8) == -1 and "aligned" in L.vllm_last_error().decode()
    assert v16.value == 7, "a refused forward leaves the out-parameter alone"
    assert bwd(gout=PTR + 8) == -1 and "aligned" in L.vllm_last_error().decode()
    lone_bias = _lib.VllmMsdaLayerGrads(value_proj_b=PTR)
    assert bwd(grads=lone_bias) == -1 and "bias" in L.vllm_last_error().decode()
    assert bwd(v=2) == -1 and "value_is_bf16" in L.vllm_last_error().decode()
    enc = (2, 252, 252)                                             # Lq == S: the value is never bf16
    nb_enc = L.vllm_msda_layer_backward_workspace_bytes(ctypes.byref(d), *enc)
    ns_enc = L.vllm_msda_layer_saved_bytes(ctypes.byref(d), *enc)
    rc = L.vllm_msda_layer_backward(ctypes.byref(d), p, p, p, None, p, p, *enc, p, ns_enc, 1, p, p, p, ctypes.byref(g), p, nb_enc, None)
    assert rc == -1 and "value_is_bf16" in L.vllm_last_error().decode()


def test_ctypes_mirror_matches_the_header():
    src = open(_lib.HEADER).read()
    m = re.search(r"typedef struct VllmMsdaLayerGrads \{(.*?)\} VllmMsdaLayerGrads;", src, flags=re.S)
    assert m, "VllmMsdaLayerGrads is not declared"
    names = re.findall(r"\*\s*(\w+)", re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S))
    assert names == [n for n, _ in _lib.VllmMsdaLayerGrads._fields_]
    assert names == [f"{lin}_{k}" for lin in T.LINEARS for k in ("w", "b")]
    assert ctypes.sizeof(_lib.VllmMsdaLayerGrads) == _lib.lib().vllm_msda_layer_grads_sizeof() == 64
    _lib.check_struct_layouts()
    protos = _lib.parse_header()
    for name in QUERIES + ("vllm_msda_layer_forward_train", "vllm_msda_layer_backward", "vllm_msda_prep_backward_f32",
                           "vllm_f32_to_bf16_masked", "vllm_bf16_to_f32", "vllm_msda_layer_grads_sizeof"):
        assert name in protos, name
    assert len(protos["vllm_msda_layer_forward_train"][1]) == 17 and len(protos["vllm_msda_layer_backward"][1]) == 20
    assert _lib.header_abi_version() == 2 == _lib.lib().vllm_abi_version()
    for name in ("vllm_msda_layer_forward_train", "vllm_msda_layer_backward", "vllm_msda_prep_backward_f32", "vllm_bf16_to_f32"):
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + name + r"\s*\(", src, flags=re.S), f"no 'Alignment' line directly above {name}"


def _module(dtype=torch.bfloat16):
    return A.MSDeformAttn(d_model=64, n_levels=2, n_heads=2, n_points=4).to(dtype)


def test_predicate_refuses_cpu_fp32_mixed_dtypes_and_reference_point_gradients(monkeypatch):
    mod = _module()
    lin = (mod.value_proj, mod.sampling_offsets, mod.attention_weights, mod.output_proj)
    q, x = torch.zeros(1, 3, 64, dtype=torch.bfloat16), torch.zeros(1, 5, 64, dtype=torch.bfloat16)
    assert not A.msda_layer_train_ok(q, x, *lin)                                   # CPU tensors
    # the conditions on dtypes and sizes, without a device: `is_cuda` is all the CPU tensors above fail
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert A.msda_layer_train_ok(q, x, *lin)
    assert not A.msda_layer_train_ok(q.float(), x.float(), *lin)               # fp32 inputs
    assert not A.msda_layer_train_ok(q, x.float(), *lin)                       # mixed inputs
    f32 = _module(torch.float32)
    assert not A.msda_layer_train_ok(q, x, f32.value_proj, f32.sampling_offsets, f32.attention_weights, f32.output_proj)
    mixed = _module()
    mixed.sampling_offsets.bias.data = mixed.sampling_offsets.bias.data.float()   # the modules' fp32 grid-init bias
    assert not A.msda_layer_train_ok(q, x, mixed.value_proj, mixed.sampling_offsets, mixed.attention_weights, mixed.output_proj)
    ref = torch.rand(1, 3, 2, 2)
    assert A.msda_layer_train_ok(q, x, *lin, reference_points=ref)
    assert not A.msda_layer_train_ok(q, x, *lin, reference_points=ref.requires_grad_(True))
    assert not A.msda_layer_train_ok(torch.zeros(1, 3, 96, dtype=torch.bfloat16), x, *lin)   # d_model % 64


def test_modules_default_to_the_composed_path():
    import types
    cfg = types.SimpleNamespace(d_model=64, num_feature_levels=2, disable_custom_kernels=False)
    mods = (A.MSDeformAttn(64, 2, 2, 4), A.MSDeformAttnKeyAware(64, 2, 2, 4), A.MultiScaleDeformableAttention(64, 2, 2, 4),
            A.MultiScaleDeformableAttentionOptimized(64, 2, 2, 4), A.GroundingDinoMultiscaleDeformableAttention(cfg, 2, 4))
    for m in mods:
        assert m.native_training is False, type(m).__name__


@pytest.mark.parametrize("tag", ["unipose_ref2", "unipose_ref4", "unipose_ref4_norm"])
def test_truth_forward_is_the_layer_oracle_on_the_reference_run(tag):
    g = load_golden("msda_layer.npz")
    M, L, P = int(g["n_heads"]), int(g["n_levels"]), int(g["n_points"])
    four_d = bool(g[f"{tag}.use4d"])
    params = {n: (g[f"{tag}.sd.{n}.weight"], g[f"{tag}.sd.{n}.bias"]) for n in T.LINEARS}
    want, _, _ = O.layer_forward(g[f"{tag}.query"], g[f"{tag}.ref"], g[f"{tag}.src"], g["shapes"], g["lsi"], g[f"{tag}.mask"], params, M, L, P,
                                 use_4d_normalizer=four_d)
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    p = {f"{n}.{k}": t64(g[f"{tag}.sd.{n}.{k}"]) for n in T.LINEARS for k in ("weight", "bias")}
    got = T.layer(p, t64(g[f"{tag}.query"]), t64(g[f"{tag}.ref"]), t64(g[f"{tag}.src"]), torch.from_numpy(g["shapes"]),
                  torch.from_numpy(g[f"{tag}.mask"]).bool(), M, P, four_d)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(got.numpy(), g[f"{tag}.out_f64"], rtol=2e-6, atol=2e-6)     # (the reference's fp32 operator: test_oracle_msda.py)


@pytest.mark.parametrize("ref_dim,four_d", [(2, False), (4, False), (4, True)])
@pytest.mark.parametrize("L,P", [(3, 4), (4, 8)])
def test_prep_backward_formula_is_autograd_of_softmax_and_sampling_locations(ref_dim, four_d, L, P):
    R, M = 9, 2
    gl, gw, _, ref, shapes = T.prep_case(R, M, L, P, ref_dim)
    g = torch.Generator().manual_seed(L * P + ref_dim)
    off = (torch.randn(R, M, L, P, 2, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    logit = (torch.randn(R, M, L * P, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    w = F.softmax(logit, -1)
    loc = A._sampling_locations(ref.double()[None], off[None], shapes, P, four_d)[0]
    ((loc * gl.double()).sum() + (w * gw.double()).sum()).backward()
    d_off, d_logit, mag_off, mag_logit = T.prep_backward_ref(gl, gw, w.detach(), ref, shapes, P, four_d)
    torch.testing.assert_close(d_off, off.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(d_logit, logit.grad, rtol=1e-11, atol=1e-14)
    assert (mag_off >= d_off.abs()).all() and (mag_logit >= d_logit.abs() - 1e-15).all()


def test_integer_round_to_nearest_even_is_torchs():
    x = torch.cat([torch.randn(4097) * 3, torch.tensor([0.0, -0.0, 1.00390625, 1.01171875, float("inf"), -float("inf"), 3.3895314e38, 1e-40])])
    assert torch.equal(T.bf16_rne(x), x.to(torch.bfloat16).view(torch.int16))
    assert torch.isnan(T.bf16_rne(torch.tensor([float("nan")])).view(torch.bfloat16)).all()


def test_cases_cover_what_the_gpu_tests_say_they_reach():
    c = {k: T.make_case(k) for k in T.CASES}
    a, b, enc, dec, e = (c[k] for k in sorted(c))
    assert (a["L"], T.npad(a["M"], a["L"], a["P"])) == (3, 320) and a["ref_dim"] == 4
    assert T.npad(b["M"], b["L"], b["P"]) == 128 and b["four_d"]
    assert enc["Lq"] == enc["S"] >= 4096 and enc["C"] // enc["M"] == 32 and enc["P"] == 4      # the MFMA backward's shape
    assert dec["Lq"] == 900 != dec["S"] and B_rows(dec) >= 4096                                # the streaming value GEMM: bf16 value
    assert (e["P"], e["L"]) == (8, 4) and e["padding_mask"] is None
    for k in c.values():
        assert k["padding_mask"] is None or (k["padding_mask"][-1].any() and not k["padding_mask"][0].any())


def B_rows(case):
    return T.B * case["S"]
