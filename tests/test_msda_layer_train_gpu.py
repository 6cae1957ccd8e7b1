"""GPU: the deformable-attention layer's native training path -- vllm_msda_layer_forward_train / vllm_msda_layer_backward, their three
elementwise kernels, the autograd node and the module switches (``native_training``).

Yardstick (msda_layer_train_inputs.py, CPU, never the code under test): torch fp64 autograd of the reference's statements is the truth,
torch's bf16 autograd of the same statements (fp32 around the operator) the comparator; every native tensor must be within 1.25 x the
comparator's distance from the truth (the assembled-bf16 margin of test_clip_layer_train_gpu.py / test_vit_layer_train_gpu.py).  The
cases are the smallest that reach each route (msda_layer_train_inputs.CASES), B = 2, the last image partly padded.

grad_value is accumulated with float atomics, so what descends from it (the value_proj gradients, grad_input_flatten) is held to the 1.25
rule only; everything else (the output, grad_query, the output_proj and query-linear gradients) is deterministic and compared bit for bit
between runs."""
import ctypes
import functools
import types

import pytest
import torch
from torch import nn

import msda_layer_train_inputs as T
import test_workspace_contract_gpu as WC
from bounds import P, assert_bound, stream
from visionllm_amd import _lib
from visionllm_amd import ms_deform_attn as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CASE_NAMES = sorted(T.CASES)
FROM_GRAD_VALUE = ("value_proj.weight", "value_proj.bias", "input_flatten")     # float atomics upstream: no bit identity claimed
DETERMINISTIC = tuple(n for n in T.PARAM_NAMES + ("query", "input_flatten") if n not in FROM_GRAD_VALUE)


# ---- 1: the prep-backward kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref_dim,four_d", [(2, 0), (4, 0), (4, 1)])
@pytest.mark.parametrize("L,Pn", [(L, Pn) for L in (1, 2, 3, 4, 8) for Pn in (4, 8)])
def test_prep_backward_kernel_against_fp64(L, Pn, ref_dim, four_d):
    lib = _lib.lib()
    M = 5
    N = T.npad(M, L, Pn)
    MLP = M * L * Pn
    for R in (1, 63, 257):
        gl, gw, w, ref, shapes = T.prep_case(R, M, L, Pn, ref_dim)
        dq = torch.full((R, N), NAN, device=DEV).to(torch.bfloat16)
        dev = [t.to(DEV) for t in (gl, gw, w, ref, shapes)]
        _lib.check(lib.vllm_msda_prep_backward_f32(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), R, M, L, Pn, ref_dim, four_d, P(dq), N,
                                                   stream()), "vllm_msda_prep_backward_f32")
        d_off, d_logit, mag_off, mag_logit = T.prep_backward_ref(gl, gw, w, ref, shapes, Pn, bool(four_d))
        got = dq.cpu()
        tag = f"L{L} P{Pn} ref{ref_dim}{'n' if four_d else ''} R{R}"
        assert_bound(got[:, :2 * MLP].reshape(d_off.shape), d_off, mag_off, f"d_offset {tag}")
        assert_bound(got[:, 2 * MLP:3 * MLP].reshape(d_logit.shape), d_logit, mag_logit, f"d_logit {tag}")
        assert (got[:, 3 * MLP:].view(torch.int16) == 0).all(), f"{tag}: pad columns are not exact zeros"


def test_prep_backward_kernel_wide_pad_and_unaligned_rows():
    """a row stride beyond the least one (every pad column is still the kernel's), and operands that are not 16-byte aligned (the
    any-shape kernel): the same bound"""
    lib = _lib.lib()
    R, M, L, Pn = 63, 8, 4, 4
    MLP = M * L * Pn
    gl, gw, w, ref, shapes = T.prep_case(R, M, L, Pn, 2, seed=3)
    d_off, d_logit, mag_off, mag_logit = T.prep_backward_ref(gl, gw, w, ref, shapes, Pn, False)
    dev = [t.to(DEV) for t in (gl, gw, w, ref, shapes)]
    for N, skew in ((3 * MLP + 128, 0), (3 * MLP + 2, 0), (3 * MLP + 64, 1)):
        store = torch.full((R * N + 8,), NAN, device=DEV).to(torch.bfloat16)
        dq = store[skew:skew + R * N].view(R, N)
        _lib.check(lib.vllm_msda_prep_backward_f32(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), R, M, L, Pn, 2, 0, P(dq), N, stream()),
                   "vllm_msda_prep_backward_f32")
        got = dq.cpu()
        assert_bound(got[:, :2 * MLP].reshape(d_off.shape), d_off, mag_off, f"d_offset N{N} skew{skew}")
        assert_bound(got[:, 2 * MLP:3 * MLP].reshape(d_logit.shape), d_logit, mag_logit, f"d_logit N{N} skew{skew}")
        assert (got[:, 3 * MLP:].view(torch.int16) == 0).all()
        rest = torch.cat([store[:skew], store[skew + R * N:]])
        assert torch.isnan(rest.float()).all(), "the kernel wrote outside its rows"
    assert lib.vllm_msda_prep_backward_f32(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), R, M, L, Pn, 2, 0, P(dq), 3 * MLP - 1,
                                           stream()) == -1


# ---- 2: narrowing with the key-padding mask, widening ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(5, 4097), (4097, 1), (300, 256), (1, 8), (3, 4100)])
def test_masked_narrowing_is_round_to_nearest_even_and_zero_on_masked_rows(rows, cols):
    lib = _lib.lib()
    g = torch.Generator().manual_seed(rows + cols)
    src = torch.randn(rows, cols, generator=g) * 3
    ties = torch.tensor([1.00390625, 1.01171875, -1.00390625, -1.01171875])            # half way between two bf16 numbers: to the even one
    idx = torch.arange(0, rows * cols, 7)
    src.view(-1)[idx] = ties[torch.arange(idx.numel()) % 4]
    mask = torch.rand(rows, generator=g) < 0.3
    mask[-1] = True
    src[mask] = NAN                                                # a padded key's row may hold anything
    src[0, 0] = NAN if not mask[0] else src[0, 0]                  # a live NaN stays a NaN
    want = T.bf16_rne(src)
    want[mask] = 0
    for m in (mask, None):
        dst = torch.full((rows, cols), 7.0, device=DEV).to(torch.bfloat16)
        dm = None if m is None else m.to(DEV).to(torch.uint8)
        _lib.check(lib.vllm_f32_to_bf16_masked(P(src.to(DEV)), P(dst), rows, cols, P(dm), stream()), "vllm_f32_to_bf16_masked")
        got = dst.cpu().view(torch.int16)
        if m is None:
            live = ~torch.isnan(src)
            assert torch.equal(got[live], T.bf16_rne(src)[live]) and torch.isnan(dst.cpu()[~live].float()).all()
        else:
            ok = ~torch.isnan(want.view(torch.bfloat16).float())
            assert torch.equal(got[ok], want[ok])
            assert torch.isnan(dst.cpu().float()[~ok]).all()
            assert (got[mask] == 0).all(), "masked rows are not exact zeros"


@pytest.mark.parametrize("n", [1, 7, 8, 4097, 8 * 1024 + 5])
def test_widening_is_bit_exact(n):
    g = torch.Generator().manual_seed(n)
    bits = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)     # every bf16 pattern, NaNs and infinities included
    src = bits.to(DEV)
    dst = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().vllm_bf16_to_f32(P(src), P(dst), n, stream()), "vllm_bf16_to_f32")
    got = dst.cpu().view(torch.int32)
    assert torch.equal(got[:n], bits.to(torch.int32) << 16)
    assert (got[n:] == 0).all()
    assert _lib.lib().vllm_bf16_to_f32(ctypes.c_void_p(src.data_ptr() + 2), P(dst), max(n - 1, 0), stream()) == (-1 if n > 1 else 0)


# ---- the layer ---------------------------------------------------------------------------------------------------------------------------
class Linears(nn.Module):
    """the four nn.Linear of a deformable-attention module, and nothing else: what the autograd node is given"""

    def __init__(self, case):
        super().__init__()
        C, MLP = case["C"], case["M"] * case["L"] * case["P"]
        self.value_proj, self.sampling_offsets = nn.Linear(C, C), nn.Linear(C, 2 * MLP)
        self.attention_weights, self.output_proj = nn.Linear(C, MLP), nn.Linear(C, C)


def load(mod, case):
    mod.load_state_dict({k: v.float() for k, v in case["params"].items()})
    return mod.to(DEV).to(torch.bfloat16).eval()


@functools.lru_cache(maxsize=None)
def dev_case(name):
    c = T.make_case(name)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}         # ("params" stays the CPU dict ``load`` reads)
    d["linears"] = load(Linears(c), c)
    return d


def function_call(c, lin=None):
    lin = lin or c["linears"]
    return lambda q, x: A.msda_layer_train(q, c["reference_points"], x, c["spatial_shapes"], c["level_start_index"], c["padding_mask"],
                                           lin.value_proj, lin.sampling_offsets, lin.attention_weights, lin.output_proj, c["M"], c["L"], c["P"],
                                           c["four_d"])


def run(call, mod, c, need_q=True, need_x=True, gout=None, q=None, x=None):
    """one forward + backward -> (out, {query, input_flatten, PARAM_NAMES: grad or None})"""
    for p in mod.parameters():
        p.grad = None
    q = (c["query"] if q is None else q).detach().requires_grad_(need_q)
    x = (c["input_flatten"] if x is None else x).detach().requires_grad_(need_x)
    out = call(q, x)
    out.backward(c["grad_out"] if gout is None else gout)
    grads = {n: p.grad for n, p in mod.named_parameters()}
    grads.update(query=q.grad, input_flatten=x.grad)
    for p in mod.parameters():
        p.grad = None
    return out.detach(), grads


@functools.lru_cache(maxsize=None)
def native(name):
    c = dev_case(name)
    return run(function_call(c), c["linears"], c)


def same_bits(got, want, names, tag):
    for n in names:
        assert (got[n] is None) == (want[n] is None), (tag, n)
        if want[n] is not None:
            assert torch.equal(got[n], want[n]), f"{tag}: {n} differs by up to {(got[n].float() - want[n].float()).abs().max().item():.3g}"


# ---- 3: the forward has the inference layer's bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_forward_train_has_the_inference_layers_bits(name):
    c = dev_case(name)
    lin = c["linears"]
    out, _ = native(name)
    with torch.no_grad():
        want = A.msda_layer_forward(c["query"], c["reference_points"], c["input_flatten"], c["spatial_shapes"], c["level_start_index"],
                                    c["padding_mask"], lin.value_proj, lin.sampling_offsets, lin.attention_weights, lin.output_proj, c["M"],
                                    c["L"], c["P"], c["four_d"])
    assert out.dtype == torch.bfloat16 and torch.equal(out, want)


# ---- 4: every gradient against the truth, within 1.25 x the bf16 comparator's distance -----------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_layer_gradients(name):
    c = dev_case(name)
    out, g = native(name)
    y64, g64 = T.truth(name)
    y16, g16 = T.comparator(name)
    assert out.dtype == torch.bfloat16 and out.shape == y64.shape
    rows = [("out", out, y16, y64)] + [(n, g[n], g16[n], g64[n]) for n in ("query", "input_flatten") + T.PARAM_NAMES]
    worst = []
    for n, got, t16, t64 in rows:
        assert got is not None and got.dtype == torch.bfloat16 and got.shape == t64.shape, n
        assert torch.isfinite(got.float()).all(), n
        rn, rt = T.rel_rms(got.cpu(), t64), T.rel_rms(t16, t64)
        print(f"{name} {n}: native {rn:.4g} comparator {rt:.4g} ratio {rn / rt:.3f}")
        if rn > T.MARGIN * rt:
            worst.append(f"{n}: {rn:.4g} > {T.MARGIN} x {rt:.4g}")
    assert not worst, worst
    if c["padding_mask"] is not None:
        assert (g["input_flatten"][c["padding_mask"]].view(torch.int16) == 0).all(), "grad_input_flatten is not exactly zero under padded keys"


# ---- 5: the module flavours ----------------------------------------------------------------------------------------------------------------
def flavours(c):
    """name -> (module, call(q, x) -> out [B, Lq, C], what to add to grad_query's comparison)"""
    M, L, Pn, C = c["M"], c["L"], c["P"], c["C"]
    cfg = types.SimpleNamespace(d_model=C, num_feature_levels=L, disable_custom_kernels=False)
    ref, ss, lsi, mask = c["reference_points"], c["spatial_shapes"], c["level_start_index"], c["padding_mask"]
    four = bool(c["four_d"])
    uni = load(A.MSDeformAttn(C, L, M, Pn, use_4D_normalizer=four), c)
    aware = load(A.MSDeformAttnKeyAware(C, L, M, Pn, use_4D_normalizer=four), c)
    key = torch.zeros(c["query"].shape[0], 1, C, device=DEV, dtype=torch.bfloat16)
    out = {"unipose": (uni, lambda q, x: uni(q, ref, x, ss, lsi, mask)),
           "key_aware": (aware, lambda q, x: aware(q, key, ref, x, ss, lsi, mask))}
    if not four:
        mm = load(A.MultiScaleDeformableAttention(C, M, L, Pn, dropout=0.1, batch_first=False), c)
        opt = load(A.MultiScaleDeformableAttentionOptimized(C, M, L, Pn, dropout=0.1, batch_first=True), c)
        gd = load(A.GroundingDinoMultiscaleDeformableAttention(cfg, M, Pn), c)
        zero = torch.zeros_like(c["query"])
        kw = dict(key_padding_mask=mask, reference_points=ref, spatial_shapes=ss, level_start_index=lsi)
        out["mmcv_seq_first"] = (mm, lambda q, x: mm(q.transpose(0, 1), value=x.transpose(0, 1), identity=zero.transpose(0, 1), **kw).transpose(0, 1))
        out["mmcv_optimized"] = (opt, lambda q, x: opt(q, value=x, identity=zero, **kw))
        out["gdino"] = (gd, lambda q, x: gd(q, attention_mask=None if mask is None else ~mask, encoder_hidden_states=x, reference_points=ref,
                                            spatial_shapes=ss, level_start_index=lsi)[0])
    return out


@pytest.mark.parametrize("name", ["a_L3_generic_pad320", "b_4d_normalizer_pad128"])
def test_module_flavours(name, monkeypatch):
    c = dev_case(name)
    base_out, base = native(name)
    calls = []
    real = A.MSDeformAttnLayerFunction.apply
    monkeypatch.setattr(A.MSDeformAttnLayerFunction, "apply", lambda *a: (calls.append(1), real(*a))[1])
    for tag, (mod, call) in flavours(c).items():
        assert mod.native_training is False
        del calls[:]
        out, g = run(call, mod, c)                       # the flag off: the composed path, as before
        assert not calls, f"{tag}: the native node ran with native_training off"
        assert all(v is not None for v in g.values()), tag
        mod.native_training = True
        out, g = run(call, mod, c)
        assert len(calls) == 1, (tag, calls)
        assert torch.equal(out, base_out), tag
        same_bits(g, base, DETERMINISTIC, tag)
        for n in FROM_GRAD_VALUE:
            assert T.rel_rms(g[n], base[n]) < 1e-2, (tag, n)
        with torch.no_grad():                            # without grad the flag changes nothing: the fused inference call
            del calls[:]
            assert torch.equal(call(c["query"], c["input_flatten"]), base_out) and not calls
    # mmcv: the identity and the dropout stay in torch, around the node
    mod, _ = flavours(c).get("mmcv_seq_first", (None, None))
    if mod is not None:
        mod.native_training = True
        q = c["query"].transpose(0, 1).detach().requires_grad_(True)
        ident = torch.randn_like(q).requires_grad_(True)
        y = mod(q, value=c["input_flatten"].transpose(0, 1), identity=ident, key_padding_mask=c["padding_mask"],
                reference_points=c["reference_points"], spatial_shapes=c["spatial_shapes"], level_start_index=c["level_start_index"])
        assert torch.equal(y, base_out.transpose(0, 1) + ident)
        y.backward(c["grad_out"].transpose(0, 1))
        assert torch.equal(ident.grad, c["grad_out"].transpose(0, 1)) and torch.equal(q.grad, base["query"].transpose(0, 1))
        # GDINO with output_attentions keeps the composed path (the weights stay inside the native call)
        gd, _ = flavours(c)["gdino"]
        gd.native_training = True
        del calls[:]
        y, aw = gd(c["query"].detach().requires_grad_(True), encoder_hidden_states=c["input_flatten"], reference_points=c["reference_points"],
                   spatial_shapes=c["spatial_shapes"], level_start_index=c["level_start_index"], output_attentions=True)
        assert aw is not None and not calls and y.requires_grad
    # reference points that require grad keep the composed path
    uni, _ = flavours(c)["unipose"]
    uni.native_training = True
    del calls[:]
    ref = c["reference_points"].detach().clone().requires_grad_(True)
    y = uni(c["query"], ref, c["input_flatten"], c["spatial_shapes"], c["level_start_index"], c["padding_mask"])
    y.backward(c["grad_out"])
    assert not calls and ref.grad is not None


# ---- 6: frozen subsets, determinism, accumulation ----------------------------------------------------------------------------------------
SUBSETS = {
    "output_proj_only": (("output_proj.weight", "output_proj.bias"), False, False),          # stops behind the first weight-gradient GEMM
    "offset_bias_and_query": (("sampling_offsets.bias",), True, False),                      # a bias rides on its weight's launch
    "value_proj_and_input": (("value_proj.weight", "value_proj.bias"), False, True),
    "inputs_only": ((), True, True),                                                          # a frozen module in front of trainable layers
    "attention_weights_only": (("attention_weights.weight", "attention_weights.bias"), False, False),
}


@pytest.mark.parametrize("subset", sorted(SUBSETS))
@pytest.mark.parametrize("name", ["a_L3_generic_pad320", "d_decoder_bf16_value"])
def test_frozen_subsets(name, subset):
    c = dev_case(name)
    lin = c["linears"]
    trainable, need_q, need_x = SUBSETS[subset]
    base_out, base = native(name)
    try:
        for n, p in lin.named_parameters():
            p.requires_grad_(n in trainable)
        out, g = run(function_call(c), lin, c, need_q, need_x)
    finally:
        for p in lin.parameters():
            p.requires_grad_(True)
    assert torch.equal(out, base_out)
    wanted = set(trainable) | ({"query"} if need_q else set()) | ({"input_flatten"} if need_x else set())
    y64, g64 = T.truth(name)
    y16, g16 = T.comparator(name)
    for n in T.PARAM_NAMES + ("query", "input_flatten"):
        if n not in wanted:
            assert g[n] is None, f"{n} got a gradient it was not asked for"
        elif n in DETERMINISTIC:
            assert torch.equal(g[n], base[n]), n
        else:
            rn, rt = T.rel_rms(g[n].cpu(), g64[n]), T.rel_rms(g16[n], g64[n])
            print(f"{name} {subset} {n}: native {rn:.4g} comparator {rt:.4g}")
            assert rn <= T.MARGIN * rt, f"{n}: {rn:.4g} > {T.MARGIN} x {rt:.4g}"


@pytest.mark.parametrize("name", ["a_L3_generic_pad320", "c_encoder"])
def test_deterministic_and_accumulating(name):
    c = dev_case(name)
    lin = c["linears"]
    base_out, base = native(name)
    out, g = run(function_call(c), lin, c)
    assert torch.equal(out, base_out)
    same_bits(g, base, DETERMINISTIC, "second run")
    q = c["query"].detach().requires_grad_(True)
    call = function_call(c)
    call(q, c["input_flatten"]).backward(c["grad_out"])
    call(q, c["input_flatten"]).backward(c["grad_out"])
    for n, p in lin.named_parameters():
        if n in DETERMINISTIC:
            assert torch.equal(p.grad, base[n] + base[n]), n
        else:
            assert T.rel_rms(p.grad, base[n].float() * 2) < 1e-2, n
        p.grad = None
    assert torch.equal(q.grad, base["query"] + base["query"])


def test_misaligned_query_view_and_side_stream():
    name = "a_L3_generic_pad320"
    c = dev_case(name)
    lin = c["linears"]
    base_out, base = native(name)
    B, Lq, C = c["query"].shape
    store = torch.zeros(B * Lq * C + 1, device=DEV, dtype=torch.bfloat16)
    q_off = store[1:].view(B, Lq, C)
    q_off.copy_(c["query"])
    assert q_off.data_ptr() % 16 != 0
    out, g = run(function_call(c), lin, c, q=q_off)
    assert torch.equal(out, base_out)
    same_bits(g, base, DETERMINISTIC, "offset view")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out, g = run(function_call(c), lin, c)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(out, base_out)
    same_bits(g, base, DETERMINISTIC, "side stream")


# ---- 7: failure handling -------------------------------------------------------------------------------------------------------------------
def test_in_place_change_of_a_saved_input_raises():
    c = dev_case("b_4d_normalizer_pad128")
    lin = load(Linears(T.make_case("b_4d_normalizer_pad128")), T.make_case("b_4d_normalizer_pad128"))
    q = c["query"].clone().requires_grad_(True)
    x = c["input_flatten"].clone()
    y = function_call(c, lin)(q, x)
    x.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(c["grad_out"])
    y = function_call(c, lin)(q, c["input_flatten"])
    with torch.no_grad():
        lin.attention_weights.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(c["grad_out"])


def c_call_setup(name):
    c = dev_case(name)
    lin = c["linears"]
    params = [p for n in T.LINEARS for p in (getattr(lin, n).weight, getattr(lin, n).bias)]
    keep = []
    d = A._train_desc((c["M"], c["L"], c["P"], c["four_d"]), c["ref_dim"], c["C"], params, keep)
    mask = None if c["padding_mask"] is None else c["padding_mask"].to(torch.uint8)
    return c, params, d, mask, keep


def test_invalid_calls_write_nothing():
    L = _lib.lib()
    c, params, d, mask, keep = c_call_setup("a_L3_generic_pad320")
    Bn, Lq, S, C = T.B, c["Lq"], c["S"], c["C"]
    dims = (Bn, Lq, S)
    ns, nf, nb = (getattr(L, q)(ctypes.byref(d), *dims) for q in ("vllm_msda_layer_saved_bytes", "vllm_msda_layer_forward_train_workspace_bytes",
                                                                   "vllm_msda_layer_backward_workspace_bytes"))
    seven = lambda *s: torch.full(s, 7.0, device=DEV).to(torch.bfloat16)
    out, gq, gx = seven(Bn, Lq, C), seven(Bn, Lq, C), seven(Bn, S, C)
    saved = torch.full((ns,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((max(nf, nb),), 7, dtype=torch.uint8, device=DEV)
    grads = [seven(*p.shape) for p in params]
    names = [n for n, _ in _lib.VllmMsdaLayerGrads._fields_]
    gs = _lib.VllmMsdaLayerGrads(**{n: t.data_ptr() for n, t in zip(names, grads)})
    v16 = ctypes.c_int(7)
    q, x, ref, gout = c["query"], c["input_flatten"], c["reference_points"], c["grad_out"]
    ss, lsi = c["spatial_shapes"], c["level_start_index"]

    def fwd(dd=d, nws=nf, nsv=ns, qq=q, wsp=ws):
        return L.vllm_msda_layer_forward_train(ctypes.byref(dd), P(qq), P(ref), P(x), P(mask), P(ss), P(lsi), *dims, P(out), P(saved), nsv,
                                               ctypes.byref(v16), P(wsp), nws, stream())

    def bwd(dd=d, nws=nb, nsv=ns, gg=gs, go=gout, wsp=ws, v=0, sizes=dims):
        return L.vllm_msda_layer_backward(ctypes.byref(dd), P(q), P(ref), P(x), P(mask), P(ss), P(lsi), *sizes, P(saved), nsv, v, P(go), P(gq), P(gx),
                                          ctypes.byref(gg), P(wsp), nws, stream())

    bad = A._train_desc((7, c["L"], c["P"], c["four_d"]), c["ref_dim"], C, params, keep)          # 256 % 7
    assert fwd(dd=bad) == -1 and bwd(dd=bad) == -1 and L.vllm_msda_layer_backward_workspace_bytes(ctypes.byref(bad), *dims) < 0
    assert fwd(nws=nf - 1) == -1 and b"workspace" in L.vllm_last_error()
    assert bwd(nws=nb - 1) == -1 and b"workspace" in L.vllm_last_error()
    off8 = ws[8:]
    assert fwd(wsp=off8) == -1 and b"workspace" in L.vllm_last_error()
    assert bwd(wsp=off8) == -1 and b"workspace" in L.vllm_last_error()
    assert fwd(wsp=None) == -1 and bwd(wsp=None) == -1
    assert fwd(nsv=ns - 1) == -1 and bwd(nsv=ns - 1) == -1 and b"saved" in L.vllm_last_error()
    q_off = torch.zeros(q.numel() + 1, device=DEV, dtype=torch.bfloat16)[1:].view(q.shape)
    assert fwd(qq=q_off) == -1 and b"aligned" in L.vllm_last_error()
    go_off = torch.zeros(q.numel() + 1, device=DEV, dtype=torch.bfloat16)[1:].view(q.shape)
    assert bwd(go=go_off) == -1 and b"aligned" in L.vllm_last_error()
    assert bwd(go=None) == -1
    lone = _lib.VllmMsdaLayerGrads(**{n: (t.data_ptr() if n != "output_proj_w" else None) for n, t in zip(names, grads)})
    assert bwd(gg=lone) == -1 and b"bias gradient" in L.vllm_last_error()
    assert bwd(v=2) == -1
    torch.cuda.synchronize()
    for t in [out, gq, gx] + grads:
        assert (t == 7.0).all()
    assert (saved == 7).all() and (ws == 7).all() and v16.value == 7
    assert fwd() == 0 and v16.value == 0 and bwd() == 0                         # and the valid calls go through
    torch.cuda.synchronize()
    base_out, base = native("a_L3_generic_pad320")
    assert torch.equal(out, base_out) and torch.equal(gq, base["query"])
    # no queries: nothing to do forward; every parameter gradient and grad_input_flatten is an empty sum
    assert L.vllm_msda_layer_forward_train(ctypes.byref(d), P(q), P(ref), P(x), P(mask), P(ss), P(lsi), Bn, 0, S, P(out), None, 0, ctypes.byref(v16), None,
                                           0, stream()) == 0
    assert bwd(sizes=(Bn, 0, S), wsp=None, nws=0, nsv=0) == 0
    torch.cuda.synchronize()
    for t in grads + [gx]:
        assert (t.view(torch.int16) == 0).all()
    assert torch.equal(gq, base["query"])


# ---- 8: the caller-workspace contract of both entries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_L3_generic_pad320", "c_encoder", "d_decoder_bf16_value"])
def test_msda_layer_train_workspace(name, monkeypatch):
    """Every request of the node (the forward's, the backward's) is a fresh buffer of exactly the bytes the query answers, at the least
    alignment, NaN-filled, between guard bytes: the deterministic tensors keep the clean run's bits, the others the 1.25 rule."""
    c = dev_case(name)
    lin = c["linears"]
    base_out, base = native(name)
    y64, g64 = T.truth(name)
    y16, g16 = T.comparator(name)

    def one(W):
        out, g = run(function_call(c), lin, c)
        return dict(out=out, **g)

    outs, spaces = WC.three_runs(one, widest_row_bytes=max(c["C"], T.npad(c["M"], c["L"], c["P"])) * 4, patch=monkeypatch, exempt=FROM_GRAD_VALUE)
    assert len(spaces[0].sizes) == 2 and min(spaces[0].sizes) > 0, spaces[0].sizes
    same_bits(outs[0], dict(out=base_out, **base), ("out",) + DETERMINISTIC, "baseline")
    for o in outs:
        for n in FROM_GRAD_VALUE:
            assert torch.isfinite(o[n].float()).all(), n
            rn, rt = T.rel_rms(o[n].cpu(), g64[n]), T.rel_rms(g16[n], g64[n])
            assert rn <= T.MARGIN * rt, f"{n}: {rn:.4g} > {T.MARGIN} x {rt:.4g}"


@pytest.mark.parametrize("name", ["a_L3_generic_pad320", "d_decoder_bf16_value"])
def test_c_entries_take_exactly_the_queries_bytes(name):
    """straight through the C ABI: saved memory and both workspaces of exactly the queries' bytes, hostile and guarded"""
    L = _lib.lib()
    c, params, d, mask, keep = c_call_setup(name)
    Bn, Lq, S, C = T.B, c["Lq"], c["S"], c["C"]
    dims = (Bn, Lq, S)
    ns, nf, nb = (getattr(L, q)(ctypes.byref(d), *dims) for q in ("vllm_msda_layer_saved_bytes", "vllm_msda_layer_forward_train_workspace_bytes",
                                                                   "vllm_msda_layer_backward_workspace_bytes"))
    names = [n for n, _ in _lib.VllmMsdaLayerGrads._fields_]
    q, x, ref, gout = c["query"], c["input_flatten"], c["reference_points"], c["grad_out"]
    ss, lsi = c["spatial_shapes"], c["level_start_index"]

    def one(W):
        saved, _ = W.take(ns)
        ws, n = W.take(nf)
        out, gq, gx = WC.nan_bf16(Bn, Lq, C), WC.nan_bf16(Bn, Lq, C), WC.nan_bf16(Bn, S, C)
        grads = [WC.nan_bf16(*p.shape) for p in params]
        gs = _lib.VllmMsdaLayerGrads(**{k: t.data_ptr() for k, t in zip(names, grads)})
        v16 = ctypes.c_int(-1)
        _lib.check(L.vllm_msda_layer_forward_train(ctypes.byref(d), P(q), P(ref), P(x), P(mask), P(ss), P(lsi), *dims, P(out), P(saved), ns,
                                                   ctypes.byref(v16), P(ws), n, stream()), "vllm_msda_layer_forward_train")
        assert v16.value == (1 if name == "d_decoder_bf16_value" else 0)
        ws, n = W.take(nb)
        _lib.check(L.vllm_msda_layer_backward(ctypes.byref(d), P(q), P(ref), P(x), P(mask), P(ss), P(lsi), *dims, P(saved), ns, v16.value, P(gout),
                                              P(gq), P(gx), ctypes.byref(gs), P(ws), n, stream()), "vllm_msda_layer_backward")
        return dict(out=out, query=gq, input_flatten=gx, **dict(zip(T.PARAM_NAMES, grads)))

    outs, _ = WC.three_runs(one, widest_row_bytes=max(C, T.npad(c["M"], c["L"], c["P"])) * 4, exempt=FROM_GRAD_VALUE)
    base_out, base = native(name)
    same_bits(outs[0], dict(out=base_out, **base), ("out",) + DETERMINISTIC, "C call")
    for o in outs:
        for n in FROM_GRAD_VALUE:
            assert torch.isfinite(o[n].float()).all() and T.rel_rms(o[n], base[n]) < 1e-2, n
