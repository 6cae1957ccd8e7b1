"""GPU: every MSDA backward kernel, and the layer's training path on top of them, ON the pixel lattice a freshly initialised module
samples (lattice_inputs.py): integer pixel positions and their fp32 neighbours, the acceptance edges from both sides.

grad_sampling_loc is discontinuous across a cell border, so a kernel whose ``loc * H - 0.5`` rounds differently (one fused multiply-add)
returns the other one-sided derivative at such a point.  The reference is the fixed-cell one: the cell from the index-exact contract
(``oracle.msda.sample_index`` on the locations in their own dtype), the value from torch fp64 autograd of the bilinear sum in that cell.
No point is left out of any comparison; the bounds are those the existing backward tests use away from the borders."""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lattice_inputs as LI
import msda_layer_train_inputs as T
from bounds import P as PTR, stream
from test_msda_gpu import _bf16_vs_reference_arithmetic
from visionllm_amd import _lib
from visionllm_amd import ms_deform_attn as A
from visionllm_amd.ms_deform_attn import _sampling_locations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = ["init", "nudged"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _backward(g):
    gv, gl, gw = A.ms_deform_attn_backward(_t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"]), _t(g["go"]), 64)
    return gv.cpu().numpy(), gl.cpu().numpy(), gw.cpu().numpy()


def _check_f32(key, what):
    """the case ``key`` (lattice_inputs.make_case's arguments) through ms_deform_attn_backward, twice -> the first run's gradients"""
    g, ref = LI.make_case(*key), LI.reference(*key)
    gv, gl, gw = _backward(g)
    _, gl2, gw2 = _backward(g)
    assert np.isfinite(gv).all() and np.isfinite(gl).all() and np.isfinite(gw).all(), what
    assert np.array_equal(gl, gl2) and np.array_equal(gw, gw2), f"{what}: two runs give different per-point gradients"
    LI.check_point_gradients(gl, gw, ref, what)
    LI.check_grad_value_f32(gv, ref, what)
    return gv, gl, gw


# ---- the windowed matrix-core backward and the plain atomic backward (encoder shape) ---------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shapes,B,M", [(LI.ENCODER_MAPS, 2, 8), (LI.ODD_MAPS, 1, 3)])
def test_encoder_shape_backward_on_the_lattice(shapes, B, M, variant):
    """Lq = S >= 4096, D 32, P 4: msda_tiled = 1 (msda_bwd_mfma.hip) and 0 (the plain atomic kernel), each against the fixed-cell
    reference at every point, and against each other as test_backward_f32_encoder_shape_tiled_vs_plain_vs_oracle demands."""
    key = (shapes, M, 32, 4, B, None, variant)
    g = LI.make_case(*key)
    fwd = LI.O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    res = {}
    old = _lib.set_option("msda_tiled", 1)
    try:
        for mode in (1, 0):
            _lib.set_option("msda_tiled", mode)
            res[mode] = _check_f32(key, f"msda_tiled = {mode}, {variant}")
            # the forward of the same option (generation 9 / 4 with their own copy of the location arithmetic, the gather kernel):
            # continuous in the location, but a wrong cell at a map border drops or adds a corner
            out = A.ms_deform_attn_forward(_t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"]), 64)
            np.testing.assert_allclose(out.cpu().numpy(), fwd, rtol=4e-6, atol=4e-6, err_msg=f"forward, msda_tiled = {mode}")
    finally:
        _lib.set_option("msda_tiled", old)
    for i in (1, 2):
        scale = np.abs(res[0][i]).max() + 1e-12
        np.testing.assert_allclose(res[1][i], res[0][i], rtol=1e-4, atol=2e-6 * scale)
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-4, atol=1e-4)


# ---- the vectorised and the generic backward (Lq != S) ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D,M,P", [(32, 8, 4), (64, 2, 8), (16, 4, 2), (4, 3, 1), (128, 1, 4)])
def test_vectorised_backward_on_the_lattice(D, M, P, variant):
    """D / 4 a power of two, 77 queries that are a seeded subset of the cells"""
    _check_f32((LI.SMALL_MAPS, M, D, P, 2, 77, variant), f"vectorised D{D} M{M} P{P}, {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", [30, 71])
def test_generic_backward_f32_on_the_lattice(D, variant):
    _check_f32((LI.SMALL_MAPS, 2, D, 4, 2, 77, variant), f"generic D{D}, {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("D", [4, 30])
def test_backward_f64_on_the_lattice(D, variant):
    """the fp64 entry on the fp64 lattice (the module's statements in fp64, nudged by fp64 ulps): the cells of the fp64 locations"""
    key = (LI.SMALL_MAPS, 2, D, 4, 2, 77, variant, "float64")
    g, ref = LI.make_case(*key), LI.reference(*key)
    assert g["loc"].dtype == np.float64
    gv, gl, gw = _backward(g)
    _, gl2, gw2 = _backward(g)
    assert np.array_equal(gl, gl2) and np.array_equal(gw, gw2)
    tol = dict(rtol=1e-10, atol=1e-12)
    LI.check_point_gradients(gl, gw, ref, f"fp64 D{D}, {variant}", gl_tol=tol, gw_tol=tol)
    np.testing.assert_allclose(gv, ref["gv"], **tol)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("function", ["MSDeformAttnFunction", "MultiScaleDeformableAttnFunction"])
def test_autograd_functions_on_the_lattice(function, variant):
    """the UniPose / HF autograd node and the mmcv flavour: the gradients autograd hands back are the checked ones"""
    key = (LI.SMALL_MAPS, 8, 32, 4, 2, 77, variant)
    g, ref = LI.make_case(*key), LI.reference(*key)
    v, loc, w = (_t(g[k]).requires_grad_(True) for k in ("value", "loc", "attw"))
    out = getattr(A, function).apply(v, _t(g["shapes"]), _t(g["lsi"]), loc, w, 64)
    out.backward(_t(g["go"]))
    LI.check_point_gradients(loc.grad.cpu().numpy(), w.grad.cpu().numpy(), ref, function)
    LI.check_grad_value_f32(v.grad.cpu().numpy(), ref, function)
    # and the forward they ran (continuous in the location; a wrong cell at a map border drops or adds a corner)
    np.testing.assert_allclose(out.detach().cpu().numpy(), LI.O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"]), rtol=2e-5, atol=2e-5)


# ---- the layer's training path at the init state ------------------------------------------------------------------------------------------------
LAYER_MAPS = {"encoder": (LI.ENCODER_MAPS, 1), "small": (((12, 16), (6, 8), (3, 4)), 2)}      # name -> maps, images
LAYER_M, LAYER_C, LAYER_P = 8, 256, 4


def _fresh_module(flavour, L):
    """a module as its constructor leaves it (zero query weights, the direction grid as the offset bias), then bf16 on the GPU; the three
    constructors run the same statements, so one seed gives the three the same parameters"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(77)
        if flavour == "unipose":
            mod = A.MSDeformAttn(LAYER_C, L, LAYER_M, LAYER_P)
        elif flavour == "mmcv":
            mod = A.MultiScaleDeformableAttention(LAYER_C, LAYER_M, L, LAYER_P, dropout=0.1, batch_first=False)
        else:
            cfg = types.SimpleNamespace(d_model=LAYER_C, num_feature_levels=L, disable_custom_kernels=False)
            mod = A.GroundingDinoMultiscaleDeformableAttention(cfg, LAYER_M, LAYER_P)
    return mod.to(DEV).to(torch.bfloat16).eval()


def _composed_forward(flavour, mod, c):
    """the module's composed path (grad enabled, trainable parameters, native_training off): torch bf16 linears around the fp32 operator"""
    q, x, ref, ss, lsi, mask = (c[k].to(DEV) for k in ("query", "input_flatten", "reference_points", "spatial_shapes", "level_start_index",
                                                         "padding_mask"))
    assert mod.native_training is False
    with torch.enable_grad():
        if flavour == "unipose":
            return mod(q, ref, x, ss, lsi, mask).detach()
        if flavour == "mmcv":
            return mod(q.transpose(0, 1), value=x.transpose(0, 1), identity=torch.zeros_like(q).transpose(0, 1), key_padding_mask=mask,
                       reference_points=ref, spatial_shapes=ss, level_start_index=lsi).transpose(0, 1).detach()
        return mod(q, attention_mask=~mask, encoder_hidden_states=x, reference_points=ref, spatial_shapes=ss, level_start_index=lsi)[0].detach()


@functools.lru_cache(maxsize=None)
def _layer_inputs(name):
    """CPU tensors: bf16 query / input_flatten / grad_out, the pixel centres as reference points (replicated over the levels), the last
    image's tail padded.  Cached: leave it unchanged."""
    maps, Bn = LAYER_MAPS[name]
    L = len(maps)
    S = sum(h * w for h, w in maps)
    g = torch.Generator().manual_seed(8000 + S)
    bf = lambda t: t.to(torch.bfloat16)
    query, src = bf(torch.randn(Bn, S, LAYER_C, generator=g)), bf(torch.randn(Bn, S, LAYER_C, generator=g))
    grad_out = bf(torch.randn(Bn, S, LAYER_C, generator=g) / math.sqrt(LAYER_C))
    ref = LI.pixel_centres(maps)[None, :, None, :].expand(Bn, S, L, 2).contiguous()
    mask = torch.zeros(Bn, S, dtype=torch.bool)
    mask[-1, -(S // 7):] = True
    return dict(query=query, input_flatten=src, grad_out=grad_out, reference_points=ref, spatial_shapes=torch.tensor(maps, dtype=torch.int64),
                level_start_index=torch.from_numpy(LI.O.level_start_index(maps)), padding_mask=mask, maps=maps, B=Bn, S=S, L=L)


def _layer_statements(p, c, dtype, cells, loc_value=None, op_dtype=None):
    """autograd of the statements of msda_layer_train_inputs.layer in ``dtype`` with the operator replaced by fixed_cell_msda at ``cells``.
    ``loc_value``: the location's VALUE (the tensor the forward that ran saved); its derivative path still runs through the offsets.
    -> out, {query, input_flatten, PARAM_NAMES: grad}, value, attention weights"""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in p.items()}
    q = c["query"].detach().to(dtype).requires_grad_(True)
    x = c["input_flatten"].detach().to(dtype).requires_grad_(True)
    N, Lq, C = q.shape
    M, Pn, L = LAYER_M, LAYER_P, c["L"]
    value = F.linear(x, p["value_proj.weight"], p["value_proj.bias"]).masked_fill(c["padding_mask"][..., None], float(0)).view(N, c["S"], M, C // M)
    off = F.linear(q, p["sampling_offsets.weight"], p["sampling_offsets.bias"]).view(N, Lq, M, L, Pn, 2)
    aw = F.softmax(F.linear(q, p["attention_weights.weight"], p["attention_weights.bias"]).view(N, Lq, M, L * Pn), -1).view(N, Lq, M, L, Pn)
    loc = _sampling_locations(c["reference_points"].to(dtype), off, c["spatial_shapes"], Pn, False)
    if loc_value is not None:
        loc = loc_value.to(dtype) + (loc - loc.detach())
    od = op_dtype or dtype
    h, w, ok = cells
    core = LI.fixed_cell_msda(value.to(od), c["maps"], c["level_start_index"].tolist(), loc.to(od), aw.to(od), h, w, ok).to(dtype)
    out = F.linear(core, p["output_proj.weight"], p["output_proj.bias"])
    out.backward(c["grad_out"].to(dtype))
    grads = {k: v.grad for k, v in p.items()}
    grads.update(query=q.grad, input_flatten=x.grad)
    return out.detach(), grads, value.detach(), aw.detach()


_LAYER_TRUTH = {}


def _layer_truth(name, params, saved_loc):
    """(parameters, saved locations, cells, truth, comparator) of a map set, computed for the first flavour and shared by the others --
    whose parameters and saved locations are asserted to be the same bits"""
    if name not in _LAYER_TRUTH:
        c = _layer_inputs(name)
        cells = LI.cells(c["maps"], saved_loc.numpy())
        truth = _layer_statements(params, c, torch.float64, cells, loc_value=saved_loc)
        comparator = _layer_statements(params, c, torch.bfloat16, cells, op_dtype=torch.float32)
        _LAYER_TRUTH[name] = (params, saved_loc, cells, truth, comparator)
    kept = _LAYER_TRUTH[name]
    assert all(torch.equal(params[k], kept[0][k]) for k in T.PARAM_NAMES) and torch.equal(saved_loc, kept[1])
    return kept[2:]


@pytest.mark.parametrize("flavour", ["unipose", "mmcv", "gdino"])
@pytest.mark.parametrize("name", sorted(LAYER_MAPS))
def test_layer_training_path_at_the_init_state(name, flavour):
    """vllm_msda_layer_forward_train / vllm_msda_layer_backward through the C ABI on a bf16 module as its constructor leaves it, with
    pixel-centre reference points: the backward must differentiate the forward that actually ran.  The cells are the index-exact
    contract on the locations the forward SAVED; the truth is fp64 autograd of the reference's statements with the operator at those
    cells (the location's value the saved one, its derivative through the offsets); the comparator the same statements in bf16 (fp32
    around the operator) at the same cells.  Every gradient within MARGIN x the comparator's distance (test_layer_gradients' criterion),
    the output within _bf16_vs_reference_arithmetic of the module's composed path."""
    lib = _lib.lib()
    c = _layer_inputs(name)
    Bn, S, Lc, C, M, Pn = c["B"], c["S"], c["L"], LAYER_C, LAYER_M, LAYER_P
    mod = _fresh_module(flavour, Lc)
    params = [p for n in T.LINEARS for p in (getattr(mod, n).weight, getattr(mod, n).bias)]
    assert float(mod.sampling_offsets.weight.detach().abs().max()) == 0 and float(mod.attention_weights.weight.detach().abs().max()) == 0
    keep = []
    d = A._train_desc((M, Lc, Pn, False), 2, C, params, keep)
    dims = (Bn, S, S)
    ns, nf, nb = (getattr(lib, f)(ctypes.byref(d), *dims) for f in ("vllm_msda_layer_saved_bytes", "vllm_msda_layer_forward_train_workspace_bytes",
                                                                    "vllm_msda_layer_backward_workspace_bytes"))
    assert min(ns, nf, nb) > 0
    dev = {k: c[k].to(DEV) for k in ("query", "input_flatten", "grad_out", "reference_points", "spatial_shapes", "level_start_index")}
    mask = c["padding_mask"].to(DEV).to(torch.uint8)
    saved = torch.zeros(ns, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(max(nf, nb), dtype=torch.uint8, device=DEV)
    nan16 = lambda *s: torch.full(s, float("nan"), device=DEV).to(torch.bfloat16)
    out, gq, gx = nan16(Bn, S, C), nan16(Bn, S, C), nan16(Bn, S, C)
    grads = [nan16(*p.shape) for p in params]
    names = [n for n, _ in _lib.VllmMsdaLayerGrads._fields_]
    gs = _lib.VllmMsdaLayerGrads(**{n: t.data_ptr() for n, t in zip(names, grads)})
    v16 = ctypes.c_int(-1)
    common = (PTR(dev["query"]), PTR(dev["reference_points"]), PTR(dev["input_flatten"]), PTR(mask), PTR(dev["spatial_shapes"]),
              PTR(dev["level_start_index"]), *dims)
    _lib.check(lib.vllm_msda_layer_forward_train(ctypes.byref(d), *common, PTR(out), PTR(saved), ns, ctypes.byref(v16), PTR(ws), nf, stream()),
               "vllm_msda_layer_forward_train")
    assert v16.value in (0, 1)
    _lib.check(lib.vllm_msda_layer_backward(ctypes.byref(d), *common, PTR(saved), ns, v16.value, PTR(dev["grad_out"]), PTR(gq), PTR(gx),
                                            ctypes.byref(gs), PTR(ws), nb, stream()), "vllm_msda_layer_backward")
    torch.cuda.synchronize()
    # what the forward saved (include/vllm_hip.h: value, locations, weights, each piece rounded up to 256 bytes)
    up = lambda n: (n + 255) // 256 * 256
    MLP = M * Lc * Pn
    o_loc = up(Bn * S * C * 4)
    o_w = o_loc + up(Bn * S * MLP * 2 * 4)
    raw = saved.cpu()
    sv_value = (raw[:Bn * S * C * 2].view(torch.bfloat16).float() if v16.value else raw[:Bn * S * C * 4].view(torch.float32)).view(Bn, S, M, C // M)
    sv_loc = raw[o_loc:o_loc + Bn * S * MLP * 8].view(torch.float32).view(Bn, S, M, Lc, Pn, 2).clone()
    sv_w = raw[o_w:o_w + Bn * S * MLP * 4].view(torch.float32).view(Bn, S, M, Lc, Pn)
    near, flip = LI.lattice_shares(c["maps"], sv_loc.numpy())
    print(f"{name} {flavour}: saved locations: near-border share {near:.3f}, fp32/fp64 cell-flip share {flip:.3f}")
    assert near >= 0.2, "the layer's saved locations are not on the lattice"
    cpu_params = {n: p.detach().cpu() for n, p in zip(T.PARAM_NAMES, params)}
    cells, (y64, g64, value64, aw64), (y16, g16, _, _) = _layer_truth(name, cpu_params, sv_loc)
    # the saved weights and value are the statements' (zero logits: a uniform softmax; the value a bf16 GEMM's fp32 result, masked)
    assert float((sv_w.double() - aw64).abs().max()) <= 1e-6
    assert T.rel_rms(sv_value, value64) <= 2.0 ** -8 and float(sv_value[c["padding_mask"]].abs().max()) == 0
    got = dict(zip(T.PARAM_NAMES, grads), query=gq, input_flatten=gx)
    worst = []
    for n in ("query", "input_flatten") + T.PARAM_NAMES:
        assert got[n].dtype == torch.bfloat16 and got[n].shape == g64[n].shape and torch.isfinite(got[n].float()).all(), n
        rn, rt = T.rel_rms(got[n].cpu(), g64[n]), T.rel_rms(g16[n], g64[n])
        print(f"{name} {flavour} {n}: native {rn:.4g} comparator {rt:.4g}")
        if rn > T.MARGIN * rt:
            worst.append(f"{n}: {rn:.4g} > {T.MARGIN} x {rt:.4g}")
    assert not worst, worst
    assert (gx[mask.bool()].view(torch.int16) == 0).all()
    _bf16_vs_reference_arithmetic(out, _composed_forward(flavour, mod, c), y64.numpy(), f"{name} {flavour}")
