"""Every public op on operands where real callers put them: contiguous views at a storage offset, and caller streams.

The rest of the suite builds its inputs as fresh allocations (256-byte aligned) and runs on the default stream.  Callers also pass
views (x[1:], a chunk of one flat buffer, parameters loaded into one packed storage) -- the reference's ops only ask for
is_contiguous() -- and enqueue work on streams of their own.  Here:

* offset views: every operand displaced alone, then all of them, at every 16-byte misalignment the dtype allows, with the
  buffer around the view holding a sentinel (NaN); the result is checked against the same reference, at the same tolerance, as the
  op's aligned test, and ops that write into a caller's buffer leave every byte outside the view as it was.  The shapes are the ones
  that take the fast kernels when aligned, so each pointer gate is checked along with the path it falls back to.
* the C ABI: an entry point with an alignment requirement (include/vllm_hip.h) returns VLLM_EINVAL, names the requirement and
  writes nothing.
* caller streams: an op called under `torch.cuda.stream(s)` is ordered behind the work on `s` that produced its inputs and leaves
  its result on `s`; the encoder on one stream and the projector / deformable-attention layer on another (the three share scratch
  memory per stream) give exactly the results of a serial run.
"""
import ast

import numpy as np
import pytest
import torch

import lattice_inputs as LI
from conftest import golden_sd, load_golden
from msda_inputs import make_inputs
from oracle import dcnv3 as OD
from oracle import msda as O
from oracle import region as OR
from oracle import vit as V
from visionllm_amd import _lib
from visionllm_amd import dcnv3 as D3
from visionllm_amd import ms_deform_attn as A
from visionllm_amd import region_encoder as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# byte offsets (mod 16) a contiguous view of each element type can sit at, other than 0
OFFSETS = {torch.float32: (4, 8, 12), torch.bfloat16: (2, 4, 6, 8, 10, 12, 14), torch.float16: (2, 4, 6, 8, 10, 12, 14),
           torch.float64: (8,), torch.uint8: (1, 7, 8), torch.int64: (8,)}
ENCODER_SHAPES = [(72, 64), (36, 32), (18, 16), (9, 8)]      # S = 6120: Lq == S >= 4096 takes the LDS-tiled kernels


def _sentinel(dtype):
    return float("nan") if dtype.is_floating_point else 0x5A


def placed(t, off):
    """-> (view, parent): a contiguous copy of `t` at byte offset `off` of a larger buffer (256-byte aligned base) whose other
    elements hold a sentinel (NaN for floating types)."""
    es = t.element_size()
    assert off % es == 0
    k, n = off // es, t.numel()
    parent = torch.full((k + n + 64 // es,), _sentinel(t.dtype), dtype=t.dtype, device=DEV)
    view = parent[k:k + n].view(t.shape)
    view.copy_(t.to(DEV))
    assert view.is_contiguous() and view.data_ptr() % 16 == off % 16
    return view, parent


def cases(ops):
    """ops {name: tensor} -> [(label, {name: byte offset})]: each operand alone at every offset its dtype allows, then all of
    them together (the k-th offset of each)."""
    out = []
    for name, t in ops.items():
        out += [(f"{name}@{o}", {name: o}) for o in OFFSETS[t.dtype]]
    for k in range(max(len(OFFSETS[t.dtype]) for t in ops.values())):
        out.append((f"all#{k}", {n: OFFSETS[t.dtype][k % len(OFFSETS[t.dtype])] for n, t in ops.items()}))
    return out


def displaced(ops, where):
    return {n: (placed(t, where[n])[0] if n in where else t) for n, t in ops.items()}


def bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


# ---- MSDA operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["encoder_remembered", "encoder_unknown", "decoder"])
def test_msda_forward_f32_offset_views(shape):
    enc = shape.startswith("encoder")
    g = make_inputs(1 if enc else 2, 8, 32, ENCODER_SHAPES if enc else [(21, 19), (11, 10), (6, 5), (3, 3)], 4,
                    Lq=None if enc else 333, mode="encoder_like" if enc else "stress", seed=17)
    ss, lsi = _t(g["shapes"]), _t(g["lsi"])
    if shape == "encoder_remembered":
        assert A.remember_geometry(ss) == A.GEO_PYRAMID
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    tol = 4e-6 if enc else 2e-5        # the aligned tests' bounds (test_msda_gpu.py: tiled kernels / gather kernels)
    ho, wo, mo = O.sample_index(g["shapes"], g["loc"])
    ops = {"value": _t(g["value"]), "loc": _t(g["loc"]), "attw": _t(g["attw"])}
    for label, where in cases(ops):
        a = displaced(ops, where)
        out = A.ms_deform_attn_forward(a["value"], ss, lsi, a["loc"], a["attw"], 64)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=tol, atol=tol, err_msg=label)
        h, w, mk = A.sample_index(ss, a["loc"])
        assert np.array_equal(mk.cpu().numpy(), mo) and np.array_equal(h.cpu().numpy(), ho) and np.array_equal(w.cpu().numpy(), wo), label


def test_msda_forward_f64_and_bf16_offset_views():
    g = load_golden("msda_kat_seed3.npz")
    ss, lsi = _t(g["shapes"]), _t(g["lsi"])
    ops = {"value": _t(g["value"], torch.float64), "loc": _t(g["loc"], torch.float64), "attw": _t(g["attw"], torch.float64)}
    for label, where in cases(ops):
        a = displaced(ops, where)
        out = A.ms_deform_attn_forward(a["value"], ss, lsi, a["loc"], a["attw"], 64)
        np.testing.assert_allclose(out.cpu().numpy(), g["out_f64"], rtol=1e-12, atol=1e-15, err_msg=label)
    # bf16 value (the entry point requires 16-byte aligned value / 8-byte aligned loc: the wrapper copies a view that misses it)
    g = make_inputs(2, 8, 32, [(21, 19), (11, 10), (6, 5), (3, 3)], 4, Lq=200, mode="stress", seed=5)
    vb = torch.from_numpy(g["value"]).to(torch.bfloat16)
    ref = O.forward(vb.float().numpy(), g["shapes"], g["lsi"], g["loc"], g["attw"])
    ss, lsi = _t(g["shapes"]), _t(g["lsi"])
    ops = {"value": vb.to(DEV), "loc": _t(g["loc"]), "attw": _t(g["attw"])}
    for label, where in cases(ops):
        a = displaced(ops, where)
        out = A.ms_deform_attn_forward(a["value"], ss, lsi, a["loc"], a["attw"], 64)
        np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=8e-3, atol=8e-3, err_msg=label)


def _border_free(loc, shapes):
    """Points away from exact pixel borders (where d/dloc is discontinuous: fp32 and fp64 may pick different sides, so the fp64 oracle
    is the reference for these points only; the others go against lattice_inputs' fixed-cell reference)."""
    sel = np.isfinite(loc).all(-1)
    for l, (H, W) in enumerate(shapes):
        fy = np.nan_to_num(loc[:, :, :, l, :, 1].astype(np.float64)) * H - 0.5
        fx = np.nan_to_num(loc[:, :, :, l, :, 0].astype(np.float64)) * W - 0.5
        sel[:, :, :, l] &= ~((np.abs(fy - np.round(fy)) < 1e-4) | (np.abs(fx - np.round(fx)) < 1e-4))
    return sel


@pytest.mark.parametrize("shape", ["encoder", "decoder"])
def test_msda_backward_f32_offset_views(shape):
    """Encoder shape: the matrix-core backward when aligned (it writes the per-point gradients itself, so the allocating flavour
    leaves them uninitialised -- the query must see the displaced pointers); decoder shape: the vectorised kernel."""
    enc = shape == "encoder"
    shapes = ENCODER_SHAPES if enc else [(13, 11), (7, 6), (4, 3)]
    g = make_inputs(1 if enc else 2, 8, 32, shapes, 4, Lq=None if enc else 77, mode="encoder_like" if enc else "stress", seed=23)
    Lq = g["loc"].shape[1]
    go = np.random.default_rng(3).standard_normal((g["value"].shape[0], Lq, 8 * 32)).astype(np.float32)
    rv, rl, rw = O.backward(g["value"].astype(np.float64), g["shapes"], g["lsi"], g["loc"].astype(np.float64),
                            g["attw"].astype(np.float64), go.astype(np.float64))
    rv32, _, _ = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], go)
    mag, _, _ = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], np.abs(g["attw"]), np.abs(go))
    sel = _border_free(g["loc"], shapes)
    # the finite points at a border: the one-sided derivative of the cell the index-exact contract puts them in (lattice_inputs.py), at
    # the same bounds; the reference is the same for every placement
    finite = np.isfinite(g["loc"]).all(-1)
    drop = finite & ~sel
    fl, fw, _ = LI.fixed_cell_point_gradients(g["value"], shapes, g["lsi"], g["loc"], g["attw"], go, drop)
    assert enc or drop.sum() > 0          # (the stress fixture holds 0.0 / 0.5 / 1.0 on purpose)
    ss, lsi = _t(g["shapes"]), _t(g["lsi"])
    ops = {"value": _t(g["value"]), "loc": _t(g["loc"]), "attw": _t(g["attw"]), "grad_out": _t(go)}
    gv0, gl0 = torch.zeros_like(ops["value"]), torch.empty_like(ops["loc"])
    assert _lib.lib().vllm_msda_backward_f32_writes_point_grads(_lib.ptr(ops["value"]), _lib.ptr(ops["loc"]), _lib.ptr(ops["grad_out"]),
                                                               _lib.ptr(gv0), _lib.ptr(gl0), *g["value"].shape[:2], 8, 32, len(shapes), Lq,
                                                               4) == int(enc)
    for label, where in cases(ops):
        a = displaced(ops, where)
        gv, gl, gw = A.ms_deform_attn_backward(a["value"], ss, lsi, a["loc"], a["attw"], a["grad_out"], 64)
        assert torch.isfinite(gl).all() and torch.isfinite(gw).all(), label
        np.testing.assert_allclose(gw.cpu().numpy()[sel], rw[sel], rtol=1e-4, atol=1e-4, err_msg=label)
        np.testing.assert_allclose(gl.cpu().numpy()[sel], rl[sel], rtol=2e-3, atol=2e-3, err_msg=label)
        np.testing.assert_allclose(gw.cpu().numpy()[drop], fw[drop], err_msg=label, **LI.GW_TOL)
        np.testing.assert_allclose(gl.cpu().numpy()[drop], fl[drop], err_msg=label, **LI.GL_TOL)
        assert (gl.cpu().numpy()[~finite] == 0).all() and (gw.cpu().numpy()[~finite] == 0).all(), label
        assert (np.abs(gv.cpu().numpy() - rv32) <= 2.0 ** -18 * mag + 1e-7).all(), label


def test_msda_backward_f64_offset_views():
    g = make_inputs(1, 2, 32, [(3, 2), (2, 1)], 2, Lq=2, mode="stress", seed=32, dtype=np.float64)
    g["value"] *= 0.01
    go = np.random.default_rng(1).standard_normal((1, 2, 64))
    rv, rl, rw = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], go)
    ss, lsi = _t(g["shapes"]), _t(g["lsi"])
    ops = {"value": _t(g["value"]), "loc": _t(g["loc"]), "attw": _t(g["attw"]), "grad_out": _t(go)}
    for label, where in cases(ops):
        a = displaced(ops, where)
        gv, gl, gw = A.ms_deform_attn_backward(a["value"], ss, lsi, a["loc"], a["attw"], a["grad_out"], 2)
        for got, ref in ((gv, rv), (gl, rl), (gw, rw)):
            np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-10, atol=1e-13, err_msg=label)


@pytest.mark.parametrize("shapes,Lq", [([(12, 16), (6, 8), (3, 4)], 50), (ENCODER_SHAPES, None)])
def test_msda_layer_module_bf16_offset_views(shapes, Lq):
    from test_msda_gpu import _layer_case, _layer_truth
    mod, q, ref, src, ss, lsi, mask = _layer_case(1, shapes, Lq, 2, 0, seed=41)
    truth, ref_bf16 = _layer_truth(mod, q, ref, src, ss, lsi, mask)
    rms = np.sqrt((truth ** 2).mean())
    err_ref = np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms
    ops = {"query": q, "input_flatten": src, "reference_points": ref}
    for label, where in cases(ops):
        a = displaced(ops, where)
        with torch.no_grad():
            out = mod(a["query"], a["reference_points"], a["input_flatten"], ss, lsi, mask)
        o = out.double().cpu().numpy()
        err = np.sqrt(((o - truth) ** 2).mean()) / rms
        assert err <= max(err_ref * 1.05, 4e-3), (label, err, err_ref)     # test_fused_layer_vs_oracle's bounds
        assert np.abs(o - truth).max() <= 2e-2 * np.abs(truth).max(), label


# ---- DCNv3 -----------------------------------------------------------------------------------------------------------
DCN_CASES = [(1, 24, 24, 4, 16, 3, 1, 1, 1, 1.0),      # group channels 16: pipelined / LDS-tiled forward
             (1, 20, 22, 2, 32, 3, 1, 1, 1, 1.0),      # 32: tiled forward, windowed backward
             (2, 9, 11, 3, 7, 3, 1, 1, 1, 0.7)]        # odd channel count: scalar kernels


def _dcn_inputs(N, H, W, G, C, k, s, p, d, seed):
    rng = np.random.default_rng(seed)
    Ho, Wo = OD.out_size(H, W, k, k, s, s, p, p, d, d)
    inp = rng.standard_normal((N, H, W, G * C)).astype(np.float32)
    off = (rng.standard_normal((N, Ho, Wo, G * k * k * 2)) * 2.5).astype(np.float32)
    msk = rng.random((N, Ho, Wo, G * k * k)).astype(np.float32)
    go = rng.standard_normal((N, Ho, Wo, G * C)).astype(np.float32)
    return inp, off, msk, go


@pytest.mark.parametrize("case", DCN_CASES, ids=["c16", "c32", "c7"])
def test_dcnv3_f32_f64_offset_views(case):
    N, H, W, G, C, k, s, p, d, sc = case
    inp, off, msk, go = _dcn_inputs(N, H, W, G, C, k, s, p, d, seed=H + C)
    geo = (k, k, s, s, p, p, d, d, G, C, sc)
    ref = OD.forward(inp, off, msk, *geo)
    ri, ro, rm = OD.backward(inp, off, msk, go, *geo)
    mi, _, _ = OD.backward(np.abs(inp), off, np.abs(msk), np.abs(go), *geo)
    ops = {"input": _t(inp), "offset": _t(off), "mask": _t(msk), "grad_out": _t(go)}
    for label, where in cases(ops):
        a = displaced(ops, where)
        out = D3.dcnv3_forward(a["input"], a["offset"], a["mask"], *geo)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-5, atol=2e-5, err_msg=label)
        gi, gof, gm = D3.dcnv3_backward(a["input"], a["offset"], a["mask"], *geo, a["grad_out"])
        assert (np.abs(gi.cpu().numpy() - ri) <= 2.0 ** -18 * mi + 1e-7).all(), label
        np.testing.assert_allclose(gof.cpu().numpy(), ro, rtol=2e-4, atol=3e-6 * (np.abs(ro).max() + 1e-12), err_msg=label)
        np.testing.assert_allclose(gm.cpu().numpy(), rm, rtol=2e-4, atol=3e-6 * (np.abs(rm).max() + 1e-12), err_msg=label)
    d64 = lambda x: x.astype(np.float64)   # noqa: E731
    ref = OD.forward(d64(inp), d64(off), d64(msk), *geo)
    ri, ro, rm = OD.backward(d64(inp), d64(off), d64(msk), d64(go), *geo)
    ops = {k_: v.double() for k_, v in ops.items()}
    for label, where in cases(ops):
        a = displaced(ops, where)
        out = D3.dcnv3_forward(a["input"], a["offset"], a["mask"], *geo)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-12, atol=1e-15, err_msg=label)
        gi, gof, gm = D3.dcnv3_backward(a["input"], a["offset"], a["mask"], *geo, a["grad_out"])
        for got, r in ((gi, ri), (gof, ro), (gm, rm)):
            np.testing.assert_allclose(got.cpu().numpy(), r, rtol=1e-10, atol=1e-12 * max(np.abs(r).max(), 1e-30) + 1e-18, err_msg=label)


@pytest.mark.parametrize("tag", ["c16", "c32", "c5"])
def test_dcnv3_f16_offset_views(tag):
    """Half precision against the fixture of the reference's twin (test_half_precision_forward_and_backward's bounds).  The native
    backward requires 16-byte aligned tensors; the reference accepts any contiguous view, e.g. a batch slice of `mask`."""
    g = load_golden("dcnv3_half.npz")
    kh, kw, sh, sw, ph, pw, dh, dw, M, Dc = [int(v) for v in g[f"{tag}.params"]]
    geo = (kh, kw, sh, sw, ph, pw, dh, dw, M, Dc, float(g[f"{tag}.offset_scale"]))
    h = lambda k: torch.from_numpy(g[f"{tag}.{k}"]).to(DEV)   # noqa: E731
    ops = {"input": h("input"), "offset": h("offset"), "mask": h("mask"), "grad_out": h("grad_out")}
    refs = {k: g[f"{tag}.{k}"].astype(np.float32) for k in ("grad_input", "grad_offset", "grad_mask")}
    variants = cases(ops)
    # the batch slice of ADVICE r6: mask[1:] of a batch one larger (misaligned whenever Ho*Wo*G*kh*kw % 8 != 0)
    m = ops["mask"]
    big = torch.cat([torch.full_like(m[:1], float("nan")), m])
    variants.append(("mask batch slice", {"mask_view": big[1:]}))
    for label, where in variants:
        a = displaced(ops, {k: v for k, v in where.items() if k in ops})
        if "mask_view" in where:
            a["mask"] = where["mask_view"]
        out = D3.dcnv3_forward(a["input"], a["offset"], a["mask"], *geo)
        np.testing.assert_allclose(out.float().cpu().numpy(), g[f"{tag}.out"].astype(np.float32), rtol=1e-3, atol=1e-3, err_msg=label)
        grads = D3.dcnv3_backward(a["input"], a["offset"], a["mask"], *geo, a["grad_out"])
        for ours, key in zip(grads, ("grad_input", "grad_offset", "grad_mask")):
            assert ours.dtype == torch.float16
            ref = refs[key]
            np.testing.assert_allclose(ours.float().cpu().numpy(), ref, rtol=2e-3, atol=2e-3 * max(np.abs(ref).max(), 1e-3),
                                       err_msg=f"{label} {key}")


# ---- region point sampling -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W,P", [(4, 256, 24, 24, 2304), (2, 17, 5, 9, 300)])   # pixel-weight form (HW % 4 == 0) / fallback
def test_point_sample_offset_views(N, C, H, W, P):
    torch.manual_seed(N + C)
    x = torch.randn(N, C, H, W)
    c = torch.rand(N, P, 2) * 1.3 - 0.15
    v = torch.rand(N, P) > 0.4
    ref = OR.point_sample(x, c)
    ref_mean = OR.masked_mean(ref, v)
    ops = {"input": x.to(DEV), "coords": c.to(DEV), "valid": v.to(torch.uint8).to(DEV)}
    for label, where in cases(ops):
        a = displaced(ops, where)
        with torch.no_grad():
            torch.testing.assert_close(R.point_sample(a["input"], a["coords"]).cpu(), ref, rtol=1e-5, atol=1e-5, msg=label)
            torch.testing.assert_close(R.point_sample_masked_mean(a["input"], a["coords"], a["valid"]).cpu(), ref_mean,
                                       rtol=1e-4, atol=1e-5, msg=label)


# ---- ViT path: attention and norm hooks, bridge, encoders -----------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_flash_attention_hook_offset_views(dtype):
    from test_vit_gpu import ulp_close
    from visionllm_amd.flash_attention import FlashAttention
    torch.manual_seed(7)
    B, S, H, Dh = 1, 577, 2, 64
    qkv = torch.randn(B, S, 3, H, Dh, device=DEV).to(dtype)
    q, k, v = qkv.double().cpu().permute(2, 0, 3, 1, 4).unbind(0)
    p = torch.softmax((q * Dh ** -0.5) @ k.transpose(-2, -1), -1)
    ref64, mag = (p @ v).transpose(1, 2), (p @ v.abs()).transpose(1, 2)
    for label, where in cases({"qkv": qkv}):
        out, _ = FlashAttention()(displaced({"qkv": qkv}, where)["qkv"])
        if dtype == torch.bfloat16:       # test_attention_vs_oracle's per-element bound
            ulp_close(out, ref64, 1.0, mag, 2.0 ** -8, f"FlashAttention bf16 {label}")
        else:                             # test_attention_fp16_vs_oracle's
            err = (out.double().cpu() - ref64).abs()
            ulp16 = torch.maximum(2.0 ** (torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -14))) - 10),
                                  torch.tensor(2.0 ** -24, dtype=torch.float64))
            assert ((err - 2.0 ** -10 * mag).clamp_min(0) / ulp16).max().item() <= 1.0, label


def test_rmsnorm_hook_offset_views():
    from test_vit_gpu import ulp_close
    from visionllm_amd.intern_vit import InternRMSNorm
    torch.manual_seed(9)
    C = 1024
    n = InternRMSNorm(C, eps=1e-6).to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        n.weight.copy_(1 + 0.2 * torch.randn(C))
    x = (torch.randn(3, 37, C, device=DEV) * 2 + 0.3).to(torch.bfloat16)
    xd, wd = x.double().cpu(), n.weight.detach().double().cpu()
    r64 = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-6) * wd
    for label, where in cases({"hidden_states": x}):
        ulp_close(n(displaced({"hidden_states": x}, where)["hidden_states"]), r64, 1.5, None, 0.0, f"InternRMSNorm hook {label}")


def _pack_parameters(module, off):
    """Make every parameter of `module` a view into ONE flat buffer, each at byte offset `off` (mod 16) -- how a loader that maps a
    checkpoint into one storage hands them over.  Returns the buffer."""
    params = list(module.parameters())
    es = params[0].element_size()
    step = off // es
    sizes = [p.numel() for p in params]
    flat = torch.full((sum(sizes) + (len(params) + 1) * (16 // es + step),), float("nan"), dtype=params[0].dtype, device=DEV)
    pos = 0
    for p, n in zip(params, sizes):
        pos = (pos + 16 // es - 1) // (16 // es) * (16 // es) + step      # 16-byte boundary + the displacement
        view = flat[pos:pos + n].view(p.shape)
        view.copy_(p.data)
        p.data = view
        assert p.data_ptr() % 16 == off % 16
        pos += n
    return flat


@pytest.mark.parametrize("kind,ps", [("internvl_mlp", True), ("linear", False)])
def test_bridge_offset_views_and_packed_parameters(kind, ps):
    from visionllm_amd.bridge import build_vl_bridge
    from test_vit_gpu import close
    torch.manual_seed(3)
    n, hw, C, Cl = 3, 8, 128, 256
    hidden = torch.randn(n, 1 + hw * hw, C).to(torch.bfloat16)
    br = build_vl_bridge(kind, C, Cl, use_pixelshuffle=ps)
    with torch.no_grad():
        for p in br.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    sd = {k: v.detach().to(torch.bfloat16).float() for k, v in br.state_dict().items()}
    ref = V.bridge_forward(sd, kind, V.select_features([hidden.float(), hidden.float()], -2, ps))
    br = br.to(DEV).to(torch.bfloat16).requires_grad_(False)
    aligned = br.project_hidden_state(hidden.to(DEV), ps)
    close(aligned, ref, 1.5e-2, f"bridge {kind}")
    for label, where in cases({"hidden": hidden.to(DEV)}):
        out = br.project_hidden_state(displaced({"hidden": hidden.to(DEV)}, where)["hidden"], ps)
        close(out, ref, 1.5e-2, f"bridge {kind} {label}")
        assert torch.equal(out, aligned), label
    for off in (2, 8, 14):
        _pack_parameters(br, off)
        h, _ = placed(hidden, off)
        out = br.project_hidden_state(h, ps)
        close(out, ref, 1.5e-2, f"bridge {kind} packed @{off}")
        assert torch.equal(out, aligned), off


@pytest.mark.parametrize("arch", ["internvit", "clip"])
def test_encoder_pixel_offset_views_and_packed_parameters(arch):
    """pixel_values displaced (bf16 and fp32: the patch gather reads scalars, nothing is copied) and a model whose parameters are
    views into one packed buffer (the plan passes aligned copies): the hidden states of the aligned run, bit for bit, and the
    oracle's bound (test_vit_gpu.py::_check_states); CLIP's pooled output is the post-layernorm of the class token."""
    from test_vit_gpu import _check_states, _oracle_errors
    if arch == "internvit":
        from visionllm_amd.intern_vit import InternVisionConfig, InternVisionModel
        g = load_golden("internvit_small_d64.npz")
        cfgd = ast.literal_eval(str(g["cfg"]))
        model = InternVisionModel(InternVisionConfig(**cfgd))
        fwd = V.intern_vit_forward
    else:
        from transformers import CLIPVisionConfig
        from visionllm_amd.clip_vit import CLIPVisionModel
        g = load_golden("clip_small_d64.npz")
        cfgd = ast.literal_eval(str(g["cfg"]))
        model = CLIPVisionModel(CLIPVisionConfig(**cfgd))
        fwd = lambda s, c, xx: V.clip_vit_forward(s, c, xx)   # noqa: E731
    sd = golden_sd(g)
    model.load_state_dict(sd, strict=arch == "internvit")
    model = model.to(DEV).to(torch.bfloat16)
    x = torch.from_numpy(g["pixel_values"])
    ref, lo = _oracle_errors(fwd, sd, cfgd, x)
    base = model(x.to(torch.bfloat16).to(DEV), output_hidden_states=True)
    _check_states(base.hidden_states, ref, lo, arch)
    for dtype in (torch.bfloat16, torch.float32):
        px = x.to(torch.bfloat16).to(dtype).to(DEV)
        for label, where in cases({"pixel_values": px}):
            out = model(displaced({"pixel_values": px}, where)["pixel_values"], output_hidden_states=True)
            for i, (a_, b_) in enumerate(zip(out.hidden_states, base.hidden_states)):
                assert torch.equal(a_, b_), f"{arch} {dtype} {label} hs[{i}]"
            assert torch.equal(out.pooler_output, base.pooler_output), label
    for off in (2, 6, 8):
        _pack_parameters(model, off)
        px, _ = placed(x.to(torch.bfloat16), off)
        out = model(px, output_hidden_states=True)
        for i, (a_, b_) in enumerate(zip(out.hidden_states, base.hidden_states)):
            assert torch.equal(a_, b_), f"{arch} packed @{off} hs[{i}]"
        assert torch.equal(out.pooler_output, base.pooler_output), f"{arch} packed @{off}"


# ---- token splices and the row movers (in place: the bytes around the view stay as they were) -----------------------
def test_splice_visual_tokens_offset_views():
    from visionllm_amd.splice import splice_visual_tokens
    torch.manual_seed(1)
    B, L, C, T, IMP = 3, 40, 64, 6, 7
    ids = torch.randint(10, 50, (B, L))
    ids[0, 3:3 + 2 * T] = IMP
    ids[2, 10:10 + T] = IMP
    split = [2, 1, 1]
    emb = torch.randn(B, L, C).to(torch.bfloat16)
    feats = torch.randn(sum(split), T, C).to(torch.bfloat16)
    ref = emb.clone().reshape(B * L, C)
    sel = ids == IMP
    has = sel.sum(-1) != 0
    has_t = torch.cat([has[i][None].repeat(split[i]) for i in range(B)])
    ref[sel.reshape(-1)] = feats[has_t].reshape(-1, C)
    for label, where in cases({"inputs_embeds": emb, "image_features": feats}):
        e, parent = placed(emb, where.get("inputs_embeds", 0))
        before = bits(parent)
        f = displaced({"image_features": feats.to(DEV)}, where)["image_features"]
        out = splice_visual_tokens(e, ids.to(DEV), IMP, f, split)
        assert out.data_ptr() == e.data_ptr() and torch.equal(e.cpu().reshape(B * L, C), ref), label
        k = (e.data_ptr() - parent.data_ptr())
        after = bits(parent)
        assert torch.equal(after[:k], before[:k]) and torch.equal(after[k + e.numel() * 2:], before[k + e.numel() * 2:]), label


def test_splice_region_tokens_offset_views():
    from visionllm_amd.splice import splice_region_tokens
    torch.manual_seed(2)
    B, L, C, REG = 2, 30, 128, 5
    ids = torch.randint(10, 50, (B, L))
    ids[0, [2, 9]] = REG
    ids[1, [0, 17, 29]] = REG
    emb = torch.randn(B, L, C).to(torch.bfloat16)
    feats = torch.randn(5, C).to(torch.bfloat16)
    ref = emb.clone()
    ref[ids == REG] = feats
    for label, where in cases({"inputs_embeds": emb, "region_features": feats}):
        e, parent = placed(emb, where.get("inputs_embeds", 0))
        before = bits(parent)
        f = displaced({"region_features": feats.to(DEV)}, where)["region_features"]
        with torch.no_grad():
            splice_region_tokens(e, ids.to(DEV), REG, f)
        assert torch.equal(e.cpu(), ref), label
        k = e.data_ptr() - parent.data_ptr()
        after = bits(parent)
        assert torch.equal(after[:k], before[:k]) and torch.equal(after[k + e.numel() * 2:], before[k + e.numel() * 2:]), label


def _last_error():
    return _lib.lib().vllm_last_error().decode()


@pytest.mark.parametrize("entry", ["scatter_rows", "copy_rows"])
def test_row_movers_c_abi_alignment_contract(entry):
    """vllm_scatter_rows_bf16 (exported, timed by bench.py --full, otherwise untested) and vllm_copy_rows_bf16: aligned, an exact
    copy against torch indexing with every guard byte untouched; src or dst off 16 bytes: VLLM_EINVAL naming the requirement, and
    nothing written."""
    L_ = _lib.lib()
    torch.manual_seed(5)
    n, C, dst_rows = 37, 72, 50
    src = torch.randn(n, C).to(torch.bfloat16)
    idx = torch.randperm(dst_rows)[:n]
    idx[3] = dst_rows + 4            # out of range: skipped
    idx[8] = -1
    dst0 = torch.randn(dst_rows, C).to(torch.bfloat16)
    want = dst0.clone()
    ok = (idx >= 0) & (idx < dst_rows)
    want[idx[ok]] = src[ok]
    st = _lib.current_stream(torch.device(DEV))
    di = idx.to(DEV)

    def call(s, d):
        if entry == "scatter_rows":
            return L_.vllm_scatter_rows_bf16(_lib.ptr(s), _lib.ptr(di), _lib.ptr(d), n, C, dst_rows, st)
        return L_.vllm_copy_rows_bf16(_lib.ptr(s), None, _lib.ptr(d), _lib.ptr(di), n, C, n, dst_rows, st)

    for so in (0,) + OFFSETS[torch.bfloat16]:
        for do in (0,) + OFFSETS[torch.bfloat16]:
            if so and do and so != do:
                continue
            s, _ = placed(src, so) if so else (src.to(DEV), None)
            d, parent = placed(dst0, do)
            before = bits(parent)
            rc = call(s, d)
            torch.cuda.synchronize()
            after = bits(parent)
            k = d.data_ptr() - parent.data_ptr()
            if so % 16 == 0 and do % 16 == 0:
                assert rc == 0, _last_error()
                assert torch.equal(d.cpu(), want)
                assert torch.equal(after[:k], before[:k]) and torch.equal(after[k + d.numel() * 2:], before[k + d.numel() * 2:])
            else:
                assert rc == -1 and "16-byte aligned" in _last_error(), (so, do, rc, _last_error())
                assert torch.equal(after, before), (so, do)


def test_gemm_output_view_c_abi_contract():
    """vllm_gemm_bf16 with Y a view into a caller's buffer: where Y's alignment meets the documented requirement (8 bytes) the
    result is the aligned call's, bit for bit, and no byte outside the view changes; elsewhere VLLM_EINVAL names the requirement
    and nothing is written."""
    L_ = _lib.lib()
    torch.manual_seed(6)
    M, N, K = 300, 256, 128
    X = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    W = (torch.randn(N, K, device=DEV) * 0.05).to(torch.bfloat16)
    b = (torch.randn(N, device=DEV) * 0.1).to(torch.bfloat16)
    st = _lib.current_stream(torch.device(DEV))
    Y0 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    assert L_.vllm_gemm_bf16(_lib.ptr(X), _lib.ptr(W), _lib.ptr(b), _lib.ptr(Y0), M, N, K, K, K, N, _lib.EPI_BIAS, None, None, 0, 0, st) == 0
    from test_vit_gpu import close
    close(Y0, X.float() @ W.float().t() + b.float(), 1e-2, "gemm")
    for off in OFFSETS[torch.bfloat16]:
        Y, parent = placed(torch.zeros(M, N, dtype=torch.bfloat16), off)
        before = bits(parent)
        rc = L_.vllm_gemm_bf16(_lib.ptr(X), _lib.ptr(W), _lib.ptr(b), _lib.ptr(Y), M, N, K, K, K, N, _lib.EPI_BIAS, None, None, 0, 0, st)
        torch.cuda.synchronize()
        after = bits(parent)
        k = Y.data_ptr() - parent.data_ptr()
        if off % 8 == 0:
            assert rc == 0, _last_error()
            assert torch.equal(Y, Y0), off
            assert torch.equal(after[:k], before[:k]) and torch.equal(after[k + Y.numel() * 2:], before[k + Y.numel() * 2:]), off
        else:
            assert rc == -1 and "8-byte aligned" in _last_error(), (off, _last_error())
            assert torch.equal(after, before), off


def test_native_alignment_errors_name_the_requirement():
    """Entry points with an alignment requirement (include/vllm_hip.h) refuse a pointer that misses it with VLLM_EINVAL and a
    message naming it -- never a silent wrong answer."""
    L_ = _lib.lib()
    st = _lib.current_stream(torch.device(DEV))
    x, _ = placed(torch.randn(4, 64).to(torch.bfloat16), 2)
    w = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    y = torch.empty(4, 64, dtype=torch.bfloat16, device=DEV)
    assert L_.vllm_rmsnorm_bf16(_lib.ptr(x), 64, _lib.ptr(w), _lib.ptr(y), 64, 4, 64, 1e-6, st) == -1
    assert "16-byte aligned" in _last_error()
    assert L_.vllm_layernorm_bf16(_lib.ptr(x), 64, _lib.ptr(w), _lib.ptr(w), _lib.ptr(y), 64, 4, 64, 1e-5, st) == -1
    assert "16-byte aligned" in _last_error()
    qkv, _ = placed(torch.randn(1, 8, 3, 1, 64).to(torch.bfloat16), 8)
    out = torch.empty(1, 8, 1, 64, dtype=torch.bfloat16, device=DEV)
    assert L_.vllm_attn_fwd_qkvpacked_bf16(_lib.ptr(qkv), _lib.ptr(out), 1, 8, 1, 64, 0.125, st) == -1
    assert "16-byte aligned" in _last_error()
    c, _ = placed(torch.rand(1, 5, 2), 4)
    inp = torch.randn(1, 3, 4, 4, device=DEV)
    o = torch.empty(1, 3, 5, device=DEV)
    assert L_.vllm_point_sample_f32(_lib.ptr(inp), _lib.ptr(c), 1, 3, 4, 4, 5, _lib.ptr(o), st) == -1
    assert "8-byte aligned" in _last_error()
    torch.cuda.synchronize()


# ---- caller streams --------------------------------------------------------------------------------------------------
SLEEP_CYCLES = 4_000_000            # ~2 ms at the MI355X's clock: the side stream is still busy when the op is enqueued


def _op_cases():
    """name -> (run(**inputs) -> tensor or tuple, inputs): small shapes of every public op."""
    from visionllm_amd.bridge import build_vl_bridge
    from visionllm_amd.flash_attention import FlashAttention
    from visionllm_amd.intern_vit import InternRMSNorm, InternVisionConfig, InternVisionModel
    from visionllm_amd.splice import splice_region_tokens, splice_visual_tokens
    torch.manual_seed(0)
    ops = {}
    g = make_inputs(2, 8, 32, [(21, 19), (11, 10), (6, 5), (3, 3)], 4, Lq=120, mode="stress", seed=2)
    ss, lsi = _t(g["shapes"]), _t(g["lsi"])
    ops["msda_forward"] = (lambda value, loc, attw: A.ms_deform_attn_forward(value, ss, lsi, loc, attw, 64),
                           {"value": _t(g["value"]), "loc": _t(g["loc"]), "attw": _t(g["attw"])})
    go = torch.randn(2, 120, 256, device=DEV)
    ops["msda_backward"] = (lambda value, loc, attw, grad_out: tuple(A.ms_deform_attn_backward(value, ss, lsi, loc, attw, grad_out, 64)),
                            {"value": _t(g["value"]), "loc": _t(g["loc"]), "attw": _t(g["attw"]), "grad_out": go})
    inp, off, msk, gout = _dcn_inputs(1, 20, 22, 2, 32, 3, 1, 1, 1, seed=4)
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 2, 32, 1.0)
    ops["dcnv3_forward"] = (lambda input, offset, mask: D3.dcnv3_forward(input, offset, mask, *geo),
                            {"input": _t(inp), "offset": _t(off), "mask": _t(msk)})
    ops["dcnv3_backward_f16"] = (lambda input, offset, mask, grad_out: D3.dcnv3_backward(input, offset, mask, *geo, grad_out),
                                 {"input": _t(inp).half(), "offset": _t(off).half(), "mask": _t(msk).half(), "grad_out": _t(gout).half()})
    cv = torch.rand(2, 300, device=DEV) > 0.3
    ops["point_sample"] = (lambda input, coords: (R.point_sample(input, coords), R.point_sample_masked_mean(input, coords, cv)),
                           {"input": torch.randn(2, 64, 24, 24, device=DEV), "coords": torch.rand(2, 300, 2, device=DEV)})
    fa = FlashAttention()
    ops["flash_attention"] = (lambda qkv: fa(qkv)[0], {"qkv": torch.randn(1, 193, 3, 2, 64, device=DEV).to(torch.bfloat16)})
    rn = InternRMSNorm(256).to(DEV).to(torch.bfloat16)
    ops["rmsnorm"] = (lambda x: rn(x), {"x": torch.randn(2, 33, 256, device=DEV).to(torch.bfloat16)})
    br = build_vl_bridge("internvl_mlp", 128, 256, use_pixelshuffle=True).to(DEV).to(torch.bfloat16).requires_grad_(False)
    ops["bridge"] = (lambda h: br.project_hidden_state(h, True), {"h": torch.randn(3, 65, 128, device=DEV).to(torch.bfloat16)})
    gv = load_golden("internvit_small_d64.npz")
    enc = InternVisionModel(InternVisionConfig(**ast.literal_eval(str(gv["cfg"]))))
    enc.load_state_dict(golden_sd(gv))
    enc = enc.to(DEV).to(torch.bfloat16)
    ops["encoder"] = (lambda px: enc(px, output_hidden_states=True).hidden_states,
                      {"px": torch.from_numpy(gv["pixel_values"]).to(DEV).to(torch.bfloat16)})
    ids = torch.randint(10, 50, (2, 40), device=DEV)
    ids[0, 3:9] = 7
    ids[1, 20:26] = 7
    ops["splice_visual_tokens"] = (lambda emb, feats: splice_visual_tokens(emb, ids, 7, feats),
                                   {"emb": torch.randn(2, 40, 64, device=DEV).to(torch.bfloat16),
                                    "feats": torch.randn(2, 6, 64, device=DEV).to(torch.bfloat16)})
    rid = torch.randint(10, 50, (2, 40), device=DEV)
    rid[0, 5] = rid[1, 11] = 3
    ops["splice_region_tokens"] = (lambda emb, feats: splice_region_tokens(emb, rid, 3, feats),
                                   {"emb": torch.randn(2, 40, 64, device=DEV).to(torch.bfloat16),
                                    "feats": torch.randn(2, 64, device=DEV).to(torch.bfloat16)})
    from test_msda_gpu import _layer_case
    mod, q, ref, src, lss, llsi, mask = _layer_case(1, [(12, 16), (6, 8), (3, 4)], 50, 2, 0, seed=3)
    ops["msda_layer"] = (lambda q, src: mod(q, ref, src, lss, llsi, mask), {"q": q, "src": src})
    return ops


OP_NAMES = ["msda_forward", "msda_backward", "dcnv3_forward", "dcnv3_backward_f16", "point_sample", "flash_attention", "rmsnorm",
            "bridge", "encoder", "splice_visual_tokens", "splice_region_tokens", "msda_layer"]


ATOMIC_SUMS = {("msda_backward", 0), ("dcnv3_backward_f16", 0)}     # grad_value / grad_input


@pytest.fixture(scope="module")
def op_cases():
    return _op_cases()


def _host(r):
    return [t.cpu() for t in (r if isinstance(r, (tuple, list)) else (r,)) if t is not None]


@pytest.mark.parametrize("name", OP_NAMES)
def test_op_runs_on_the_callers_stream(name, op_cases):
    """On a side stream s: a ~2 ms sleep, then the in-place writes that produce the op's inputs, then the op under
    torch.cuda.stream(s).  The result must equal the default-stream call bit for bit, and a consumer on s (the copy to the host,
    which waits for s only) must see it: an op that enqueued anywhere but s would read the NaN the inputs held before."""
    run, inputs = op_cases[name]
    with torch.no_grad():
        want = _host(run(**{k: v.clone() for k, v in inputs.items()}))
        bufs = {k: torch.full_like(v, _sentinel(v.dtype)) for k, v in inputs.items()}
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            torch.cuda._sleep(SLEEP_CYCLES)
            for k, v in inputs.items():
                bufs[k].copy_(v)
            got = _host(run(**bufs))            # (.cpu() synchronises the current stream: s)
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if (name, i) in ATOMIC_SUMS:     # floating-point atomics: the order of the sums (and so the last bits) varies run to run
            torch.testing.assert_close(a.float(), b.float(), rtol=1e-3, atol=1e-3 * float(b.float().abs().max()), msg=name)
            continue
        assert torch.equal(a.view(torch.uint8) if a.dtype != torch.bool else a, b.view(torch.uint8) if b.dtype != torch.bool else b), \
            f"{name}: output {i} differs from the default-stream call"


def _vitl_width_encoder():
    from visionllm_amd.intern_vit import InternVisionConfig, InternVisionModel
    torch.manual_seed(1)
    cfg = dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=4, image_size=448, patch_size=14,
               qk_normalization=False, qkv_bias=True, hidden_act="gelu", layer_norm_eps=1e-6)
    model = InternVisionModel(InternVisionConfig(**cfg))
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if p.dim() >= 2 or "embedding" in n_:
                p.normal_(0, 0.02)
            elif n_.endswith("ls1") or n_.endswith("ls2"):
                p.fill_(0.1)
    return model.to(DEV).to(torch.bfloat16).eval()


def test_encoder_and_det_head_on_two_streams_are_bit_identical_to_serial():
    """The encoder (ViT-L width, 4 tiles of 1025 tokens) on stream A while the projector and the fused deformable-attention layer run
    on stream B, started after a short sleep so that they overlap it; three rounds with different sleeps (one measurement each,
    not a retry).  The three used to share one scratch buffer per device: every output must equal the serial run's bit for bit."""
    from test_msda_gpu import _layer_case
    from visionllm_amd.bridge import build_vl_bridge
    enc = _vitl_width_encoder()
    px = torch.randn(4, 3, 448, 448, device=DEV).to(torch.bfloat16)
    br = build_vl_bridge("internvl_mlp", 1024, 1024, use_pixelshuffle=True).to(DEV).to(torch.bfloat16).requires_grad_(False)
    hid = torch.randn(2, 1 + 32 * 32, 1024, device=DEV).to(torch.bfloat16)
    mod, q, ref, src, ss, lsi, mask = _layer_case(1, ENCODER_SHAPES, None, 2, 0, seed=5)
    with torch.no_grad():
        A.remember_geometry(ss)
        serial = (enc(px, output_hidden_states=True).hidden_states, br.project_hidden_state(hid, True), mod(q, ref, src, ss, lsi, mask))
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
        for sleep in (20_000, 400_000, 2_000_000):
            sa.wait_stream(torch.cuda.current_stream())
            sb.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(sa):
                hs = enc(px, output_hidden_states=True).hidden_states
            with torch.cuda.stream(sb):
                torch.cuda._sleep(sleep)
                tok = br.project_hidden_state(hid, True)
                det = mod(q, ref, src, ss, lsi, mask)
            torch.cuda.synchronize()
            for i, (a, b) in enumerate(zip(hs, serial[0])):
                assert torch.equal(a, b), f"sleep {sleep}: encoder hs[{i}]"
            assert torch.equal(tok, serial[1]), f"sleep {sleep}: projector"
            assert torch.equal(det, serial[2]), f"sleep {sleep}: deformable-attention layer"


def test_scratch_growth_on_another_stream():
    """The projector on stream A with a small batch, then -- without a synchronisation -- on stream B with a batch large enough to
    grow the scratch: both results right (the buffer stream A's kernels use is neither replaced nor reused under them)."""
    from visionllm_amd.bridge import build_vl_bridge
    torch.manual_seed(8)
    br = build_vl_bridge("internvl_mlp", 256, 512, use_pixelshuffle=True).to(DEV).to(torch.bfloat16).requires_grad_(False)
    small = torch.randn(1, 1 + 16 * 16, 256, device=DEV).to(torch.bfloat16)
    large = torch.randn(24, 1 + 32 * 32, 256, device=DEV).to(torch.bfloat16)
    sa, sb = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    with torch.no_grad():
        want_small, want_large = br.project_hidden_state(small, True), br.project_hidden_state(large, True)
        torch.cuda.synchronize()
        _lib._workspaces.clear()
        br.project_hidden_state(small, True)   # a small scratch made on the default stream (where a shared one would live)
        torch.cuda.synchronize()
        sa.wait_stream(torch.cuda.current_stream())
        sb.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(sa):
            torch.cuda._sleep(SLEEP_CYCLES)
            got_small = br.project_hidden_state(small, True)
        with torch.cuda.stream(sb):
            got_large = br.project_hidden_state(large, True)
        # memory the default stream gets back from the allocator now, written while stream A's projector may still be running
        torch.cuda._sleep(SLEEP_CYCLES)
        junk = torch.full((small.numel() * 64,), 7, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
    del junk
    assert torch.equal(got_small, want_small) and torch.equal(got_large, want_large)
