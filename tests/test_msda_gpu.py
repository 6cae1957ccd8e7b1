"""GPU parity tests for the MSDA operator: HIP (through the C ABI) vs the CPU oracle / golden fixtures."""
import json

import numpy as np
import pytest
import torch

import lattice_inputs as LI
from conftest import load_golden
from msda_inputs import CFG4_SHAPES, make_inputs
from oracle import msda as O
from visionllm_amd import ms_deform_attn as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(dtype) if dtype is not None else t


def _run(g, dtype=torch.float32):
    fd = dtype if dtype != torch.bfloat16 else torch.float32
    return A.ms_deform_attn_forward(_t(g["value"], dtype), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"], fd),
                                    _t(g["attw"], fd), 64)


def _run_general(g):
    """fp32 forward with the host's geometry hint forced to VLLM_GEO_GENERAL: at the encoder shape (Lq == S, D 32, P 4) the library
    then runs generation 4 (msda_tiled4.hip) on any level maps, nested ones included."""
    from visionllm_amd import _lib
    v, ss, lsi, loc, w = _t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"])
    B, S, M, D = v.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    out = torch.empty((B, Lq, M * D), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().vllm_msda_forward_f32_geo(_lib.ptr(v), _lib.ptr(ss), _lib.ptr(lsi), _lib.ptr(loc), _lib.ptr(w), B, S, M, D, L,
                                                    Lq, P, A.GEO_GENERAL, _lib.ptr(out), _lib.current_stream(v.device)))
    return out


def _check_bf16_route(g):
    """vllm_msda_forward_bf16 (generation 6 on exact 2x pyramids, the gather kernel otherwise): two runs bit-identical, finite,
    the oracle on the bf16-rounded value within the bound of test_generation6_bf16_value, and the bf16 gather route
    (msda_tiled = 0) within one bf16 ulp (+ the 2e-6 floor of the fp32 kernel comparisons, for sums that cancel)."""
    from visionllm_amd import _lib
    vb = torch.from_numpy(g["value"]).to(torch.bfloat16)
    ref = O.forward(vb.float().numpy(), g["shapes"], g["lsi"], g["loc"], g["attw"])
    run = lambda: A.ms_deform_attn_forward(vb.to(DEV), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"]), 64)
    old = _lib.set_option("msda_tiled", 1)
    try:
        auto, again = run(), run()
        _lib.set_option("msda_tiled", 0)
        gather = run()
    finally:
        _lib.set_option("msda_tiled", old)
    assert auto.dtype == torch.bfloat16 and gather.dtype == torch.bfloat16
    assert torch.equal(auto, again), "race: two runs of the bf16 operator differ"
    assert torch.isfinite(auto).all()
    a, b = auto.float().cpu().numpy(), gather.float().cpu().numpy()
    err = np.abs(a - ref)
    assert (err <= 2.0 ** -8 * np.abs(ref) + 1e-6).all(), err.max()   # one rounding to bf16 (half an ulp = 2^-9 relative)
    m = np.maximum(np.abs(a), np.abs(b))
    ulp = np.exp2(np.floor(np.log2(np.where(m > 0, m, 1.0))) - 7)    # bf16: 8 significant bits
    assert (np.abs(a - b) <= ulp + 2e-6).all(), np.abs(a - b).max()


GOLD = ["msda_kat_seed3.npz", "msda_stress_small.npz", "msda_stress_d32.npz", "msda_odd_channels.npz"]


@pytest.mark.parametrize("name", GOLD)
def test_forward_f64_vs_reference_golden(name):
    g = load_golden(name)
    out = _run(g, torch.float64).cpu().numpy()
    np.testing.assert_allclose(out, g["out_f64"], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", GOLD)
def test_forward_f32_vs_reference_golden(name):
    g = load_golden(name)
    out = _run(g, torch.float32).cpu().numpy().astype(np.float64)
    ref = g["out_f64"]
    err = np.abs(out - ref).max()
    if name == "msda_kat_seed3.npz":
        # the reference's own float thresholds (test_ms_deformable_attn.py:129-134)
        assert err < 1e-9 and (np.abs(out - ref) / np.abs(ref)).max() < 1e-6
    assert err <= 2e-6 * max(np.abs(ref).max(), 1e-3)


@pytest.mark.parametrize("mode,D,M,P", [("encoder_like", 32, 8, 4), ("stress", 32, 8, 4), ("stress", 16, 4, 2),
                                         ("stress", 64, 2, 8), ("stress", 4, 3, 1), ("stress", 128, 2, 4),
                                         ("stress", 20, 2, 3), ("stress", 256, 1, 4)])
def test_forward_f32_vs_oracle_and_index_exact(mode, D, M, P):
    shapes = [(21, 19), (11, 10), (6, 5), (3, 3)]
    g = make_inputs(3, M, D, shapes, P, Lq=None if mode == "encoder_like" else 333, mode=mode, seed=D + P)
    out = _run(g).cpu().numpy()
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    np.testing.assert_allclose(out, ref, rtol=2e-5, atol=2e-5)
    # integer part: exact
    h, w, mk = A.sample_index(_t(g["shapes"]), _t(g["loc"]))
    ho, wo, mo = O.sample_index(g["shapes"], g["loc"])
    assert np.array_equal(mk.cpu().numpy(), mo)
    assert np.array_equal(h.cpu().numpy(), ho) and np.array_equal(w.cpu().numpy(), wo)


def test_forward_bf16_variant():
    shapes = [(21, 19), (11, 10), (6, 5), (3, 3)]
    g = make_inputs(2, 8, 32, shapes, 4, Lq=200, mode="stress", seed=5)
    vb = torch.from_numpy(g["value"]).to(torch.bfloat16)
    out = A.ms_deform_attn_forward(vb.to(DEV), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"]), 64)
    ref = O.forward(vb.float().numpy(), g["shapes"], g["lsi"], g["loc"], g["attw"])
    # only the final rounding to bf16 differs: 2^-8 relative
    np.testing.assert_allclose(out.float().cpu().numpy(), ref, rtol=8e-3, atol=8e-3)


def test_full_size_cfg4_vs_oracle_and_properties():
    """BASELINE cfg 4 shapes (168^2..21^2, M8 D32 P4), B=2: whole-tensor oracle comparison + linearity."""
    g = make_inputs(2, 8, 32, CFG4_SHAPES, 4, mode="encoder_like", seed=0)
    out = _run(g)
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    # tight: a fused loc*H-0.5 (one rounding instead of the reference's two) shows up as ~1e-5 wherever loc*H crosses
    # a power of two (regression test for the backend-contraction bug found on hardware)
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=4e-6, atol=4e-6)
    h, w, mk = A.sample_index(_t(g["shapes"]), _t(g["loc"]))
    ho, wo, mo = O.sample_index(g["shapes"], g["loc"])
    assert np.array_equal(mk.cpu().numpy(), mo) and np.array_equal(h.cpu().numpy(), ho) \
        and np.array_equal(w.cpu().numpy(), wo)
    # linearity in value: f(2*v + v2) == 2*f(v) + f(v2)
    v2 = torch.randn_like(_t(g["value"]))
    g2 = dict(g)
    lhs = A.ms_deform_attn_forward(2 * _t(g["value"]) + v2, _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]),
                                   _t(g["attw"]), 64)
    rhs = 2 * out + A.ms_deform_attn_forward(v2, _t(g2["shapes"]), _t(g2["lsi"]), _t(g2["loc"]), _t(g2["attw"]), 64)
    torch.testing.assert_close(lhs, rhs, rtol=1e-4, atol=1e-4)
    # constant value + interior points -> weights sum to one -> output == the constant
    gi = make_inputs(1, 8, 32, CFG4_SHAPES, 4, Lq=1000, mode="stress", seed=3)
    loc = np.clip(gi["loc"], 0.2, 0.8)
    cst = torch.full((1, gi["value"].shape[1], 8, 32), 1.25, device=DEV)
    o = A.ms_deform_attn_forward(cst, _t(gi["shapes"]), _t(gi["lsi"]), _t(loc), _t(gi["attw"]), 64)
    torch.testing.assert_close(o, torch.full_like(o, 1.25), rtol=1e-5, atol=1e-5)


def test_full_size_cfg4_batch8_vs_oracle():
    """BASELINE configs[3] at its stated batch size (B = 8, the shape bench.py times): whole-tensor comparison with the C
    oracle + index-exact integer parts."""
    g = make_inputs(8, 8, 32, CFG4_SHAPES, 4, mode="encoder_like", seed=8)
    out = _run(g)
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=4e-6, atol=4e-6)
    h, w, mk = A.sample_index(_t(g["shapes"]), _t(g["loc"]))
    ho, wo, mo = O.sample_index(g["shapes"], g["loc"])
    assert np.array_equal(mk.cpu().numpy(), mo) and np.array_equal(h.cpu().numpy(), ho) and np.array_equal(w.cpu().numpy(), wo)


@pytest.mark.parametrize("mode", ["encoder_like", "wide_offsets", "odd_geometry"])
def test_tiled_kernel_matches_gather_kernel(mode):
    """The LDS-tiled kernel (encoder shape: Lq == S, D=32, P=4) runs the same arithmetic as the gather kernel."""
    from visionllm_amd import _lib
    if mode == "odd_geometry":      # maps whose sizes are not multiples of the 8x16 query tile, 3 levels
        shapes = [(61, 83), (31, 42), (9, 5)]
        g = make_inputs(2, 8, 32, shapes, 4, mode="encoder_like", seed=4)
    else:
        g = make_inputs(2, 8, 32, CFG4_SHAPES, 4, mode="encoder_like", seed=1)
    if mode == "wide_offsets":      # far-away samples: windows exceed the LDS budget -> per-level global fallback
        rng = np.random.default_rng(0)
        g["loc"] = (g["loc"] + rng.standard_normal(g["loc"].shape).astype(np.float32) * 0.2).astype(np.float32)
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    old = _lib.set_option("msda_tiled", 0)
    try:
        plain = _run(g)
        _lib.set_option("msda_tiled", 1)
        # automatic (generation 9 on nested maps, else 4); generation 4 on any maps through the GEO_GENERAL hint
        runs = {"automatic": (_run(g), _run(g)), "generation 4": (_run_general(g), _run_general(g))}
    finally:
        _lib.set_option("msda_tiled", old)
    for variant, (tiled, again) in runs.items():
        assert torch.equal(tiled, again), f"race: two runs of the same kernel differ ({variant})"
        # same arithmetic per (query, point); only the compiler's contraction choices may differ between kernels
        torch.testing.assert_close(tiled, plain, rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(tiled.cpu().numpy(), ref, rtol=4e-6, atol=4e-6)



MSDA_TILED_ACCEPTED = (0, 1, 21)


def test_msda_tiled_0_1_21_match_the_oracle():
    """Every value vllm_set_option("msda_tiled") accepts, at the cfg-4 encoder shape (nested 2x pyramid, Lq == S, D = 32, P = 4,
    L = 4): 0 gather; 1 generation 9; 21 generation 9 with its phase clock.  The phase-clock build produces the profiles' numbers: its
    results must be the oracle's too.  Each value: oracle tolerance of test_tiled_kernel_matches_gather_kernel, two runs bit-identical."""
    from visionllm_amd import _lib
    g = make_inputs(2, 8, 32, CFG4_SHAPES, 4, mode="encoder_like", seed=1)
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    old = _lib.set_option("msda_tiled", 1)
    try:
        for variant in MSDA_TILED_ACCEPTED:
            assert _lib.set_option("msda_tiled", variant) >= 0, variant
            out = _run(g)
            again = _run(g)
            assert torch.equal(out, again), f"msda_tiled = {variant}: two runs differ"
            np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=4e-6, atol=4e-6, err_msg=f"msda_tiled = {variant}")
    finally:
        _lib.set_option("msda_tiled", old)

PYRAMIDS = {
    "L4_partial_tiles": [(72, 104), (36, 52), (18, 26), (9, 13)],     # 104 / 16 = 6.5 tiles per row
    "L3": [(64, 80), (32, 40), (16, 20)],
    "L2_odd_rows": [(76, 64), (38, 32)],                              # 76 / 8 = 9.5 tile rows
    "L1": [(72, 64)],
    # nested maps that are NOT exact halves (the ceil- / floor-divided levels of a detection backbone): same kernel, masked cells
    "L4_ceil_divided": [(50, 83), (25, 42), (13, 21), (7, 11)],
    "L4_floor_divided": [(51, 83), (25, 41), (12, 20), (6, 10)],
    "L3_mixed_rounding": [(45, 70), (23, 35), (11, 18)],
}


@pytest.mark.parametrize("name", sorted(PYRAMIDS))
@pytest.mark.parametrize("mode", ["encoder_like", "mixed", "uniform"])
def test_generation6_pyramid_items(name, mode):
    """The pyramid-item kernels (one item = an 8 x 16 region of level 0 with the queries of every level): generation 9 (fp32, the
    automatic choice) and generation 6 (the bf16-value operator, exact 2x pyramids): partial tiles, 1-4 levels, windows that fit
    the arena (encoder_like), a mix of staged and global-memory levels (far offsets on a third of the points, rejected /
    non-finite points), and everything from global memory (uniform locations).  Equal to the gather kernel and to the oracle;
    two runs are bit-identical (race screen)."""
    from visionllm_amd import _lib
    shapes = PYRAMIDS[name]
    g = make_inputs(2, 8, 32, shapes, 4, mode="encoder_like", seed=len(shapes))
    rng = np.random.default_rng(7)
    if mode == "mixed":
        loc = g["loc"].copy()
        flat = loc.reshape(-1, 2)
        flat[1::3] += rng.standard_normal(flat[1::3].shape).astype(np.float32) * 0.15
        flat[3::29] = 1.7
        flat[5::97] = np.nan
        flat[6::101] = np.inf
        g["loc"] = loc
    elif mode == "uniform":
        g["loc"] = (rng.random(g["loc"].shape, dtype=np.float32) * 1.1 - 0.05).astype(np.float32)
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    old = _lib.set_option("msda_tiled", 0)
    try:
        plain = _run(g)
        _lib.set_option("msda_tiled", 1)    # automatic = generation 9
        t9, again = _run(g), _run(g)
    finally:
        _lib.set_option("msda_tiled", old)
    assert torch.equal(t9, again), "race: two runs of generation 9 differ"
    assert torch.isfinite(t9).all()
    torch.testing.assert_close(t9, plain, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(t9.cpu().numpy(), ref, rtol=4e-6, atol=4e-6)
    _check_bf16_route(g)


def test_generation6_bf16_value():
    """bf16 value / output (what the fused layer hands over): converted to fp32 while the windows are staged, so the
    result is the fp32 kernel's on the bf16-rounded value, rounded once to bf16."""
    from visionllm_amd import _lib
    shapes = PYRAMIDS["L4_partial_tiles"]
    g = make_inputs(2, 8, 32, shapes, 4, mode="encoder_like", seed=3)
    rng = np.random.default_rng(1)
    flat = g["loc"].reshape(-1, 2)
    flat[1::5] += rng.standard_normal(flat[1::5].shape).astype(np.float32) * 0.2   # some levels from global memory
    vb = torch.from_numpy(g["value"]).to(torch.bfloat16)
    ref = O.forward(vb.float().numpy(), g["shapes"], g["lsi"], g["loc"], g["attw"])
    outs = {}
    old = _lib.set_option("msda_tiled", 1)
    try:
        for mode in (1, 0):
            _lib.set_option("msda_tiled", mode)
            outs[mode] = A.ms_deform_attn_forward(vb.to(DEV), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"]), 64)
    finally:
        _lib.set_option("msda_tiled", old)
    for mode, o in outs.items():
        assert o.dtype == torch.bfloat16
        err = np.abs(o.float().cpu().numpy() - ref)
        assert (err <= 2.0 ** -8 * np.abs(ref) + 1e-6).all(), (mode, err.max())   # one rounding to bf16 (half an ulp = 2^-9 relative)


def test_generation6_output_is_written_exactly_once_everywhere():
    """Every (query, head) row of the output is produced by exactly one item: poison the output, run, no poison left
    (pyramid with partial tiles in both directions)."""
    shapes = [(76, 104), (38, 52), (19, 26)]
    g = make_inputs(1, 8, 32, shapes, 4, mode="encoder_like", seed=2)
    out = _run(g)
    assert torch.isfinite(out).all()
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=4e-6, atol=4e-6)


def test_nonfinite_values_outside_the_footprint_do_not_leak():
    g = make_inputs(1, 2, 32, [(4, 4)], 4, Lq=16, mode="stress", seed=9)
    loc = np.full_like(g["loc"], 0.999)  # bottom-right pixel: only corner 1 in bounds
    v = g["value"].copy()
    v[0, :15] = np.nan  # every other pixel is NaN; clamped addresses may touch them
    o = A.ms_deform_attn_forward(_t(v), _t(g["shapes"]), _t(g["lsi"]), _t(loc), _t(g["attw"]), 64)
    assert torch.isfinite(o).all()
    ref = O.forward(v, g["shapes"], g["lsi"], loc, g["attw"])
    np.testing.assert_allclose(o.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


def test_nan_and_inf_sampling_locations_contribute_nothing():
    """Reference: the acceptance test is false for NaN / +-inf coordinates, so such points are skipped."""
    from visionllm_amd import _lib
    g = make_inputs(1, 8, 32, [(72, 64), (36, 32)], 4, mode="encoder_like", seed=6)   # Lq = S >= 4096: tiled kernels too
    loc = g["loc"].copy()
    flat = loc.reshape(-1)
    flat[5::37] = np.nan
    flat[11::53] = np.inf
    flat[12::59] = -np.inf
    ref = O.forward(g["value"], g["shapes"], g["lsi"], loc, g["attw"])
    assert np.isfinite(ref).all()
    outs = []
    for tiled in (0, 1):
        old = _lib.set_option("msda_tiled", tiled)
        try:
            outs.append(A.ms_deform_attn_forward(_t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(loc), _t(g["attw"]), 64))
            if tiled == 1:
                outs.append(_run_general(dict(g, loc=loc)))   # generation 4
        finally:
            _lib.set_option("msda_tiled", old)
    for out in outs:
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)
    _check_bf16_route(dict(g, loc=loc))


def test_edge_cases_and_errors():
    shapes = torch.tensor([[2, 3]], device=DEV)
    lsi = torch.tensor([0], device=DEV)
    v = torch.zeros(1, 6, 2, 4, device=DEV)
    out = A.ms_deform_attn_forward(v, shapes, lsi, torch.zeros(1, 0, 2, 1, 2, 2, device=DEV),
                                   torch.zeros(1, 0, 2, 1, 2, device=DEV), 64)
    assert out.shape == (1, 0, 8)
    with pytest.raises(RuntimeError):  # not contiguous
        A.ms_deform_attn_forward(torch.zeros(1, 6, 4, 2, device=DEV).transpose(2, 3), shapes, lsi,
                                 torch.zeros(1, 1, 2, 1, 2, 2, device=DEV), torch.zeros(1, 1, 2, 1, 2, device=DEV), 64)
    with pytest.raises(RuntimeError):  # batch % im2col_step (ms_deform_attn_cuda.cu:50-52)
        A.ms_deform_attn_forward(torch.zeros(3, 6, 2, 4, device=DEV), shapes, lsi,
                                 torch.zeros(3, 1, 2, 1, 2, 2, device=DEV), torch.zeros(3, 1, 2, 1, 2, device=DEV), 2)
    with pytest.raises(RuntimeError):  # cpu tensor
        A.ms_deform_attn_forward(v.cpu(), shapes, lsi, torch.zeros(1, 1, 2, 1, 2, 2, device=DEV),
                                 torch.zeros(1, 1, 2, 1, 2, device=DEV), 64)


@pytest.mark.parametrize("Lq", [29, None])   # gather kernels / encoder shape (Lq == S: LDS-tiled kernels)
def test_empty_level_adds_nothing_and_touches_no_memory(Lq):
    """A level with H == 0 or W == 0: the reference accepts the point (h_im = -0.5 > -1, ms_deform_im2col_cuda.cuh:277-292)
    but every corner test fails, so the level contributes exactly zero and no address is formed.  (the
    clamped unconditional loads would have read index -1.)"""
    shapes = [(6, 8), (0, 5), (3, 4), (2, 0)]
    S = 48 + 12
    lq = S if Lq is None else Lq
    rng = np.random.default_rng(1)
    value = rng.standard_normal((2, S, 8, 32)).astype(np.float32)
    loc = (rng.random((2, lq, 8, 4, 4, 2)) * 1.1 - 0.05).astype(np.float32)
    attw = rng.random((2, lq, 8, 4, 4)).astype(np.float32)
    ss = np.array(shapes, dtype=np.int64)
    lsi = np.array([0, 48, 48, 60], dtype=np.int64)
    ref = O.forward(value.astype(np.float64), ss, lsi, loc.astype(np.float64), attw.astype(np.float64))
    out = A.ms_deform_attn_forward(_t(value), _t(ss), _t(lsi), _t(loc), _t(attw), 64)
    np.testing.assert_allclose(out.cpu().numpy(), ref.reshape(out.shape), rtol=1e-4, atol=1e-4)
    out64 = A.ms_deform_attn_forward(_t(value).double(), _t(ss), _t(lsi), _t(loc).double(), _t(attw).double(), 64)
    np.testing.assert_allclose(out64.cpu().numpy(), ref.reshape(out.shape), rtol=1e-12, atol=1e-12)
    # the two live levels alone give the same answer: the empty ones added nothing
    keep = [0, 2]
    ref2 = O.forward(value.astype(np.float64), ss[keep], np.array([0, 48]), loc[:, :, :, keep].astype(np.float64),
                     attw[:, :, :, keep].astype(np.float64))
    np.testing.assert_allclose(ref, ref2, rtol=0, atol=1e-12)
    go = rng.standard_normal((2, lq, 256)).astype(np.float32)
    gv, gl, gw = A.ms_deform_attn_backward(_t(value), _t(ss), _t(lsi), _t(loc), _t(attw), _t(go), 64)
    assert torch.isfinite(gv).all()
    assert (gl[:, :, :, [1, 3]] == 0).all() and (gw[:, :, :, [1, 3]] == 0).all()
    rv, rl, rw = O.backward(value.astype(np.float64), ss, lsi, loc.astype(np.float64), attw.astype(np.float64),
                            go.astype(np.float64))
    np.testing.assert_allclose(gv.cpu().numpy(), rv, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(gw.cpu().numpy(), rw, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("channels", [4, 30, 32, 64, 71, 1025])  # the reference's gradcheck list (:139-146)
def test_backward_vs_oracle_f64(channels):
    N, M, Lq, L, P = 1, 2, 2, 2, 2
    shapes = [(3, 2), (2, 1)]
    g = make_inputs(N, M, channels, shapes, P, Lq=Lq, mode="stress", seed=channels, dtype=np.float64)
    g["value"] *= 0.01
    rng = np.random.default_rng(1)
    go = rng.standard_normal((N, Lq, M * channels))
    gv, gl, gw = A.ms_deform_attn_backward(_t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]),
                                           _t(g["attw"]), _t(go), 2)
    rv, rl, rw = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], go)
    np.testing.assert_allclose(gv.cpu().numpy(), rv, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gl.cpu().numpy(), rl, rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(gw.cpu().numpy(), rw, rtol=1e-10, atol=1e-13)


def test_backward_f32_and_autograd_function():
    shapes = [(9, 7), (5, 4)]
    g = make_inputs(2, 4, 32, shapes, 4, Lq=50, mode="stress", seed=2)
    v = _t(g["value"]).requires_grad_(True)
    loc = _t(g["loc"]).requires_grad_(True)
    w = _t(g["attw"]).requires_grad_(True)
    out = A.MSDeformAttnFunction.apply(v, _t(g["shapes"]), _t(g["lsi"]), loc, w, 64)
    go = torch.randn_like(out)
    out.backward(go)
    rv, rl, rw = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], go.cpu().numpy())
    np.testing.assert_allclose(v.grad.cpu().numpy(), rv, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(loc.grad.cpu().numpy(), rl, rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(w.grad.cpu().numpy(), rw, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("D,M,P", [(32, 8, 4), (64, 2, 8), (16, 4, 2), (4, 3, 1), (128, 1, 4)])
def test_backward_f32_vectorised_vs_oracle(D, M, P):
    """fp32 backward through the vectorised kernel (D/4 a power of two) incl. rejected / border points."""
    shapes = [(13, 11), (7, 6), (4, 3)]
    g = make_inputs(2, M, D, shapes, P, Lq=77, mode="stress", seed=D + P)
    rng = np.random.default_rng(3)
    go = rng.standard_normal((2, 77, M * D)).astype(np.float32)
    gv, gl, gw = A.ms_deform_attn_backward(_t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"]),
                                           _t(go), 64)
    rv, rl, rw = O.backward(g["value"].astype(np.float64), g["shapes"], g["lsi"], g["loc"].astype(np.float64),
                            g["attw"].astype(np.float64), go.astype(np.float64))
    # d/dloc is discontinuous at exact pixel borders, which the stress fixture contains (0.0 / 0.5 / 1.0): the fp32 and
    # fp64 evaluations may pick different sides there -> the fp64 oracle is the reference away from those points only
    sel = np.ones(g["loc"].shape[:-1], dtype=bool)
    for l, (H, W) in enumerate(shapes):
        fy = g["loc"][:, :, :, l, :, 1].astype(np.float64) * H - 0.5
        fx = g["loc"][:, :, :, l, :, 0].astype(np.float64) * W - 0.5
        sel[:, :, :, l] &= ~((np.abs(fy - np.round(fy)) < 1e-4) | (np.abs(fx - np.round(fx)) < 1e-4))
    np.testing.assert_allclose(gw.cpu().numpy()[sel], rw[sel], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(gl.cpu().numpy()[sel], rl[sel], rtol=2e-3, atol=2e-3)
    # the border points: against the one-sided derivative of the cell the index-exact contract puts them in (lattice_inputs.py), at
    # the same bounds -- no point is skipped
    fl, fw, _ = LI.fixed_cell_point_gradients(g["value"], shapes, g["lsi"], g["loc"], g["attw"], go, ~sel)
    assert (~sel).sum() > 0
    np.testing.assert_allclose(gw.cpu().numpy()[~sel], fw[~sel], **LI.GW_TOL)
    np.testing.assert_allclose(gl.cpu().numpy()[~sel], fl[~sel], **LI.GL_TOL)
    # grad_value: PER ELEMENT against the fp32 oracle (same integer parts by the index-exact contract, so no border flips):
    # only the order of the fp32 sums differs -> 2^-18 of the summed |terms| (oracle on |grad_out|; the weights are >= 0)
    rv32, _, _ = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], go)
    mag, _, _ = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], np.abs(g["attw"]), np.abs(go))
    assert (np.abs(gv.cpu().numpy() - rv32) <= 2.0 ** -18 * mag + 1e-7).all()
    assert np.abs(rv32 - rv).max() <= 1e-3 * (1 + np.abs(rv).max())   # (fp32 oracle vs fp64 oracle: sanity)


@pytest.mark.parametrize("case", ["mfma_encoder_shape", "forced_fallback", "decoder_shape", "misaligned_grad_loc"])
def test_backward_allocating_flavour_never_returns_uninitialised_gradients(case, monkeypatch):
    """ms_deform_attn_backward allocates grad_sampling_loc / grad_attn_weight UNINITIALISED when
    vllm_msda_backward_f32_writes_point_grads says the kernel will write every element, and zero-fills them otherwise.  The query and
    the dispatch inside vllm_msda_backward_f32 must agree: here torch.empty_like hands out NaN-poisoned buffers and the result must be
    finite and EQUAL to the in-place flavour run on zero-filled buffers -- on the matrix-core path (encoder shape), with the LDS-tiled
    kernels switched off, with Lq != S, and with a grad_sampling_loc the vector path must refuse (the query sees the caller's pointer)."""
    from visionllm_amd import _lib
    shapes = [(40, 36), (20, 18), (10, 9), (5, 5)]
    Lq = None if case != "decoder_shape" else 300
    g = make_inputs(2, 8, 32, shapes, 4, Lq=Lq, mode="stress", seed=11)
    t = {k: _t(v) for k, v in g.items()}
    go = torch.randn(t["loc"].shape[0], t["loc"].shape[1], 8 * 32, device=DEV)
    real_empty_like = torch.empty_like

    def poisoned(x, *a, **k):
        r = real_empty_like(x, *a, **k)
        if r.is_floating_point():
            r.fill_(float("nan"))
        if case == "misaligned_grad_loc" and r.shape == t["loc"].shape:
            big = torch.full((x.numel() + 1,), float("nan"), dtype=x.dtype, device=x.device)
            r = big[1:].view(x.shape)          # 4 bytes off a 16-byte boundary
        return r
    old = _lib.set_option("msda_tiled", 0) if case == "forced_fallback" else None
    try:
        monkeypatch.setattr(A.torch, "empty_like", poisoned)
        gv, gl, gw = A.ms_deform_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["attw"], go, 64)
        monkeypatch.setattr(A.torch, "empty_like", real_empty_like)
        rv, rl, rw = torch.zeros_like(t["value"]), torch.zeros_like(t["loc"]), torch.zeros_like(t["attw"])
        A.ms_deform_attn_backward_(t["value"], t["shapes"], t["lsi"], t["loc"], t["attw"], go, rv, rl, rw, 64)
    finally:
        if old is not None:
            _lib.set_option("msda_tiled", old)
    assert torch.isfinite(gl).all() and torch.isfinite(gw).all() and torch.isfinite(gv).all()
    # (grad_value is accumulated with atomics: order-dependent in the last bits; the per-point gradients are written once)
    torch.testing.assert_close(gl, rl, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gw, rw, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gv, rv, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("spread", ["near", "medium", "far"])
@pytest.mark.parametrize("shapes,B,M", [([(72, 64), (36, 32), (18, 16), (9, 8)], 2, 8), ([(65, 67), (33, 34)], 1, 3)])
def test_backward_f32_encoder_shape_tiled_vs_plain_vs_oracle(shapes, B, M, spread):
    """Encoder self-attention shape (Lq = S >= 4096, D 32, P 4): the windowed backward (msda_bwd_mfma.hip: the value window
    staged in LDS, grad_value as S^T x grad_out on the matrix cores) -- windows of one round (near), of several 128-pixel rounds
    and beyond the staging limit (medium), and the global-atomic fallback for windows over 1024 pixels (far) --, rejected /
    non-finite points, and the plain atomic kernel agree with the oracle."""
    from visionllm_amd import _lib
    g = make_inputs(B, M, 32, shapes, 4, mode="encoder_like", seed=len(shapes) + M)
    loc = g["loc"].copy()
    flat = loc.reshape(-1, 2)
    if spread == "far":
        flat[7::41] += 0.37        # far offsets: some (tile, level) windows exceed 1024 pixels -> global-atomic fallback
    elif spread == "medium":
        rng0 = np.random.default_rng(5)
        flat[2::3] += (rng0.standard_normal(flat[2::3].shape) * 0.06).astype(np.float32)   # windows of a few hundred pixels
    flat[3::29] = 1.7              # rejected points
    flat[5::97] = np.nan
    Lq = loc.shape[1]
    rng = np.random.default_rng(11)
    go = rng.standard_normal((B, Lq, M * 32)).astype(np.float32)
    rv, rl, rw = O.backward(g["value"].astype(np.float64), g["shapes"], g["lsi"], loc.astype(np.float64),
                            g["attw"].astype(np.float64), go.astype(np.float64))
    rv32, _, _ = O.backward(g["value"], g["shapes"], g["lsi"], loc, g["attw"], go)                    # fp32 oracle
    mag, _, _ = O.backward(g["value"], g["shapes"], g["lsi"], loc, np.abs(g["attw"]), np.abs(go))     # sum of |terms|
    sel = np.isfinite(loc).all(-1)
    for l, (H, W) in enumerate(shapes):   # d/dloc is discontinuous at exact pixel borders (see the vectorised test)
        fy = np.nan_to_num(loc[:, :, :, l, :, 1].astype(np.float64)) * H - 0.5
        fx = np.nan_to_num(loc[:, :, :, l, :, 0].astype(np.float64)) * W - 0.5
        sel[:, :, :, l] &= ~((np.abs(fy - np.round(fy)) < 1e-4) | (np.abs(fx - np.round(fx)) < 1e-4))
    # the finite points within 1e-4 px of a border: the fixed-cell reference (lattice_inputs.py) at the same bounds; the non-finite
    # ones: exact zeros -- no point is skipped
    finite = np.isfinite(loc).all(-1)
    drop = finite & ~sel
    fl, fw, _ = LI.fixed_cell_point_gradients(g["value"], shapes, g["lsi"], loc, g["attw"], go, drop)
    old = _lib.set_option("msda_tiled", 1)
    try:
        res = {}
        for mode in (1, 0):   # 1: LDS-tiled backward, 0: plain atomic kernel
            _lib.set_option("msda_tiled", mode)
            gv, gl, gw = A.ms_deform_attn_backward(_t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(loc), _t(g["attw"]),
                                                   _t(go), 64)
            res[mode] = (gv.cpu().numpy(), gl.cpu().numpy(), gw.cpu().numpy())
            assert np.isfinite(res[mode][0]).all() and np.isfinite(res[mode][1]).all() and np.isfinite(res[mode][2]).all()
            np.testing.assert_allclose(res[mode][2][sel], rw[sel], rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(res[mode][1][sel], rl[sel], rtol=2e-3, atol=2e-3)
            np.testing.assert_allclose(res[mode][2][drop], fw[drop], **LI.GW_TOL)
            np.testing.assert_allclose(res[mode][1][drop], fl[drop], **LI.GL_TOL)
            assert (res[mode][1][~finite] == 0).all() and (res[mode][2][~finite] == 0).all()
            assert (np.abs(res[mode][0] - rv32) <= 2.0 ** -18 * mag + 1e-7).all(), mode   # per element vs the fp32 oracle
        # the windowed kernel sums over the channels first (four dot products per point, then the bilinear weights), the plain one
        # weights per channel and sums then: the per-point gradients agree to fp32 rounding of sums of ~32 terms, grad_value differs
        # only by the order of its sums
        for i in (1, 2):
            scale = np.abs(res[0][i]).max() + 1e-12
            np.testing.assert_allclose(res[1][i], res[0][i], rtol=1e-4, atol=2e-6 * scale)
        np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-4, atol=1e-4)
    finally:
        _lib.set_option("msda_tiled", old)


# ---- the three module mirrors vs the reference's OWN module classes (fixtures: oracle/gen_golden.py::gen_msda_layer) ----
def _load_layer(g, prefix, mod):
    sd = {k[len(prefix) + 4:]: torch.from_numpy(g[k]) for k in list(g.keys()) if k.startswith(prefix + ".sd.")}
    mod.load_state_dict(sd, strict=True)
    return mod.to(DEV).eval()


def _bf16_vs_reference_arithmetic(fused, composed, ref64, what):
    """bf16 modules against the reference module's fp64 output (fixture).  The yardstick is the REFERENCE'S OWN bf16
    arithmetic -- torch bf16 linears / softmax / location math around the fp32 operator, which is what the reference module
    computes in bf16 and what our mirror's composed path runs (`composed`, taken under enable_grad so that the fused layer is
    bypassed): the fused native layer keeps every internal tensor in fp32 and must not be further from the truth than that,
    in RMS (x 1.05) and in the worst element (x 2: two different roundings of the same quantity)."""
    ref = torch.from_numpy(ref64).double()
    ef, ec = (fused.double().cpu() - ref).abs(), (composed.double().cpu() - ref).abs()
    rms_f, rms_c = float((ef ** 2).mean().sqrt()), float((ec ** 2).mean().sqrt())
    assert rms_f <= 1.05 * rms_c, (what, rms_f, rms_c)
    assert float(ef.max()) <= 2.0 * float(ec.max()), (what, float(ef.max()), float(ec.max()))


@pytest.mark.parametrize("tag", ["unipose_ref2", "unipose_ref4", "unipose_ref4_norm"])
def test_unipose_module_vs_reference_module(tag):
    g = load_golden("msda_layer.npz")
    M, L, P = int(g["n_heads"]), int(g["n_levels"]), int(g["n_points"])
    C = g[f"{tag}.query"].shape[-1]
    mod = _load_layer(g, tag, A.MSDeformAttn(d_model=C, n_levels=L, n_heads=M, n_points=P, use_4D_normalizer=bool(g[f"{tag}.use4d"])))
    args = (_t(g[f"{tag}.query"]), _t(g[f"{tag}.ref"]), _t(g[f"{tag}.src"]), _t(g["shapes"]), _t(g["lsi"]), _t(g[f"{tag}.mask"]))
    with torch.no_grad():
        out = mod(*args)                                        # fp32: torch linears around the native operator
        np.testing.assert_allclose(out.cpu().numpy(), g[f"{tag}.out_f32"], rtol=2e-5, atol=2e-5)
        mb = mod.to(torch.bfloat16)                             # bf16: the fused native layer (one C call)
        ob = mb(args[0].bfloat16(), args[1], args[2].bfloat16(), *args[3:])
    with torch.enable_grad():                                   # trainable parameters -> composed path (torch bf16 linears)
        oc = mb(args[0].bfloat16(), args[1], args[2].bfloat16(), *args[3:]).detach()
    assert ob.dtype == torch.bfloat16
    _bf16_vs_reference_arithmetic(ob, oc, g[f"{tag}.out_f64"], tag)


def test_key_aware_signature_variant():
    """unipose/ops/modules/ms_deform_attn_key_aware.py:83: ``forward(query, key, reference_points, ...)`` -- the reference's forward never
    reads ``key``; the variant must give the plain module's result bit for bit on the reference-run fixture."""
    g = load_golden("msda_layer.npz")
    tag = "unipose_ref2"
    M, L, P = int(g["n_heads"]), int(g["n_levels"]), int(g["n_points"])
    C = g[f"{tag}.query"].shape[-1]
    plain = _load_layer(g, tag, A.MSDeformAttn(d_model=C, n_levels=L, n_heads=M, n_points=P))
    aware = _load_layer(g, tag, A.MSDeformAttnKeyAware(d_model=C, n_levels=L, n_heads=M, n_points=P))
    q, ref, src = _t(g[f"{tag}.query"]), _t(g[f"{tag}.ref"]), _t(g[f"{tag}.src"])
    rest = (_t(g["shapes"]), _t(g["lsi"]), _t(g[f"{tag}.mask"]))
    key = torch.randn(q.shape[0], 1, C, device=DEV)
    with torch.no_grad():
        a, b = plain(q, ref, src, *rest), aware(q, key, ref, src, *rest)
        np.testing.assert_allclose(b.cpu().numpy(), g[f"{tag}.out_f32"], rtol=2e-5, atol=2e-5)
    assert torch.equal(a, b)


@pytest.mark.parametrize("tag", ["mmcv_ref2", "mmcv_ref4"])
def test_mmcv_module_vs_reference_module(tag):
    g = load_golden("msda_layer.npz")
    M, L, P = int(g["n_heads"]), int(g["n_levels"]), int(g["n_points"])
    C = g[f"{tag}.query"].shape[-1]
    mod = _load_layer(g, tag, A.MultiScaleDeformableAttention(embed_dims=C, num_heads=M, num_levels=L, num_points=P, dropout=0.1))
    q, src, pos = (_t(g[f"{tag}.{n}"]).transpose(0, 1) for n in ("query", "src", "query_pos"))
    kw = dict(key_padding_mask=_t(g[f"{tag}.mask"]), reference_points=_t(g[f"{tag}.ref"]), spatial_shapes=_t(g["shapes"]),
              level_start_index=_t(g["lsi"]))
    with torch.no_grad():
        out = mod(q, value=src, query_pos=pos, **kw)
        np.testing.assert_allclose(out.cpu().numpy(), g[f"{tag}.out_f32"], rtol=2e-5, atol=2e-5)
        ob = mod.to(torch.bfloat16)(q.bfloat16(), value=src.bfloat16(), query_pos=pos.bfloat16(), **kw)
    with torch.enable_grad():
        oc = mod(q.bfloat16(), value=src.bfloat16(), query_pos=pos.bfloat16(), **kw).detach()
    _bf16_vs_reference_arithmetic(ob, oc, g[f"{tag}.out_f64"], tag)


@pytest.mark.parametrize("tag", ["gdino_ref2", "gdino_ref4"])
def test_grounding_dino_module_vs_reference_module(tag):
    import types
    g = load_golden("msda_layer.npz")
    M, L, P = int(g["n_heads"]), int(g["n_levels"]), int(g["n_points"])
    C = g[f"{tag}.query"].shape[-1]
    cfg = types.SimpleNamespace(d_model=C, num_feature_levels=L, disable_custom_kernels=False)
    mod = _load_layer(g, tag, A.GroundingDinoMultiscaleDeformableAttention(cfg, num_heads=M, n_points=P))
    kw = dict(attention_mask=~_t(g[f"{tag}.mask"]), reference_points=_t(g[f"{tag}.ref"]), spatial_shapes=_t(g["shapes"]),
              level_start_index=_t(g["lsi"]))
    with torch.no_grad():
        out, aw = mod(_t(g[f"{tag}.query"]), encoder_hidden_states=_t(g[f"{tag}.src"]), position_embeddings=_t(g[f"{tag}.pos"]), **kw)
        np.testing.assert_allclose(out.cpu().numpy(), g[f"{tag}.out_f32"], rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(aw.cpu().numpy(), g[f"{tag}.attw_f32"], rtol=2e-5, atol=2e-6)
        ob, _ = mod.to(torch.bfloat16)(_t(g[f"{tag}.query"]).bfloat16(), encoder_hidden_states=_t(g[f"{tag}.src"]).bfloat16(),
                                       position_embeddings=_t(g[f"{tag}.pos"]).bfloat16(), **kw)
    with torch.enable_grad():
        oc, _ = mod(_t(g[f"{tag}.query"]).bfloat16(), encoder_hidden_states=_t(g[f"{tag}.src"]).bfloat16(),
                    position_embeddings=_t(g[f"{tag}.pos"]).bfloat16(), **kw)
    _bf16_vs_reference_arithmetic(ob, oc.detach(), g[f"{tag}.out_f64"], tag)


def test_compat_shims_module_name_and_mmcv_ext():
    """B3: ``import MultiScaleDeformableAttention as MSDA`` (unipose/ops/functions/ms_deform_attn_func.py:18; list-returning
    backward, ms_deform_attn.h:41-61) and the ``mmcv._ext`` alias (in-place backward, mmcv csrc ms_deform_attn.cpp:48-60),
    called the way the reference's autograd Functions call them."""
    import importlib
    import os
    import sys
    import types
    import visionllm_amd
    compat = os.path.join(os.path.dirname(visionllm_amd.__file__), "compat")
    g = load_golden("msda_stress_d32.npz")
    t = [_t(g[k]) for k in ("value", "shapes", "lsi", "loc", "attw")]
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    go = torch.randn(ref.shape, device=DEV)
    rv, rl, rw = O.backward(g["value"].astype(np.float64), g["shapes"], g["lsi"], g["loc"].astype(np.float64),
                            g["attw"].astype(np.float64), go.cpu().numpy().astype(np.float64))
    sys.path.insert(0, compat)
    try:
        MSDA = importlib.import_module("MultiScaleDeformableAttention")
        out = MSDA.ms_deform_attn_forward(*t, 64)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)
        gv, gl, gw = MSDA.ms_deform_attn_backward(*t, go, 64)
        np.testing.assert_allclose(gw.cpu().numpy(), rw, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(gv.cpu().numpy(), rv, rtol=1e-3, atol=1e-3)
    finally:
        sys.path.remove(compat)
        sys.modules.pop("MultiScaleDeformableAttention", None)
    had = {k: sys.modules.get(k) for k in ("mmcv", "mmcv._ext")}
    try:
        sys.modules.setdefault("mmcv", types.ModuleType("mmcv"))
        from visionllm_amd.compat import mmcv_ext
        mmcv_ext.install(force=True)
        ext = importlib.import_module("mmcv." + "_ext")           # == mmcv.utils.ext_loader.load_ext('_ext', [...])
        for fun in ("ms_deform_attn_backward", "ms_deform_attn_forward"):
            assert hasattr(ext, fun), f"{fun} miss in module _ext"
        out = ext.ms_deform_attn_forward(*t, im2col_step=64)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)
        gv, gl, gw = torch.zeros_like(t[0]), torch.zeros_like(t[3]), torch.zeros_like(t[4])
        ext.ms_deform_attn_backward(*t, go.contiguous(), gv, gl, gw, im2col_step=64)
        np.testing.assert_allclose(gw.cpu().numpy(), rw, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(gv.cpu().numpy(), rv, rtol=1e-3, atol=1e-3)
    finally:
        for k, v in had.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_modules_match_oracle_composition():
    """MSDeformAttn / mmcv module / GDINO module == (torch Linear layers + oracle op) on the same weights."""
    torch.manual_seed(0)
    shapes = [(8, 6), (4, 3)]
    S = 48 + 12
    mod = A.MSDeformAttn(d_model=64, n_levels=2, n_heads=4, n_points=4).to(DEV)
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.05)
        mod.attention_weights.weight.normal_(0, 0.5)
    q = torch.randn(2, 20, 64, device=DEV)
    src = torch.randn(2, S, 64, device=DEV)
    ref_pts = torch.rand(2, 20, 2, 2, device=DEV)
    ss = torch.tensor(shapes, device=DEV)
    lsi = torch.tensor([0, 48], device=DEV)
    mask = torch.zeros(2, S, dtype=torch.bool, device=DEV)
    mask[1, -5:] = True
    out = mod(q, ref_pts, src, ss, lsi, mask)
    with torch.no_grad():
        value = mod.value_proj(src).masked_fill(mask[..., None], 0.0).view(2, S, 4, 16)
        off = mod.sampling_offsets(q).view(2, 20, 4, 2, 4, 2)
        aw = torch.softmax(mod.attention_weights(q).view(2, 20, 4, 8), -1).view(2, 20, 4, 2, 4)
        norm = torch.stack([ss[..., 1], ss[..., 0]], -1)
        locs = ref_pts[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]
        core = O.forward(value.cpu().numpy(), ss.cpu().numpy(), lsi.cpu().numpy(), locs.cpu().numpy(), aw.cpu().numpy())
        expect = mod.output_proj(torch.from_numpy(core).to(DEV))
    torch.testing.assert_close(out, expect, rtol=1e-4, atol=1e-4)
    # mmcv module: (num_query, bs, C) layout, identity residual, dropout 0
    mm = A.MultiScaleDeformableAttention(embed_dims=64, num_heads=4, num_levels=2, num_points=4, dropout=0.0).to(DEV)
    mm.load_state_dict(mod.state_dict())
    o2 = mm(q.permute(1, 0, 2), value=src.permute(1, 0, 2), key_padding_mask=mask, reference_points=ref_pts,
            spatial_shapes=ss, level_start_index=lsi)
    torch.testing.assert_close(o2.permute(1, 0, 2), expect + q, rtol=1e-4, atol=1e-4)
    # the fork-added class (mmcv/ops/multi_scale_deform_attn_optimized.py:160): same parameters, same forward, the operator in value's
    # own dtype -- fp32: the same bits as the class above; fp64 runs in fp64 (the base class would compute it in fp64 too: mmcv's
    # cast is to fp32 only for lower precisions); gradients flow through the list-returning backward
    mo = A.MultiScaleDeformableAttentionOptimized(embed_dims=64, num_heads=4, num_levels=2, num_points=4, dropout=0.0).to(DEV)
    mo.load_state_dict(mm.state_dict(), strict=True)
    o2o = mo(q.permute(1, 0, 2), value=src.permute(1, 0, 2), key_padding_mask=mask, reference_points=ref_pts,
             spatial_shapes=ss, level_start_index=lsi)
    assert torch.equal(o2o, o2)
    qg = q.detach().clone().requires_grad_(True)
    mo(qg.permute(1, 0, 2), value=src.permute(1, 0, 2), key_padding_mask=mask, reference_points=ref_pts, spatial_shapes=ss,
       level_start_index=lsi).square().sum().backward()
    qh = q.detach().clone().requires_grad_(True)
    mm(qh.permute(1, 0, 2), value=src.permute(1, 0, 2), key_padding_mask=mask, reference_points=ref_pts, spatial_shapes=ss,
       level_start_index=lsi).square().sum().backward()
    torch.testing.assert_close(qg.grad, qh.grad, rtol=1e-4, atol=1e-5)
    mo64 = mo.double()
    o64 = mo64(q.double().permute(1, 0, 2), value=src.double().permute(1, 0, 2), key_padding_mask=mask, reference_points=ref_pts.double(),
               spatial_shapes=ss, level_start_index=lsi)
    assert o64.dtype == torch.float64
    torch.testing.assert_close(o64.float(), o2, rtol=1e-4, atol=1e-4)

    class Cfg:
        d_model, num_feature_levels, disable_custom_kernels = 64, 2, False
    gd = A.GroundingDinoMultiscaleDeformableAttention(Cfg(), 4, 4).to(DEV)
    gd.load_state_dict(mod.state_dict())
    o3, aw3 = gd(q, attention_mask=~mask, encoder_hidden_states=src, reference_points=ref_pts, spatial_shapes=ss,
                 level_start_index=lsi)
    torch.testing.assert_close(o3, expect, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(aw3, aw, rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# a13 / f2: the fused layer (vllm_msda_layer_forward) and its building blocks
# ---------------------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(torch.bfloat16)


def test_gemm_f32_epilogue_with_row_mask():
    import ctypes
    from visionllm_amd import _lib
    torch.manual_seed(0)
    Mr, N, K = 777, 160, 256
    x, w, b = _bf(torch.randn(Mr, K, device=DEV)), _bf(torch.randn(N, K, device=DEV) * 0.1), _bf(torch.randn(N, device=DEV))
    mask = (torch.rand(Mr, device=DEV) < 0.2).to(torch.uint8)
    y = torch.full((Mr, N), float("nan"), device=DEV)
    for m in (None, mask):
        _lib.check(_lib.lib().vllm_gemm_bf16(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), Mr, N, K, K, K, N,
                                             _lib.EPI_F32, None, _lib.ptr(m), 0, 0, _lib.current_stream()), "gemm f32")
        ref = x.double() @ w.double().T + b.double()
        if m is not None:
            ref = ref * (1 - m.double())[:, None]
        torch.testing.assert_close(y.double(), ref, rtol=2e-5, atol=2e-4)   # fp32 accumulation of exact bf16 products


@pytest.mark.parametrize("L,P,ref_dim,four_d", [(4, 4, 2, 0), (4, 4, 4, 0), (4, 4, 4, 1), (2, 4, 2, 0), (3, 4, 2, 0),
                                               (4, 8, 4, 0), (5, 3, 4, 1), (1, 4, 2, 0)])
def test_prep_kernel_softmax_and_locations(L, P, ref_dim, four_d):
    from visionllm_amd import _lib
    torch.manual_seed(L * 10 + P)
    R, M = 301, 8
    off = torch.randn(R, M, L, P, 2, device=DEV) * 3
    lg = torch.randn(R, M, L * P, device=DEV) * 4
    ref = torch.rand(R, L, ref_dim, device=DEV)
    shapes = torch.tensor([(7 + 3 * l, 5 + 2 * l) for l in range(L)], device=DEV)
    o, g = off.clone(), lg.clone()
    _lib.check(_lib.lib().vllm_msda_prep_f32(_lib.ptr(o), _lib.ptr(g), _lib.ptr(ref), _lib.ptr(shapes), R, M, L, P, ref_dim,
                                             four_d, _lib.current_stream()), "prep")
    aw = torch.softmax(lg.double(), -1)
    norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
    if ref_dim == 2:
        loc = ref.double()[:, None, :, None, :] + off.double() / norm[None, None, :, None, :]
    elif four_d:
        loc = ref.double()[:, None, :, None, :2] + off.double() / norm[None, None, :, None, :] * \
            ref.double()[:, None, :, None, 2:] * 0.5
    else:
        loc = ref.double()[:, None, :, None, :2] + off.double() / P * ref.double()[:, None, :, None, 2:] * 0.5
    torch.testing.assert_close(g.double(), aw, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(o.double(), loc, rtol=1e-5, atol=1e-6)


def test_f32_to_bf16_is_round_to_nearest_even():
    from visionllm_amd import _lib
    torch.manual_seed(0)
    for n in (1, 3, 4, 1027, 1 << 16):
        x = torch.randn(n, device=DEV) * 100
        x[::7] = 1.00390625   # ties
        y = torch.empty(n, dtype=torch.bfloat16, device=DEV)
        _lib.check(_lib.lib().vllm_f32_to_bf16(_lib.ptr(x), _lib.ptr(y), n, _lib.current_stream()), "cvt")
        assert torch.equal(y, x.to(torch.bfloat16))


def _layer_case(B, shapes, Lq, ref_dim, four_d, seed, M=8, P=4, C=256, masked=True):
    torch.manual_seed(seed)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    mod = A.MSDeformAttn(d_model=C, n_levels=L, n_heads=M, n_points=P, use_4D_normalizer=bool(four_d))
    with torch.no_grad():
        mod.sampling_offsets.weight.normal_(0, 0.02)
        mod.attention_weights.weight.normal_(0, 0.1)
        mod.attention_weights.bias.normal_(0, 0.5)
        mod.value_proj.bias.normal_(0, 0.1)
        mod.output_proj.bias.normal_(0, 0.1)
    mod = mod.to(DEV).to(torch.bfloat16).eval()
    Lq = S if Lq is None else Lq
    q = _bf(torch.randn(B, Lq, C, device=DEV))
    src = _bf(torch.randn(B, S, C, device=DEV))
    ref = torch.rand(B, Lq, L, ref_dim, device=DEV)
    if ref_dim == 4:
        ref[..., 2:] = ref[..., 2:] * 0.3 + 0.05
    ss = torch.tensor(shapes, device=DEV)
    lsi = torch.from_numpy(O.level_start_index(shapes)).to(DEV)
    mask = None
    if masked:
        mask = torch.zeros(B, S, dtype=torch.bool, device=DEV)
        mask[-1, -S // 7:] = True
    return mod, q, ref, src, ss, lsi, mask


def _layer_truth(mod, q, ref, src, ss, lsi, mask):
    """fp64 oracle on the module's (bf16-valued) parameters and inputs, and the reference's own arithmetic in bf16
    (bf16 linears / softmax / location math as the bf16 module would run them, fp32 operator: ms_deform_attn.py:131-139)."""
    params = {n: (getattr(mod, n).weight.detach().double().cpu().numpy(), getattr(mod, n).bias.detach().double().cpu().numpy())
              for n in ("value_proj", "sampling_offsets", "attention_weights", "output_proj")}
    m = None if mask is None else mask.cpu().numpy()
    truth, loc, aw = O.layer_forward(q.double().cpu().numpy(), ref.double().cpu().numpy(), src.double().cpu().numpy(),
                                     ss.cpu().numpy(), lsi.cpu().numpy(), m, params, mod.n_heads, mod.n_levels,
                                     mod.n_points, mod.use_4D_normalizer)
    cm = mod.cpu()
    with torch.no_grad():
        qc, sc, rc = q.cpu(), src.cpu(), ref.cpu().to(torch.bfloat16)
        B, Lq, C = qc.shape
        S = sc.shape[1]
        v = cm.value_proj(sc)
        if mask is not None:
            v = v.masked_fill(mask.cpu()[..., None], 0.0)
        off = cm.sampling_offsets(qc).view(B, Lq, cm.n_heads, cm.n_levels, cm.n_points, 2)
        awb = F.softmax(cm.attention_weights(qc).view(B, Lq, cm.n_heads, -1), -1).view(B, Lq, cm.n_heads, cm.n_levels,
                                                                                      cm.n_points)
        locb = A._sampling_locations(rc, off, ss.cpu(), cm.n_points, cm.use_4D_normalizer)
        core = O.forward(v.view(B, S, cm.n_heads, -1).float().numpy(), ss.cpu().numpy(), lsi.cpu().numpy(),
                         locb.float().numpy(), awb.float().numpy())
        ref_bf16 = cm.output_proj(torch.from_numpy(core).to(torch.bfloat16)).double().numpy()
    mod.to(DEV)
    return truth, ref_bf16


import torch.nn.functional as F  # noqa: E402


@pytest.mark.parametrize("shapes,Lq,ref_dim,four_d", [
    ([(12, 16), (6, 8), (3, 4)], 50, 2, 0),          # decoder-like: few queries, gather kernel
    ([(12, 16), (6, 8), (3, 4)], 37, 4, 0),          # 4-d reference points (boxes)
    ([(12, 16), (6, 8)], 64, 4, 1),                  # UniPose 4D normalizer
    ([(72, 64), (36, 32), (18, 16), (9, 8)], None, 2, 0),   # encoder self-attention: Lq == S -> LDS-tiled operator
])
def test_fused_layer_vs_oracle(shapes, Lq, ref_dim, four_d):
    mod, q, ref, src, ss, lsi, mask = _layer_case(2, shapes, Lq, ref_dim, four_d, seed=len(shapes) * 7 + ref_dim)
    with torch.no_grad():
        assert A.msda_layer_fused_ok(q, src, mod.value_proj, mod.sampling_offsets, mod.attention_weights, mod.output_proj)
        out = mod(q, ref, src, ss, lsi, mask)
        again = mod(q, ref, src, ss, lsi, mask)
    assert out.dtype == torch.bfloat16 and torch.equal(out, again)
    truth, ref_bf16 = _layer_truth(mod, q, ref, src, ss, lsi, mask)
    o = out.double().cpu().numpy()
    rms = np.sqrt((truth ** 2).mean())
    err = np.sqrt(((o - truth) ** 2).mean()) / rms
    err_ref = np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms
    # internal tensors are fp32, so we must be at least as close to the fp64 truth as the reference's bf16 arithmetic
    assert err <= max(err_ref * 1.05, 4e-3), (err, err_ref)
    assert np.abs(o - truth).max() <= 2e-2 * np.abs(truth).max()


def test_fused_layer_cfg4_batch8_vs_oracle_every_image():
    """The fused layer at the shape bench.py TIMES it (BASELINE configs[3]: 168^2 / 84^2 / 42^2 / 21^2, B = 8, Lq = S = 37 485,
    d_model 256, 8 heads): EPI_MSDA query GEMM at M = 299 880, bf16 operator output, 1200-pixel arena with late levels.
    fp64 oracle per image on the CPU; every image is compared on its own."""
    mod, q, ref, src, ss, lsi, mask = _layer_case(8, CFG4_SHAPES, None, 2, 0, seed=404)
    with torch.no_grad():
        out = mod(q, ref, src, ss, lsi, mask)
        again = mod(q, ref, src, ss, lsi, mask)
    assert torch.equal(out, again)
    for b in range(8):
        sl = slice(b, b + 1)
        mb = None if mask is None else mask[sl]
        truth, ref_bf16 = _layer_truth(mod, q[sl], ref[sl], src[sl], ss, lsi, mb)
        o = out[sl].double().cpu().numpy()
        rms = np.sqrt((truth ** 2).mean())
        err = np.sqrt(((o - truth) ** 2).mean()) / rms
        err_ref = np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms
        assert err <= max(err_ref * 1.05, 4e-3), (b, err, err_ref)
        assert np.abs(o - truth).max() <= 2e-2 * np.abs(truth).max(), b


@pytest.mark.parametrize("shapes,Lq,ref_dim,four_d,M", [
    ([(20, 24), (10, 12), (5, 6), (3, 3)], 77, 2, 0, 8),       # L * P == 16: query GEMM with the sampling epilogue
    ([(20, 24), (10, 12), (5, 6), (3, 3)], 130, 4, 0, 8),      # boxes
    ([(20, 24), (10, 12), (5, 6), (3, 3)], 61, 4, 1, 4),       # UniPose 4D normalizer, 4 heads (N = 192)
    ([(40, 48), (20, 24), (10, 12), (5, 6)], None, 2, 0, 8),   # pyramid + Lq == S: operator writes bf16 itself
    ([(41, 48), (20, 24), (10, 12), (5, 6)], None, 2, 0, 8),   # not a pyramid: fp32 operator + conversion pass
])
def test_fused_layer_sampling_epilogue_matches_composition(shapes, Lq, ref_dim, four_d, M):
    """msda_layer_fused 1 (one query GEMM with the softmax / location epilogue, bf16 operator output) against 0 (two GEMMs +
    prep kernel + fp32 operator + conversion pass): the same arithmetic, operation for operation, in a different launch
    structure -> the same bits."""
    from visionllm_amd import _lib
    mod, q, ref, src, ss, lsi, mask = _layer_case(2, shapes, Lq, ref_dim, four_d, seed=11 + ref_dim + M, M=M, C=32 * M)
    with torch.no_grad():
        old = _lib.lib().vllm_set_option(b"msda_layer_fused", 0)
        try:
            composed = mod(q, ref, src, ss, lsi, mask)
            _lib.lib().vllm_set_option(b"msda_layer_fused", 1)
            fused = mod(q, ref, src, ss, lsi, mask)
        finally:
            _lib.lib().vllm_set_option(b"msda_layer_fused", old)
    assert torch.isfinite(fused.float()).all()
    assert torch.equal(fused, composed), float((fused.float() - composed.float()).abs().max())
    truth, ref_bf16 = _layer_truth(mod, q, ref, src, ss, lsi, mask)
    o = fused.double().cpu().numpy()
    rms = np.sqrt((truth ** 2).mean())
    assert np.sqrt(((o - truth) ** 2).mean()) / rms <= max(np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms * 1.05, 4e-3)


@pytest.mark.parametrize("B,shapes,Lq,ref_dim,four_d,masked", [
    (2, [(60, 64), (30, 32), (15, 16), (8, 8)], None, 2, 0, True),     # encoder shape: M = 2 * 5104 rows (M % 4 == 0: the mask travels with the chunks)
    (3, [(60, 64), (30, 32), (15, 16), (8, 8)], 1371, 4, 0, True),     # boxes; query rows 4113 = 64 * 64 + 17 (ragged last chunk)
    (3, [(60, 64), (30, 32), (15, 16), (8, 8)], 1371, 4, 1, False),    # UniPose 4D normalizer, no mask
    (1, [(61, 67), (30, 32), (15, 16), (8, 8)], None, 2, 0, True),     # M = 5367 (M % 4 != 0): the masked value GEMM stays on the tile kernel
])
def test_skinny_gemm_layer_bit_identical_to_tile_kernel(B, shapes, Lq, ref_dim, four_d, masked):
    """The weight-stationary streaming GEMM (gemm_skinny.hip: K = 256, N = 256 / 384, >= 4096 rows) against the 128 x 128 tile kernel
    it replaces for the layer's three linears -- same MFMA, same K order, same epilogue arithmetic -> the layer's output is the
    same bits with the option on and off (value GEMM with / without key-padding mask, query GEMM with the softmax / location
    epilogue for 2-d / 4-d reference points, output GEMM), and two runs agree (race screen of the 4-stage ring)."""
    from visionllm_amd import _lib
    mod, q, ref, src, ss, lsi, mask = _layer_case(B, shapes, Lq, ref_dim, four_d, seed=77 + ref_dim + four_d, masked=masked)
    with torch.no_grad():
        old = _lib.lib().vllm_set_option(b"gemm_skinny", 0)
        old_v = _lib.lib().vllm_set_option(b"msda_layer_value_bf16", 0)   # (the bf16 value of decoder shapes exists on the streaming kernel only:
        try:                                                               #  this test compares the two kernels on the SAME, fp32-value path)
            tile = mod(q, ref, src, ss, lsi, mask)
            _lib.lib().vllm_set_option(b"gemm_skinny", 1)
            skinny = mod(q, ref, src, ss, lsi, mask)
            again = mod(q, ref, src, ss, lsi, mask)
        finally:
            _lib.lib().vllm_set_option(b"gemm_skinny", old)
            _lib.lib().vllm_set_option(b"msda_layer_value_bf16", old_v)
    assert torch.isfinite(skinny.float()).all()
    assert torch.equal(skinny, again)
    assert torch.equal(skinny, tile), float((skinny.float() - tile.float()).abs().max())


@pytest.mark.parametrize("B,shapes,ref_dim,four_d", [
    (1, [(64, 72), (32, 36), (16, 18)], 2, 0),     # the 3-level pixel decoder (msdeformattn_pixel_decoder.py:57-58): L * P = 12
    (2, [(48, 40), (24, 20), (12, 10)], 4, 1),     # 3 levels, boxes, 4D normaliser
    (1, [(64, 80), (32, 40)], 2, 0),               # 2 levels: L * P = 8
    (1, [(72, 64)], 4, 0),                         # 1 level
])
def test_fused_layer_fewer_than_four_levels_streaming_epilogue(B, shapes, ref_dim, four_d):
    """L * P in {4, 8, 12}: with d_model 256, 8 heads, 4 points and >= 4096 query rows the query GEMM's
    softmax / location epilogue runs in the streaming kernel (a head's 8 L offsets / 4 L logits padded to 32 / 16 feature slots of
    its wave) -- against the explicit composition (two GEMMs + msda_prep_generic_kernel, which sums the L * P exponentials
    sequentially: same value to fp32 rounding, not the same bits) and against the fp64 oracle."""
    from visionllm_amd import _lib
    mod, q, ref, src, ss, lsi, mask = _layer_case(B, shapes, None, ref_dim, four_d, seed=31 + len(shapes) + ref_dim)
    assert q.shape[0] * q.shape[1] >= 4096
    with torch.no_grad():
        old = _lib.lib().vllm_set_option(b"msda_layer_fused", 0)
        try:
            composed = mod(q, ref, src, ss, lsi, mask)
            _lib.lib().vllm_set_option(b"msda_layer_fused", 1)
            fused = mod(q, ref, src, ss, lsi, mask)
            again = mod(q, ref, src, ss, lsi, mask)
        finally:
            _lib.lib().vllm_set_option(b"msda_layer_fused", old)
    assert torch.isfinite(fused.float()).all() and torch.equal(fused, again)
    d = (fused.float() - composed.float()).abs()
    assert float(d.max()) <= 2.0 ** -7 * float(composed.float().abs().max()), float(d.max())     # at most an output ulp or two
    assert float((d > 0).float().mean()) < 0.02                                                    # ... and rarely
    truth, ref_bf16 = _layer_truth(mod, q, ref, src, ss, lsi, mask)
    o = fused.double().cpu().numpy()
    rms = np.sqrt((truth ** 2).mean())
    assert np.sqrt(((o - truth) ** 2).mean()) / rms <= max(np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms * 1.05, 4e-3)
    assert np.abs(o - truth).max() <= 2e-2 * np.abs(truth).max()


@pytest.mark.parametrize("B,ref_dim,four_d,masked", [(2, 2, 0, True), (2, 4, 0, False), (1, 4, 1, True)])
def test_fused_layer_decoder_shape_bf16_value(B, ref_dim, four_d, masked, monkeypatch):
    """Decoder cross-attention (Lq != S) over a large value set: the operator is the gather kernel whatever the value's dtype, so the
    layer stores the value in bf16 (streaming value GEMM with the key-padding mask, `vllm_msda_forward_bf16`) -- what the reference's
    bf16 module computes (it rounds the value to bf16 before the upcast, ...mask_dn.py:764-766).  Against the fp64 oracle with the
    usual bound (not further than the reference's bf16 arithmetic), the two launch structures agree bit for bit, and the fp32-value
    path (VLLM_MSDA_LAYER_VALUE_BF16=0 in a fresh process is the A/B; here: the bound holds for whichever ran)."""
    from visionllm_amd import _lib
    shapes = [(96, 96), (48, 48), (24, 24), (12, 12)]
    mod, q, ref, src, ss, lsi, mask = _layer_case(B, shapes, 900, ref_dim, four_d, seed=91 + ref_dim + B, masked=masked)
    assert src.shape[0] * src.shape[1] >= 4096
    with torch.no_grad():
        old = _lib.lib().vllm_set_option(b"msda_layer_fused", 0)
        try:
            composed = mod(q, ref, src, ss, lsi, mask)
            _lib.lib().vllm_set_option(b"msda_layer_fused", 1)
            fused = mod(q, ref, src, ss, lsi, mask)
            again = mod(q, ref, src, ss, lsi, mask)
        finally:
            _lib.lib().vllm_set_option(b"msda_layer_fused", old)
    assert torch.isfinite(fused.float()).all() and torch.equal(fused, again)
    assert torch.equal(fused, composed), float((fused.float() - composed.float()).abs().max())
    truth, ref_bf16 = _layer_truth(mod, q, ref, src, ss, lsi, mask)
    o = fused.double().cpu().numpy()
    rms = np.sqrt((truth ** 2).mean())
    err, err_ref = np.sqrt(((o - truth) ** 2).mean()) / rms, np.sqrt(((ref_bf16 - truth) ** 2).mean()) / rms
    print(json.dumps(dict(case=f"decoder layer B{B} ref_dim{ref_dim}", rel_rms=err, ref_bf16_rel_rms=err_ref)))
    assert err <= max(err_ref * 1.05, 4e-3), (err, err_ref)
    assert np.abs(o - truth).max() <= 2e-2 * np.abs(truth).max()


@pytest.mark.parametrize("M", [4096, 4097, 5000, 16384 + 63, 70001])
@pytest.mark.parametrize("epi", ["bias", "f32", "f32_masked"])
def test_skinny_gemm_vs_tile_kernel_and_fp32(M, epi):
    """The same through the C entry point `vllm_gemm_bf16` (K = 256, N = 256): automatic choice (the streaming kernel) against
    VLLM_GEMM_FORCE_128, bit for bit, ragged row counts (last chunk of 1 ... 63 rows, more chunks than CUs and fewer), strided
    input rows; and against torch fp32 within the GEMM's per-element bound."""
    from visionllm_amd import _lib
    torch.manual_seed(M)
    K = N = 256
    ldx = 256 if M % 2 else 320
    xs = _bf(torch.randn(M, ldx, device=DEV))
    x = xs[:, :K]
    w = _bf(torch.randn(N, K, device=DEV) * 0.06)
    b = _bf(torch.randn(N, device=DEV))
    masked = epi == "f32_masked"
    if masked and M % 4:
        pytest.skip("a mask with M % 4 != 0 stays on the tile kernel (covered by the layer test)")
    mask = (torch.rand(M, device=DEV) < 0.2).to(torch.uint8) if masked else None
    f32 = epi != "bias"
    code = 5 if f32 else 0

    def run(force):
        y = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32 if f32 else torch.bfloat16)
        _lib.check(_lib.lib().vllm_gemm_bf16(_lib.ptr(xs), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), M, N, K, ldx, K, N, code | force, None,
                                             _lib.ptr(mask) if masked else None, 0, 0, _lib.current_stream()), "gemm")
        return y
    auto, auto2, tile = run(0), run(0), run(0x100)
    assert torch.equal(auto, auto2)
    assert torch.equal(auto, tile), float((auto.float() - tile.float()).abs().max())
    ref = x.float() @ w.float().t() + b.float()
    if masked:
        ref = ref.masked_fill(mask.bool()[:, None], 0.0)
    mag = x.float().abs() @ w.float().abs().t() + b.float().abs()
    err = (auto.float() - ref).abs()
    bound = mag * 2.0 ** -17 + (ref.abs() * 2.0 ** -8 if not f32 else 0.0) + 1e-6
    assert bool((err <= bound).all()), float((err / bound).max())


def test_fused_layer_module_flavours_and_fallbacks():
    shapes = [(12, 16), (6, 8), (3, 4)]
    mod, q, ref, src, ss, lsi, mask = _layer_case(2, shapes, 40, 2, 0, seed=5, C=128, M=4)
    with torch.no_grad():
        expect = mod(q, ref, src, ss, lsi, mask)
        mm = A.MultiScaleDeformableAttention(embed_dims=128, num_heads=4, num_levels=3, num_points=4, dropout=0.0)
        mm = mm.to(DEV).to(torch.bfloat16).eval()
        mm.load_state_dict(mod.state_dict())
        o2 = mm(q.permute(1, 0, 2), value=src.permute(1, 0, 2), key_padding_mask=mask, reference_points=ref,
                spatial_shapes=ss, level_start_index=lsi)
        torch.testing.assert_close(o2.permute(1, 0, 2).float(), (expect + q).float(), rtol=1e-2, atol=1e-2)

        class Cfg:
            d_model, num_feature_levels, disable_custom_kernels = 128, 3, False
        gd = A.GroundingDinoMultiscaleDeformableAttention(Cfg(), 4, 4).to(DEV).to(torch.bfloat16).eval()
        gd.load_state_dict(mod.state_dict())
        o3, aw3 = gd(q, attention_mask=~mask, encoder_hidden_states=src, reference_points=ref, spatial_shapes=ss,
                     level_start_index=lsi)
        assert aw3 is None and torch.equal(o3, expect)
        # asking for the attention weights takes the composed path (same result to bf16 rounding, weights returned)
        o4, aw4 = gd(q, attention_mask=~mask, encoder_hidden_states=src, reference_points=ref, spatial_shapes=ss,
                     level_start_index=lsi, output_attentions=True)
        assert aw4 is not None and aw4.shape == (2, 40, 4, 3, 4)
        torch.testing.assert_close(o4.float(), expect.float(), rtol=3e-2, atol=3e-2)
    # fp32 modules and training keep the composed path
    assert not A.msda_layer_fused_ok(q.float(), src.float(), mod.value_proj)
    assert not A.msda_layer_fused_ok(q, src, mod.value_proj)          # grad enabled + trainable parameters
    with pytest.raises(ValueError):
        A.msda_layer_forward(q, ref[..., :1].expand(-1, -1, -1, 3), src, ss, lsi, None, mod.value_proj, mod.sampling_offsets,
                             mod.attention_weights, mod.output_proj, 4, 3, 4)



# ---------------------------------------------------------------------------------------------------------
# round 3: host-known level geometry (one kernel launch instead of two) and inference-mode tensors
@pytest.mark.parametrize("shapes", [[(72, 64), (36, 32), (18, 16), (9, 8)], [(50, 83), (25, 42), (13, 21), (7, 11)], [(61, 83), (31, 42), (9, 5)]])
def test_geometry_hint_changes_launches_not_results(shapes):
    """vllm_msda_forward_f32_geo: UNKNOWN (both kernels enqueued, the device picks), the hint a module's shape check leaves
    behind (exactly one kernel) and the opposite extreme (GENERAL forced for a pyramid) give the same tensor."""
    from visionllm_amd import _lib
    g = make_inputs(2, 8, 32, shapes, 4, mode="encoder_like", seed=11)
    v, ss, lsi, loc, w = _t(g["value"]), _t(g["shapes"]), _t(g["lsi"]), _t(g["loc"]), _t(g["attw"])
    B, S, M, D = v.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    assert A.known_geometry(ss, Lq) == A.GEO_UNKNOWN          # nobody has looked at this tensor object yet
    unknown = A.ms_deform_attn_forward(v, ss, lsi, loc, w, 64)
    geo = A.remember_geometry(ss)
    is_pyr = A.nested_maps(shapes)   # exact halves or ceil- / floor-divided levels; (31, 42) -> (9, 5) is neither
    assert is_pyr == (shapes[-1] != (9, 5))
    exact = shapes[0] == (72, 64)
    assert geo == (A.GEO_PYRAMID if exact else A.GEO_NESTED if is_pyr else A.GEO_GENERAL) and A.known_geometry(ss, Lq) == geo
    assert A.known_geometry(ss, Lq - 1) == (A.GEO_GENERAL if is_pyr else geo)   # a pyramid only for the encoder's queries
    hinted = A.ms_deform_attn_forward(v, ss, lsi, loc, w, 64)
    assert torch.equal(hinted, unknown)
    ref = O.forward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"])
    np.testing.assert_allclose(hinted.cpu().numpy(), ref, rtol=4e-6, atol=4e-6)
    out = torch.empty_like(unknown)
    _lib.check(_lib.lib().vllm_msda_forward_f32_geo(_lib.ptr(v), _lib.ptr(ss), _lib.ptr(lsi), _lib.ptr(loc), _lib.ptr(w), B, S, M,
                                                    D, L, Lq, P, A.GEO_GENERAL, _lib.ptr(out), _lib.current_stream(v.device)))
    torch.testing.assert_close(out, unknown, rtol=2e-6, atol=2e-6)    # generation 4 instead of 7: same sums, other order
    with pytest.raises(RuntimeError):
        _lib.check(_lib.lib().vllm_msda_forward_f32_geo(_lib.ptr(v), _lib.ptr(ss), _lib.ptr(lsi), _lib.ptr(loc), _lib.ptr(w), B, S,
                                                        M, D, L, Lq, P, 7, _lib.ptr(out), _lib.current_stream(v.device)))
    ss.mul_(1)                                                  # an in-place change bumps the version: knowledge is dropped
    assert A.known_geometry(ss, Lq) == A.GEO_UNKNOWN


def test_modules_run_under_inference_mode():
    """Inference tensors have no version counter (`t._version` raises): the shape-facts cache must not depend on it
    (level_pixels crashed every module under torch.inference_mode(), the normal way to serve)."""
    shapes = [(12, 16), (6, 8), (3, 4)]
    mod, q, ref, src, ss, lsi, mask = _layer_case(2, shapes, 40, 2, 0, seed=5, C=128, M=4)
    with torch.no_grad():
        expect = mod(q, ref, src, ss, lsi, mask)
    with torch.inference_mode():
        ss_i = torch.tensor(shapes, dtype=torch.int64, device=DEV)          # an inference tensor
        with pytest.raises(RuntimeError):
            ss_i._version
        assert A.level_pixels(ss_i) == sum(h * w for h, w in shapes)
        assert A.known_geometry(ss_i, 40) == A.GEO_UNKNOWN                   # never cached: a change could not be seen
        got = mod(q, ref, src, ss_i, lsi, mask)
        assert torch.equal(got, expect)
        m32 = A.MSDeformAttn(d_model=128, n_levels=3, n_heads=4, n_points=4).to(DEV).eval()   # fp32: the composed path
        o32 = m32(q.float(), ref, src.float(), ss_i, lsi, mask)
        assert torch.isfinite(o32).all()
