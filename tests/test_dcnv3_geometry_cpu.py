"""CPU: the anchors of the non-square DCNv3 geometry tests (tests/dcnv3_geometry_inputs.py).  The GPU tests compare every kernel with
oracle/dcnv3_oracle.c, so the oracle itself is pinned here on kernel, stride, pad and dilation that differ between h and w:
against the reference's own fp64 run (tests/golden/dcnv3_geometry.npz), against the independent torch restatement `reference_fp64`
and its autograd, and -- for unequal pads, which the reference's twin cannot express -- against itself on an explicitly padded map."""
import functools

import numpy as np
import pytest

import dcnv3_geometry_inputs as GI
from conftest import load_golden
from oracle import dcnv3 as O

C = 3                          # channels per group of the oracle-only runs (the oracle has one path for every channel count)
ENTRIES = [(name, hw) for name in GI.NAMES for hw in GI.MAPS]
ENTRY_IDS = [f"{name}-{h}x{w}" for name, (h, w) in ENTRIES]
FIXTURE = ["k2x3", "s1x2", "s2x1", "d2x1", "k3x2_s1x2_d2x1"]


@functools.lru_cache(maxsize=None)
def _oracle64(name, H, W, scale):
    """fp64 operands (the fp32 inputs widened) and the fp64 oracle's forward and backward on them, computed once per case"""
    inp, off, msk, go = (a.astype(np.float64) for a in GI.make_inputs(name, H, W, C))
    geo = GI.GEOMETRIES[name]
    out = O.forward(inp, off, msk, *geo, GI.G, C, scale)
    return (inp, off, msk, go), out, O.backward(inp, off, msk, go, *geo, GI.G, C, scale)


def test_the_table_is_what_the_tests_say_it_is():
    g = GI.GEOMETRIES
    assert len(g) == 12 and sorted({kh * kw for kh, kw, *_ in g.values()}) == [5, 6, 9]
    swap = lambda t: tuple(v for i in range(0, 8, 2) for v in (t[i + 1], t[i]))
    for a, b in (("k3x2", "k2x3"), ("k5x1", "k1x5"), ("s1x2", "s2x1"), ("p0x2", "p2x0"), ("d1x2", "d2x1"), ("all", "all_T")):
        assert g[b] == swap(g[a]) and g[a] != g[b]
    for name in ("all", "all_T"):
        assert all(g[name][i] != g[name][i + 1] for i in range(0, 8, 2))         # every pair differs at once
    for name in GI.NAMES[:10]:
        pairs = [i for i in range(0, 8, 2) if g[name][i] != g[name][i + 1]]
        # one pair at a time (a 5 x 1 kernel and a dilated one need their own pad to keep the output the size of the map)
        assert pairs in ([0], [2], [4], [6], [0, 4], [4, 6]), (name, pairs)


@pytest.mark.parametrize("scale", GI.SCALES)
@pytest.mark.parametrize("name,hw", ENTRIES, ids=ENTRY_IDS)
def test_conditions_on_the_inputs(name, hw, scale):
    """A condition, not a measurement: every case has an output, and both the accepted and the rejected branch of the acceptance
    test see a real share of its points (a case that leaves the band gets another offset spread in OFFSET_SPREAD, never another band)."""
    Ho, Wo = GI.out_size(*hw, *GI.GEOMETRIES[name])
    assert Ho >= 1 and Wo >= 1
    share = GI.accepted_share((name, *hw, scale))
    assert 0.30 <= share <= 0.95, share
    if hw == (5, 23):
        assert 3 <= Ho <= 7            # lower than one 8 x 8 output tile
    off, msk = GI.make_points(name, *hw)
    assert np.isfinite(off).all() and np.isfinite(msk).all()


@pytest.mark.parametrize("D", [4, 5])
@pytest.mark.parametrize("tag", FIXTURE)
def test_oracle_vs_reference_fixture(tag, D):
    """The fp64 oracle against the reference's dcnv3_core_pytorch and its fp64 autograd (bounds of
    test_backward_vs_reference_autograd_golden: the twin computes its reference points in fp32)."""
    g = load_golden("dcnv3_geometry.npz")
    k = f"{tag}.c{D}."
    kh, kw, sh, sw, ph, pw, dh, dw, M, Dc = [int(v) for v in g[k + "params"]]
    assert (kh, sh, dh) != (kw, sw, dw) and ph == pw and Dc == D
    a = (kh, kw, sh, sw, ph, pw, dh, dw, M, Dc, float(g[k + "offset_scale"]))
    d = lambda key: g[k + key].astype(np.float64)
    got = (O.forward(d("input"), d("offset"), d("mask"), *a),) + O.backward(d("input"), d("offset"), d("mask"), d("grad_out"), *a)
    for x, key in zip(got, ("out_f64", "grad_input_f64", "grad_offset_f64", "grad_mask_f64")):
        ref = g[k + key]
        assert ref.dtype == np.float64 and x.shape == ref.shape and np.abs(ref).max() > 0.1
        np.testing.assert_allclose(x, ref, rtol=1e-5, atol=2e-6 * np.abs(ref).max() + 1e-12, err_msg=key)


def test_fixture_holds_the_table_entries():
    g = load_golden("dcnv3_geometry.npz")
    assert all(v.dtype.kind in "fi" for v in g.values())                                   # arrays of numbers only
    for tag in FIXTURE[:4]:
        kh, kw, sh, sw, ph, pw, dh, dw = GI.GEOMETRIES[tag]
        assert [int(v) for v in g[f"{tag}.c4.params"][:8]] == [kh, kw, sh, sw, max(ph, pw), max(ph, pw), dh, dw]
    assert [int(v) for v in g["k3x2_s1x2_d2x1.c5.params"]] == [3, 2, 1, 2, 2, 2, 2, 1, 2, 5]


@pytest.mark.parametrize("scale", GI.SCALES)
@pytest.mark.parametrize("name,hw", ENTRIES, ids=ENTRY_IDS)
def test_oracle_vs_independent_restatement(name, hw, scale):
    """The fp64 oracle against `reference_fp64` and torch's fp64 autograd of it: the same arithmetic per (point, channel), the sums in
    another order (the suite's bounds for that)."""
    (inp, off, msk, go), out, grads = _oracle64(name, *hw, scale)
    ref = GI.reference_grads(inp, off, msk, go, GI.GEOMETRIES[name], GI.G, C, scale)
    assert out.shape == ref[0].shape
    np.testing.assert_allclose(out, ref[0], rtol=1e-12, atol=1e-15)
    for x, r, key in zip(grads, ref[1:], ("grad_input", "grad_offset", "grad_mask")):
        assert x.shape == r.shape and np.abs(r).max() > 0.1
        np.testing.assert_allclose(x, r, rtol=1e-10, atol=1e-12 * np.abs(r).max() + 1e-18, err_msg=key)


@pytest.mark.parametrize("name,hw", ENTRIES, ids=ENTRY_IDS)
def test_pads_equal_an_explicitly_padded_map(name, hw):
    """Unequal pads without the twin: the oracle on (input, ph, pw) equals the oracle with pads 0, 0 on the input embedded in a zero map
    of (H + 2 ph, W + 2 pw) -- the forward, grad_offset, grad_mask, and grad_input on the interior.  Why it is an identity: both runs
    form the same location up to the shift by the pad; a corner the original run drops as outside the map is a zero of the border in
    the padded run; and a point only the padded run accepts (loc <= -1 or loc >= size in the original's coordinates) has all four
    corners in the border or outside, so it adds zeros to the output and to the three gradients and scatters into the border only.
    What differs is the fp64 rounding of the shift (no location lies on a cell border: asserted)."""
    import torch
    H, W = hw
    kh, kw, sh, sw, ph, pw, dh, dw = geo = GI.GEOMETRIES[name]
    scale = GI.scale_of(name)
    inp, off, msk, go = (a.astype(np.float64) for a in GI.make_inputs(name, H, W, C))
    big = np.zeros((GI.N, H + 2 * ph, W + 2 * pw, GI.G * C))
    big[:, ph:ph + H, pw:pw + W] = inp
    pad0 = (kh, kw, sh, sw, 0, 0, dh, dw)
    assert GI.out_size(H + 2 * ph, W + 2 * pw, *pad0) == GI.out_size(H, W, *geo)
    out, out_p = O.forward(inp, off, msk, *geo, GI.G, C, scale), O.forward(big, off, msk, *pad0, GI.G, C, scale)
    gi, gof, gm = O.backward(inp, off, msk, go, *geo, GI.G, C, scale)
    gi_p, gof_p, gm_p = O.backward(big, off, msk, go, *pad0, GI.G, C, scale)
    loc_h, loc_w = GI.locations(torch.from_numpy(off), H, W, *geo, scale)
    assert float(torch.minimum((loc_h - loc_h.round()).abs().min(), (loc_w - loc_w.round()).abs().min())) > 1e-9   # no point on a cell border
    for x, r, key in ((out_p, out, "out"), (gof_p, gof, "grad_offset"), (gm_p, gm, "grad_mask"), (gi_p[:, ph:ph + H, pw:pw + W], gi, "grad_input")):
        assert np.abs(r).max() > 0.1
        assert np.abs(x - r).max() <= 1e-12 * np.abs(r).max(), (key, np.abs(x - r).max())


@pytest.mark.parametrize("name,hw", ENTRIES, ids=ENTRY_IDS)
def test_fp32_oracle_vs_fp64_oracle_forward(name, hw):
    """The GPU tests compare fp32 kernels with the fp32 instantiation of the oracle: it cannot carry a swap of its own."""
    scale = GI.scale_of(name)
    (inp, off, msk, _), out64, _ = _oracle64(name, *hw, scale)
    out32 = O.forward(inp.astype(np.float32), off.astype(np.float32), msk.astype(np.float32), *GI.GEOMETRIES[name], GI.G, C, scale)
    assert out32.dtype == np.float32
    np.testing.assert_allclose(out32, out64, rtol=2e-5, atol=2e-5)


def test_route_counter_is_a_host_query():
    from visionllm_amd import _lib
    L = _lib.lib()
    assert [L.vllm_dcnv3_route_launches(r) >= 0 for r in range(6)] == [True] * 6
    assert L.vllm_dcnv3_route_launches(-1) == -1 and L.vllm_dcnv3_route_launches(6) == -1
