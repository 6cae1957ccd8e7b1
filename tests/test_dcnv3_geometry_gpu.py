"""Every DCNv3 kernel on kernel, stride, pad and dilation that differ between h and w (tests/dcnv3_geometry_inputs.py), through the
C ABI.  The fp32 kernels against oracle/dcnv3_oracle.c (pinned on these geometries by test_dcnv3_geometry_cpu.py), the fp64 kernels
against the independent restatement `reference_fp64`, the half entries against the fp32 kernels.  Every parameter set that names a
route asserts from vllm_dcnv3_route_launches that this route, and no other, took exactly the launches the test made."""
import functools

import numpy as np
import pytest
import torch

import dcnv3_geometry_inputs as GI
from oracle import dcnv3 as O
from test_dcnv3_gpu import _on_and_next_to_integers
from visionllm_amd import _lib
from visionllm_amd import dcnv3 as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATHER, PIPE, TILED, BWD_VEC, BWD_GENERIC, BWD_WINDOWED = range(6)     # vllm_dcnv3_route_launches
ENTRIES = [(name, hw) for name in GI.NAMES for hw in GI.MAPS]
BOTH = [(name, hw) for name in ("all", "all_T") for hw in GI.MAPS]
eid = lambda v: "x".join(str(x) for x in v) if isinstance(v, tuple) else None


def _routes():
    L = _lib.lib()
    return [L.vllm_dcnv3_route_launches(r) for r in range(6)]


class _expect_launches:
    """with _expect_launches({route: launches}): the counters move by exactly that, every other route by nothing"""

    def __init__(self, moves):
        self.moves = [moves.get(r, 0) for r in range(6)]

    def __enter__(self):
        self.before = _routes()

    def __exit__(self, exc_type, *_):
        if exc_type is None:
            moved = [a - b for a, b in zip(_routes(), self.before)]
            assert moved == self.moves, f"launches per route {moved}, expected {self.moves}"


class _option:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _lib.set_option(self.name, self.value)

    def __exit__(self, *_):
        _lib.set_option(self.name, self.old)


@functools.lru_cache(maxsize=None)
def _case(name, H, W, C):
    """fp32 operands (numpy; shared, so no test writes to them) and the scale of the parameter set"""
    return GI.make_inputs(name, H, W, C), GI.scale_of(name)


@functools.lru_cache(maxsize=None)
def _forward_ref(name, H, W, C):
    (inp, off, msk, _), scale = _case(name, H, W, C)
    return O.forward(inp, off, msk, *GI.GEOMETRIES[name], GI.G, C, scale)


@functools.lru_cache(maxsize=None)
def _backward_ref(name, H, W, C):
    """fp32 oracle gradients and the magnitude of the terms that enter an element of grad_input (the same scatter with absolute values)"""
    (inp, off, msk, go), scale = _case(name, H, W, C)
    geo = GI.GEOMETRIES[name]
    ri, ro, rm = O.backward(inp, off, msk, go, *geo, GI.G, C, scale)
    mi, _, _ = O.backward(np.abs(inp), off, np.abs(msk), np.abs(go), *geo, GI.G, C, scale)
    return ri, ro, rm, mi


def _dev(arrays, dtype=None):
    return [torch.from_numpy(a).to(DEV) if dtype is None else torch.from_numpy(a).to(DEV).to(dtype) for a in arrays]


@pytest.mark.parametrize("C", [16, 32])
@pytest.mark.parametrize("name,hw", ENTRIES, ids=eid)
def test_forward_f32_every_route(name, hw, C):
    """dcnv3_tiled 0 / 1 / 3 = the gather, the pipelined and the two-blocks-per-CU kernel: each took its launches, matches the oracle,
    gives the same bits twice, and the tiled kernels match the gather kernel (bounds of test_tiled_kernel_vs_oracle_and_gather_kernel)."""
    (inp, off, msk, _), scale = _case(name, *hw, C)
    a = (*_dev((inp, off, msk)), *GI.GEOMETRIES[name], GI.G, C, scale)
    res = {}
    for mode, route in ((0, GATHER), (1, PIPE), (3, TILED)):
        with _option("dcnv3_tiled", mode), _expect_launches({route: 2}):
            res[mode] = (A.dcnv3_forward(*a), A.dcnv3_forward(*a))
    ref = _forward_ref(name, *hw, C)
    for mode, (out, again) in res.items():
        assert out.shape == ref.shape
        assert torch.equal(out, again), f"dcnv3_tiled = {mode}: two runs differ"
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-5, atol=2e-5, err_msg=f"dcnv3_tiled = {mode}")
        if mode:
            torch.testing.assert_close(out, res[0][0], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name,hw,C", [(n, hw, C) for n, hw in BOTH for C in (64, 20, 7, 1)] +
                         [(n, hw, C) for n in ("s1x2", "d2x1") for hw in GI.MAPS for C in (20, 7)], ids=eid)
def test_forward_f32_other_group_channels(name, hw, C):
    """The gather kernel's four instantiations: four channels per lane with a non-3x3 kernel (64, 20) and with the unrolled 3x3 loop on
    non-square stride and dilation (20), one channel per lane likewise (7, 1; 7)."""
    (inp, off, msk, _), scale = _case(name, *hw, C)
    with _expect_launches({GATHER: 1}):
        out = A.dcnv3_forward(*_dev((inp, off, msk)), *GI.GEOMETRIES[name], GI.G, C, scale)
    ref = _forward_ref(name, *hw, C)
    assert out.shape == ref.shape
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


BWD = [(n, hw, C, tiled, route) for n, hw in ENTRIES for C, tiled, route in ((32, 1, BWD_WINDOWED), (32, 0, BWD_VEC), (16, 1, BWD_VEC))] + \
      [(n, hw, C, 1, route) for n, hw in BOTH for C, route in ((4, BWD_VEC), (8, BWD_VEC), (64, BWD_VEC), (20, BWD_GENERIC), (7, BWD_GENERIC))]


@pytest.mark.parametrize("name,hw,C,tiled,route", BWD, ids=eid)
def test_backward_f32_every_route(name, hw, C, tiled, route):
    """The windowed matrix-core kernel (32 channels per group, dcnv3_bwd_tiled 1), the vectorised kernel with 1, 2, 4, 8 and 16 lanes per
    group (4 ... 64 channels) and the generic kernel (20, 7) against the fp32 oracle, with the bounds of test_backward_f32_vs_oracle."""
    arrays, scale = _case(name, *hw, C)
    a = _dev(arrays)
    call = lambda: A.dcnv3_backward(a[0], a[1], a[2], *GI.GEOMETRIES[name], GI.G, C, scale, a[3])
    with _option("dcnv3_bwd_tiled", tiled), _expect_launches({route: 2}):
        (gi, gof, gm), (gi2, gof2, gm2) = call(), call()
    ri, ro, rm, mi = _backward_ref(name, *hw, C)
    assert torch.isfinite(gi).all() and torch.isfinite(gof).all() and torch.isfinite(gm).all()
    assert torch.equal(gof, gof2) and torch.equal(gm, gm2)                     # fixed reduction trees
    assert (np.abs(gi.cpu().numpy() - ri) <= 2.0 ** -18 * mi + 1e-7).all()
    assert (np.abs(gi2.cpu().numpy() - gi.cpu().numpy()) <= 2.0 ** -18 * mi + 1e-7).all()
    sc_o, sc_m = np.abs(ro).max() + 1e-12, np.abs(rm).max() + 1e-12
    np.testing.assert_allclose(gof.cpu().numpy(), ro, rtol=2e-4, atol=3e-6 * sc_o)
    np.testing.assert_allclose(gm.cpu().numpy(), rm, rtol=2e-4, atol=3e-6 * sc_m)


@pytest.mark.parametrize("C,route", [(7, BWD_GENERIC), (32, BWD_VEC)])
@pytest.mark.parametrize("name", ["all", "all_T", "k5x1", "p0x2"])
def test_fp64_kernels_vs_independent_restatement(name, C, route):
    """The fp64 forward, and the three gradients through DCNv3Function under autograd (which also pins the order in which the function
    stores and unpacks its geometry), against `reference_fp64` and torch's fp64 autograd of it: the suite's bounds for the fp64 kernels
    against the fp64 oracle."""
    H, W = GI.MAPS[0]
    arrays, scale = _case(name, H, W, C)
    geo = GI.GEOMETRIES[name]
    ref = GI.reference_grads(*arrays, geo, GI.G, C, scale)
    inp, off, msk, go = _dev(arrays, torch.float64)
    with _expect_launches({GATHER: 1}):
        out = A.dcnv3_forward(inp, off, msk, *geo, GI.G, C, scale)
    np.testing.assert_allclose(out.cpu().numpy(), ref[0], rtol=1e-12, atol=1e-15)
    inp, off, msk = (t.requires_grad_(True) for t in (inp, off, msk))
    with _expect_launches({GATHER: 1, route: 1}):
        out2 = A.DCNv3Function.apply(inp, off, msk, *geo, GI.G, C, scale, 256)
        out2.backward(go)
    assert torch.equal(out2.detach(), out)
    for got, r, key in zip((inp.grad, off.grad, msk.grad), ref[1:], ("grad_input", "grad_offset", "grad_mask")):
        assert got.shape == r.shape
        np.testing.assert_allclose(got.cpu().numpy(), r, rtol=1e-10, atol=1e-12 * max(np.abs(r).max(), 1e-30) + 1e-18, err_msg=key)


@pytest.mark.parametrize("C,route", [(16, BWD_VEC), (32, BWD_WINDOWED), (5, BWD_GENERIC)])
@pytest.mark.parametrize("name", ["all", "all_T"])
def test_half_precision_entries(name, C, route):
    """Operands rounded to half: the half entry points add nothing but the conversions to the fp32 kernels (second check of
    test_half_precision_forward_and_backward), raw and through DCNv3Function's autograd."""
    H, W = GI.MAPS[0]
    arrays, scale = _case(name, H, W, C)
    a = (*GI.GEOMETRIES[name], GI.G, C, scale)
    inp, off, msk, go = _dev(arrays, torch.float16)
    with _expect_launches({GATHER: 1}):
        out = A.dcnv3_forward(inp, off, msk, *a)
    assert out.dtype == torch.float16
    with _option("dcnv3_tiled", 0), _expect_launches({GATHER: 1}):      # the gather kernel: the half kernel is its instantiation
        out32 = A.dcnv3_forward(inp.float(), off.float(), msk.float(), *a)
    assert torch.equal(out, out32.half())
    with _expect_launches({route: 2}):
        gi, gof, gm = A.dcnv3_backward(inp, off, msk, *a, go)
        gi32, gof32, gm32 = A.dcnv3_backward(inp.float(), off.float(), msk.float(), *a, go.float())
    assert gi.dtype == gof.dtype == gm.dtype == torch.float16
    assert float(gof32.abs().max()) > 0.1 and float(gm32.abs().max()) > 0.1
    assert torch.equal(gof, gof32.half()) and torch.equal(gm, gm32.half())
    torch.testing.assert_close(gi.float(), gi32, rtol=1e-3, atol=1e-3 * float(gi32.abs().max()))    # (atomics: the fp32 sums differ in the last bits run to run)
    x, o, m = (t.clone().requires_grad_(True) for t in (inp, off, msk))
    with _expect_launches({GATHER: 1, route: 1}):
        o2 = A.DCNv3Function.apply(x, o, m, *a, 256)
        o2.backward(go)
    assert torch.equal(o2.detach(), out) and x.grad.dtype == torch.float16
    assert torch.equal(o.grad, gof) and torch.equal(m.grad, gm)
    torch.testing.assert_close(x.grad.float(), gi.float(), rtol=1e-3, atol=1e-3 * float(gi32.abs().max()))


@pytest.mark.parametrize("C,moves", [(32, {GATHER: 1, PIPE: 1, TILED: 1, BWD_VEC: 1, BWD_WINDOWED: 1}),
                                     (16, {GATHER: 1, PIPE: 1, TILED: 1, BWD_VEC: 2})], ids=["c32", "c16"])
@pytest.mark.parametrize("name", ["all", "all_T", "s1x2", "d2x1"])
def test_locations_on_and_next_to_integers_non_square(name, C, moves):
    """The construction and the bounds of test_locations_on_and_next_to_integers_land_in_the_same_cell_in_every_kernel on non-square
    geometry: both dcnv3_bwd_tiled values and the three forward routes, each of which took its launch."""
    with _expect_launches(moves):
        _on_and_next_to_integers(GI.scale_of(name), C, GI.GEOMETRIES[name])
