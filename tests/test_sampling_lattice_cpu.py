"""CPU: the lattice inputs are what they claim, and the fixed-cell reference (lattice_inputs.fixed_cell_msda) is the C oracle's
operation -- so that test_sampling_lattice_gpu.py holds the kernels to a reference that is itself inside the bounds it sets."""
import numpy as np
import pytest
import torch

import lattice_inputs as LI
from oracle import msda as O

MAP_SETS = {"encoder": LI.ENCODER_MAPS, "odd": LI.ODD_MAPS}


@pytest.mark.parametrize("maps", sorted(MAP_SETS))
def test_the_init_state_is_on_the_lattice(maps):
    """M = 8, P = 4, the module's own statements in fp32: at least a fifth of the points lie within 1e-4 px of a cell border and at
    least a twentieth fall into another cell in fp64 than in fp32 (measured: 0.250 / 0.077 on the encoder maps, 0.509 / 0.313 on the
    odd ones).  A later edit that moves the inputs off the lattice fails here."""
    shapes = MAP_SETS[maps]
    loc = LI.init_state_locations(shapes, 8, 4, 1)
    assert loc.dtype == np.float32 and loc.shape == (1, sum(h * w for h, w in shapes), 8, len(shapes), 4, 2)
    near, flip = LI.lattice_shares(shapes, loc)
    print(f"{maps}: init near-border share {near:.3f}, fp32/fp64 cell-flip share {flip:.3f}")
    assert near >= 0.2 and flip >= 0.05, (near, flip)
    # the statements: pixel-centre reference points, the bias grid of _init_msda_parameters, ref + off / (W, H)
    grid = LI.offset_bias_grid(8, len(shapes), 4)
    assert float(grid[2, 0, 0, 0]) == pytest.approx(-4.37e-8, rel=1e-2) and float(grid[2, 0, 3, 1]) == 4.0
    assert (grid.abs().amax(-1)[:, :, 3] == 4.0).all()
    H, W = shapes[0]
    q = 5 * W + 7                                                        # the cell (5, 7) of level 0, head 0: k + 1 pixels to the right
    for k in range(4):
        assert loc[0, q, 0, 0, k, 0] == np.float32((np.float32(7.5) / np.float32(W)) + np.float32(k + 1) / np.float32(W))
        assert loc[0, q, 0, 0, k, 1] == np.float32(np.float32(5.5) / np.float32(H))
    # the nudged form stays on the lattice and reaches every acceptance edge from both sides
    nd, where = LI.nudged(loc, 3, shapes, with_edges=True)
    near_n, flip_n = LI.lattice_shares(shapes, nd)
    print(f"{maps}: nudged near-border share {near_n:.3f}, cell-flip share {flip_n:.3f}")
    # (a move of one ulp is under 1e-5 px on these maps, so the near-border share cannot fall; which side the fp32 product then rounds
    #  to is a coin's toss per coordinate, so a good part of the init state's flips must remain: a fifth of its bound is asked for)
    assert near_n >= 0.2 and flip_n >= 0.01
    moved = np.abs(nd.astype(np.float64) - loc.astype(np.float64))
    assert ((nd != loc).any(-1).mean() > 0.5) and (moved > 1e-6).any(-1).mean() < 0.07        # one ulp, but for the edge triples
    on_edge = {e: 0 for e in ("h=-1", "h=H", "w=-1", "w=W")}
    for l, (H, W) in enumerate(shapes):
        y, x = nd[:, :, :, l, :, 1], nd[:, :, :, l, :, 0]
        h_im = (y * np.float32(H)).astype(np.float32) - np.float32(0.5)
        w_im = (x * np.float32(W)).astype(np.float32) - np.float32(0.5)
        for e, hit in (("h=-1", h_im == -1), ("h=H", h_im == H), ("w=-1", w_im == -1), ("w=W", w_im == W)):
            on_edge[e] += int(hit.sum())
    assert all(v > 0 for v in on_edge.values()), on_edge
    # the construction, per edge: every point on it and every neighbour just outside it is rejected; neighbours just inside it are
    # accepted (all of them whose other coordinate is inside the map -- the lattice reaches past the map at its rim)
    _, _, ok = LI.cells(shapes, nd)
    _, _, ok0 = LI.cells(shapes, loc)
    ok, ok0 = ok.reshape(-1), ok0.reshape(-1)
    for e in range(4):
        pick = where["edge"] == e
        on, inside, outside = (where[k][pick] for k in ("on", "inside", "outside"))
        assert pick.sum() > 0 and not ok[on].any() and not ok[outside].any(), e
        assert ok[inside].sum() > 0 and ok[inside][ok0[inside]].all(), e
    assert (~ok).mean() < 0.5


CPU_CASES = [(LI.ENCODER_MAPS, 8, 4, 4, 1, None), (LI.ODD_MAPS, 3, 4, 4, 1, None), (LI.SMALL_MAPS, 4, 6, 2, 2, 77)]


@pytest.mark.parametrize("variant", ["init", "nudged"])
@pytest.mark.parametrize("shapes,M,D,P,B,Lq", CPU_CASES)
def test_fixed_cell_reference_is_the_oracles_operation(shapes, M, D, P, B, Lq, variant):
    """fp64: with the cells of the fp64 locations the fixed-cell autograd IS oracle.msda.backward (rtol 1e-10, all three gradients, every
    point); with the cells of the fp32 locations it is still that wherever the two cells agree; and the forward agrees too."""
    g = LI.make_case(shapes, M, D, P, B, Lq, variant)
    l64 = g["loc"].astype(np.float64)
    v64, a64, go64 = g["value"].astype(np.float64), g["attw"].astype(np.float64), g["go"].astype(np.float64)
    rv, rl, rw = O.backward(v64, g["shapes"], g["lsi"], l64, a64, go64)
    h64, w64, ok64 = LI.cells(shapes, l64)
    gv, gl, gw = LI.fixed_cell_backward(v64, shapes, g["lsi"], l64, a64, go64, h64, w64, ok64, chunk=2048)
    for got, ref, n in ((gv, rv, "grad_value"), (gl, rl, "grad_sampling_loc"), (gw, rw, "grad_attn_weight")):
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-12, err_msg=n)
    out = LI.fixed_cell_msda(torch.from_numpy(v64), shapes, g["lsi"], torch.from_numpy(np.nan_to_num(l64, posinf=0, neginf=0)),
                             torch.from_numpy(a64), h64, w64, ok64)
    np.testing.assert_allclose(out.numpy(), O.forward(v64, g["shapes"], g["lsi"], l64, a64), rtol=1e-10, atol=1e-12)
    ref = LI.reference(shapes, M, D, P, B, Lq, variant)
    same = (ref["ok"] == ok64) & (~ok64 | ((ref["h"] == h64) & (ref["w"] == w64)))
    assert 0.3 < same.mean() < 1.0                                     # (both kinds of points are there)
    np.testing.assert_allclose(ref["gl"][same], rl[same], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(ref["gw"][same], rw[same], rtol=1e-10, atol=1e-12)
    # where the cells differ the two are the two one-sided derivatives: far apart (the reason the reference fixes the cell)
    flipped = ~same & ok64 & ref["ok"]
    print(f"cells differ at {flipped.mean():.3f} of the points; grad_sampling_loc there differs by up to "
          f"{np.abs(ref['gl'] - rl)[flipped].max() / np.abs(rl).max():.2f} x the tensor's largest value")


@pytest.mark.parametrize("variant", ["init", "nudged"])
@pytest.mark.parametrize("shapes,M,D,P,B,Lq", CPU_CASES + [(LI.SMALL_MAPS, 2, 71, 8, 2, 77)])
def test_fp32_oracle_is_within_the_kernels_bounds_of_the_fixed_cell_reference(shapes, M, D, P, B, Lq, variant):
    """The fp32 C oracle (the arithmetic the kernels restate) against the fixed-cell fp64 reference at EVERY point, on-lattice ones
    included, at the bounds test_sampling_lattice_gpu.py holds the kernels to: the reference alone stays inside them."""
    g = LI.make_case(shapes, M, D, P, B, Lq, variant)
    ref = LI.reference(shapes, M, D, P, B, Lq, variant)
    ov, ol, ow = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], g["go"])
    LI.check_point_gradients(ol, ow, ref, f"fp32 oracle, {variant}")
    LI.check_grad_value_f32(ov, ref, f"fp32 oracle, {variant}")
    # (the fp32 oracle's grad_value against the fixed-cell fp64 one: the sanity bound of the existing tests)
    assert np.abs(ov - ref["gv"]).max() <= 1e-3 * (1 + np.abs(ref["gv"]).max())


@pytest.mark.parametrize("shapes,M,D,P,B,Lq", [(LI.ODD_MAPS, 3, 4, 4, 1, None), (LI.SMALL_MAPS, 4, 6, 2, 2, 77)])
def test_the_check_notices_a_fused_multiply_add(shapes, M, D, P, B, Lq):
    """What the GPU file exists to catch, played through on the CPU: a kernel that evaluates ``loc * H - 0.5`` with ONE rounding (a fused
    multiply-add) where the reference rounds the product first.  Its cells are computed here, its gradients are the exact one-sided
    derivatives of THOSE cells -- and the check against the reference's cells fails (it fails on one element; here more than one point
    in a thousand misses)."""
    g = LI.make_case(shapes, M, D, P, B, Lq, "init")
    ref = LI.reference(shapes, M, D, P, B, Lq, "init")
    loc = g["loc"]
    h, w = np.zeros_like(ref["h"]), np.zeros_like(ref["w"])
    ok = np.zeros_like(ref["ok"])
    with np.errstate(invalid="ignore"):
        for l, (H, W) in enumerate(shapes):
            h_im = (loc[:, :, :, l, :, 1].astype(np.float64) * H - 0.5).astype(np.float32)      # exact in fp64, rounded once: the FMA
            w_im = (loc[:, :, :, l, :, 0].astype(np.float64) * W - 0.5).astype(np.float32)
            ok[:, :, :, l] = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
            h[:, :, :, l] = np.where(ok[:, :, :, l], np.floor(h_im), 0)
            w[:, :, :, l] = np.where(ok[:, :, :, l], np.floor(w_im), 0)
    wrong = (ok != ref["ok"]) | (ok & ((h != ref["h"]) | (w != ref["w"])))
    assert wrong.mean() > 1e-3, wrong.mean()
    _, gl, gw = LI.fixed_cell_backward(g["value"], shapes, g["lsi"], loc, g["attw"], g["go"], h, w, ok, need_value=False)
    bad = np.abs(gl - ref["gl"]) > LI.GL_TOL["atol"] + LI.GL_TOL["rtol"] * np.abs(ref["gl"])
    print(f"a fused multiply-add changes the cell of {wrong.mean():.3f} of the points; grad_sampling_loc misses its bound at {bad.any(-1).mean():.3f}")
    assert bad.any(-1).mean() > 1e-3
    with pytest.raises(AssertionError):
        LI.check_point_gradients(gl, gw, ref, "fused multiply-add")
