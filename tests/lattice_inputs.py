"""MSDA inputs ON the pixel lattice, and the reference that is defined there (test_sampling_lattice_cpu.py,
test_sampling_lattice_gpu.py, the border points of test_msda_gpu.py).

A freshly constructed deformable-attention module has zero offset weights and the direction grid as the offset bias
(``_init_msda_parameters``); the encoder's reference points are pixel centres.  On the query's own level every sampling location is
then an integer pixel position, or one ulp from it (cos(pi/2) is -4.37e-8 in fp32, one diagonal head has -0.9999996).  The forward is
continuous across a cell border; grad_sampling_loc is not, so whoever evaluates ``loc * H - 0.5`` with another rounding lands in the
neighbouring cell and returns the other one-sided derivative -- an O(1) difference.

The reference here is therefore split the way the project's contract is:
  * the CELL (h_low, w_low, accepted) is the index-exact contract: ``oracle.msda.sample_index`` on the locations in their own dtype
    (the reference's operation order, pinned by the reference's golden files);
  * the VALUE is ``fixed_cell_msda``: the reference's bilinear sum in torch fp64 with the cell GIVEN.  With the cell fixed the operation
    is a polynomial in the location, so its fp64 autograd is the one-sided derivative every kernel that is in that cell must produce, to
    the usual fp32 rounding -- no point has to be left out of a comparison.
Nothing here touches torch.cuda at import; every cached result is shared between tests: leave it unchanged."""
import functools
import types

import numpy as np
import torch
from torch import nn

from oracle import msda as O
from visionllm_amd.ms_deform_attn import _init_msda_parameters, _sampling_locations

ENCODER_MAPS = ((72, 64), (36, 32), (18, 16), (9, 8))      # nested 2x pyramid, S = 6120
ODD_MAPS = ((65, 67), (33, 34))                            # not multiples of the windowed kernel's tile, not exact halves
SMALL_MAPS = ((13, 11), (7, 6), (4, 3))                    # the maps of test_backward_f32_vectorised_vs_oracle
# the bounds of the fp32 backward against the fixed-cell fp64 reference: those of test_backward_f32_vectorised_vs_oracle and
# test_backward_f32_encoder_shape_tiled_vs_plain_vs_oracle for the points they keep (a weight is off by one ulp of h_im on either side of
# a border, as anywhere else)
GW_TOL = dict(rtol=1e-4, atol=1e-4)
GL_TOL = dict(rtol=2e-3, atol=2e-3)


def offset_bias_grid(M, L, P):
    """[M, L, P, 2] fp32: the sampling_offsets bias exactly as ``_init_msda_parameters`` leaves it (run on four stand-in linears; the
    global random state is put back)"""
    with torch.random.fork_rng(devices=[]):
        mod = types.SimpleNamespace(sampling_offsets=nn.Linear(2, 2 * M * L * P), attention_weights=nn.Linear(2, M * L * P),
                                    value_proj=nn.Linear(2, 2), output_proj=nn.Linear(2, 2))
        _init_msda_parameters(mod, M, L, P)
    return mod.sampling_offsets.bias.detach().view(M, L, P, 2).clone()


def pixel_centres(shapes, dtype=torch.float32):
    """[S, 2] (x, y): the encoder's reference points, ``linspace(0.5, H - 0.5, H) / H`` per level, levels concatenated"""
    pts = []
    for H, W in shapes:
        ys, xs = torch.meshgrid(torch.linspace(0.5, H - 0.5, H, dtype=dtype) / H, torch.linspace(0.5, W - 0.5, W, dtype=dtype) / W,
                                indexing="ij")
        pts.append(torch.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    return torch.cat(pts, 0)


def init_state_locations(shapes, M, P, B, Lq=None, dtype=torch.float32, seed=0):
    """-> numpy [B, Lq, M, L, P, 2]: the sampling locations of a fresh module, by the module's own statements in ``dtype`` (the bias grid
    is fp32 as the module holds it).  Lq None: the queries are the cells (encoder); else a seeded subset of cells per image (the
    decoder-like form the gather, vectorised and generic kernels serve)."""
    L = len(shapes)
    ref = pixel_centres(shapes, dtype)                                          # [S, 2]
    S = ref.shape[0]
    if Lq is None:
        ref = ref[None].expand(B, S, 2)
    else:
        g = torch.Generator().manual_seed(9000 + seed)
        ref = torch.stack([ref[torch.randperm(S, generator=g)[:Lq]] if Lq <= S else ref[torch.randint(0, S, (Lq,), generator=g)]
                           for _ in range(B)])
    ref = ref[:, :, None, :].expand(-1, -1, L, -1)                               # replicated over the levels (valid ratios of 1)
    off = offset_bias_grid(M, L, P).to(dtype)[None, None].expand(B, ref.shape[1], -1, -1, -1, -1)
    loc = _sampling_locations(ref, off, torch.tensor(shapes, dtype=torch.int64), P)
    assert loc.dtype == dtype
    return np.ascontiguousarray(loc.numpy())


def nudged(loc, seed, shapes, with_edges=False):
    """Every coordinate moved by -1, 0 or +1 ulp of its own dtype; a seeded 1/50 of the points put ON an acceptance edge (h_im = -1,
    h_im = H, w_im = -1 or w_im = W: rejected, the comparisons are strict), and two neighbours of each -- the same level and point
    index of the next two heads (or queries) -- just inside that edge (the nearest coordinate the reference's rounded arithmetic accepts)
    and one ulp outside it.  The triples never overlap.
    ``with_edges``: -> (locations, {"on", "inside", "outside": flat point indices, "edge": 0 h = -1, 1 h = H, 2 w = -1, 3 w = W})."""
    rng = np.random.default_rng(seed)
    dt = loc.dtype.type
    step = rng.integers(-1, 2, size=loc.shape)
    out = np.where(step > 0, np.nextafter(loc, dt(np.inf)), np.where(step < 0, np.nextafter(loc, dt(-np.inf)), loc)).astype(dt)
    B, Lq, M, L, P, _ = loc.shape
    pts = out.reshape(-1, 2)
    n, LP = pts.shape[0], L * P
    # a slot = one (level, point) position in a block of three consecutive (query, head) rows: the three rows' points at that position
    slots = np.sort(rng.choice((n // (3 * LP)) * LP, size=max(n // 50, 1), replace=False))
    base = (slots // LP) * 3 * LP + slots % LP
    edge = rng.integers(0, 4, size=base.shape)
    for k, i in enumerate(base):
        H, W = shapes[(i // P) % L]
        axis, size = (1, H) if edge[k] < 2 else (0, W)
        low = edge[k] in (0, 2)
        product = dt(-0.5) if low else dt(size + 0.5)                                     # loc * size; the edge is product - 0.5
        c = dt(product / dt(size))
        cands = [c, np.nextafter(c, dt(np.inf)), np.nextafter(c, dt(-np.inf))]
        on = next((v for v in cands if dt(v * dt(size)) == product), c)                  # the coordinate whose rounded product IS the edge
        inside, outside = (dt(np.inf), dt(-np.inf)) if low else (dt(-np.inf), dt(np.inf))
        accepted = (lambda v: dt(dt(v * dt(size)) - dt(0.5)) > -1) if low else (lambda v: dt(dt(v * dt(size)) - dt(0.5)) < size)
        near = np.nextafter(on, inside)                      # just inside: the first coordinate whose ROUNDED h_im passes the strict test
        for _ in range(16):                                  # (one ulp of the coordinate can round back onto the edge)
            if accepted(near):
                break
            near = np.nextafter(near, inside)
        pts[i, axis], pts[i + LP, axis], pts[i + 2 * LP, axis] = on, near, np.nextafter(on, outside)
    if with_edges:
        return out, dict(on=base, inside=base + LP, outside=base + 2 * LP, edge=edge)
    return out


def fixed_cell_msda(value, shapes, lsi, loc, attw, h_low, w_low, ok):
    """The reference's bilinear sum (ms_deform_im2col_cuda.cuh:33-84, 237-298) with the corner cells GIVEN as integers: torch, in
    value's dtype (fp64 for the truth), differentiable in value, loc and attw.  value [B, S, M, D], loc [B, Lq, M, L, P, 2] (x, y),
    attw, h_low, w_low, ok [B, Lq, M, L, P] -> [B, Lq, M * D].  h_im = loc * H - 0.5 in that dtype, the weights from h_im - h_low and
    w_im - w_low; a corner outside the map and a point with ``ok`` false contribute nothing (a non-finite location of such a point is
    never read)."""
    B, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    h_low, w_low = torch.as_tensor(h_low).long(), torch.as_tensor(w_low).long()
    ok = torch.as_tensor(ok).bool()
    loc = torch.where(ok[..., None], loc, torch.zeros((), dtype=loc.dtype))
    out = 0
    for l in range(L):
        H, W = int(shapes[l][0]), int(shapes[l][1])
        v = value[:, int(lsi[l]):int(lsi[l]) + H * W].permute(0, 2, 1, 3)               # [B, M, HW, D]
        tr = lambda t: t[:, :, :, l].permute(0, 2, 1, 3).reshape(B, M, Lq * P)           # [B, Lq, M, P] -> [B, M, Lq * P]
        hl, wl, live = tr(h_low), tr(w_low), tr(ok)
        lh = tr(loc[..., 1]) * H - 0.5 - hl
        lw = tr(loc[..., 0]) * W - 0.5 - wl
        acc = 0
        for dh, dw, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            hh, ww = hl + dh, wl + dw
            inside = live & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)
            idx = torch.where(inside, hh * W + ww, torch.zeros((), dtype=torch.long))
            corner = v.gather(2, idx[..., None].expand(-1, -1, -1, D)) if H * W > 0 else v.new_zeros(B, M, Lq * P, D)
            acc = acc + (wt * inside)[..., None] * corner
        out = out + (acc * tr(attw)[..., None]).view(B, M, Lq, P, D).sum(3)
    return out.permute(0, 2, 1, 3).reshape(B, Lq, M * D)


def fixed_cell_backward(value, shapes, lsi, loc, attw, grad_out, h_low, w_low, ok, chunk=1024, need_value=True):
    """fp64 autograd of ``fixed_cell_msda`` on numpy operands -> numpy (grad_value, grad_sampling_loc, grad_attn_weight); the queries are
    independent, so they go through in chunks to bound the memory (``need_value`` false: grad_value is not computed, None)"""
    v = torch.from_numpy(np.asarray(value, np.float64)).requires_grad_(need_value)
    go = torch.from_numpy(np.asarray(grad_out, np.float64)).reshape(loc.shape[0], loc.shape[1], -1)
    gl, gw = np.zeros(loc.shape, np.float64), np.zeros(attw.shape, np.float64)
    ok = np.asarray(ok).astype(bool)
    for a in range(0, loc.shape[1], chunk):
        s = slice(a, a + chunk)
        lc = torch.from_numpy(np.nan_to_num(np.asarray(loc[:, s], np.float64), nan=0.0, posinf=0.0, neginf=0.0)).requires_grad_(True)
        w = torch.from_numpy(np.asarray(attw[:, s], np.float64)).requires_grad_(True)
        assert ok[:, s][~np.isfinite(loc[:, s]).all(-1)].sum() == 0, "a non-finite location is marked accepted"
        fixed_cell_msda(v, shapes, lsi, lc, w, h_low[:, s], w_low[:, s], ok[:, s]).backward(go[:, s])
        gl[:, s], gw[:, s] = lc.grad.numpy(), w.grad.numpy()
    return (v.grad.numpy() if need_value else None), gl, gw


def fixed_cell_point_gradients(value, shapes, lsi, loc, attw, grad_out, points):
    """grad_sampling_loc / grad_attn_weight of the fixed-cell reference (cells: the index-exact contract on ``loc`` in its own dtype) for
    the queries that hold a point of ``points`` (bool [B, Lq, M, L, P]); the other queries' rows stay zero.  -> gl, gw, accepted"""
    h, w, ok = cells(shapes, loc)
    gl, gw = np.zeros(loc.shape, np.float64), np.zeros(attw.shape, np.float64)
    go = np.asarray(grad_out).reshape(loc.shape[0], loc.shape[1], -1)
    for b in range(loc.shape[0]):
        qs = np.flatnonzero(points[b].any(axis=(1, 2, 3)))
        if qs.size:
            _, l, a = fixed_cell_backward(value[b:b + 1], shapes, lsi, loc[b:b + 1, qs], attw[b:b + 1, qs], go[b:b + 1, qs], h[b:b + 1, qs],
                                          w[b:b + 1, qs], ok[b:b + 1, qs], need_value=False)
            gl[b, qs], gw[b, qs] = l[0], a[0]
    return gl, gw, ok


def cells(shapes, loc):
    """the index-exact contract on the locations in their own dtype -> h_low, w_low (int32), accepted (bool)"""
    h, w, mk = O.sample_index(np.asarray(shapes, np.int64), loc)
    return h, w, (mk & 1).astype(bool)


# ---- the cases the CPU and the GPU file share -------------------------------------------------------------------------------------------
def add_nonfinite(loc):
    """a few NaN / +-inf coordinates, as the existing tests add them (rejected by the acceptance test)"""
    flat = loc.reshape(-1)
    flat[5::3001] = np.nan
    flat[11::4001] = np.inf
    flat[12::5003] = -np.inf
    return loc


@functools.lru_cache(maxsize=None)
def make_case(shapes, M, D, P, B, Lq, variant, dtype="float32"):
    """-> dict of numpy arrays: value and grad_out randn, attw a softmax of randn (a uniform attw would hide a swapped point), loc the
    init state (``variant`` "init") or ``nudged`` of it ("nudged"), with a few non-finite coordinates; shapes, lsi"""
    dt = np.dtype(dtype).type
    tdt = torch.float32 if dt is np.float32 else torch.float64
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    loc = init_state_locations(shapes, M, P, B, Lq, tdt, seed=D + P)
    if variant == "nudged":
        loc = nudged(loc, 17 + D + P, shapes)
    else:
        assert variant == "init", variant
        loc = loc.copy()
    loc = add_nonfinite(loc)
    nq = loc.shape[1]
    rng = np.random.default_rng(1000 + 7 * D + P + M)
    value = rng.standard_normal((B, S, M, D)).astype(dt)
    go = rng.standard_normal((B, nq, M * D)).astype(dt)
    logits = rng.standard_normal((B, nq, M, L * P))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    attw = (e / e.sum(-1, keepdims=True)).reshape(B, nq, M, L, P).astype(dt)
    return dict(value=value, shapes=np.array(shapes, np.int64), lsi=O.level_start_index(shapes), loc=loc, attw=attw, go=go)


@functools.lru_cache(maxsize=None)
def reference(shapes, M, D, P, B, Lq, variant, dtype="float32"):
    """-> dict: h, w, ok (the cells of the case's locations in their own dtype), gv, gl, gw (fixed-cell fp64 autograd at those cells) and,
    for an fp32 case, rv32 / mag: the fp32 C oracle's grad_value and the same on absolute values (the sum of |terms|)"""
    g = make_case(shapes, M, D, P, B, Lq, variant, dtype)
    h, w, ok = cells(shapes, g["loc"])
    gv, gl, gw = fixed_cell_backward(g["value"], shapes, g["lsi"], g["loc"], g["attw"], g["go"], h, w, ok)
    r = dict(h=h, w=w, ok=ok, gv=gv, gl=gl, gw=gw)
    if dtype == "float32":
        r["rv32"] = O.backward(g["value"], g["shapes"], g["lsi"], g["loc"], g["attw"], g["go"])[0]
        r["mag"] = O.backward(np.abs(g["value"]), g["shapes"], g["lsi"], g["loc"], np.abs(g["attw"]), np.abs(g["go"]))[0]
    return r


def lattice_shares(shapes, loc):
    """-> (share of the finite points within 1e-4 px of a cell border, share whose fp32 and fp64 cells differ)"""
    fin = np.isfinite(loc).all(-1)
    l64 = np.nan_to_num(loc.astype(np.float64))
    near = np.zeros(loc.shape[:-1], bool)
    for l, (H, W) in enumerate(shapes):
        fy, fx = l64[:, :, :, l, :, 1] * H - 0.5, l64[:, :, :, l, :, 0] * W - 0.5
        near[:, :, :, l] = (np.abs(fy - np.round(fy)) < 1e-4) | (np.abs(fx - np.round(fx)) < 1e-4)
    h32, w32, ok32 = cells(shapes, loc)
    h64, w64, ok64 = cells(shapes, l64)
    flip = (ok32 != ok64) | (ok32 & ((h32 != h64) | (w32 != w64)))
    return float(near[fin].mean()), float(flip[fin].mean())


def check_point_gradients(got_gl, got_gw, ref, what, gl_tol=GL_TOL, gw_tol=GW_TOL):
    """grad_sampling_loc and grad_attn_weight against the fixed-cell reference at EVERY point; exact zeros at the rejected ones"""
    d_l, d_w = np.abs(got_gl - ref["gl"]), np.abs(got_gw - ref["gw"])
    print(f"{what}: grad_sampling_loc max err {d_l.max():.3g} (max |ref| {np.abs(ref['gl']).max():.3g}), grad_attn_weight max err {d_w.max():.3g}")
    dead = ~ref["ok"]
    assert (got_gl[dead] == 0).all() and (got_gw[dead] == 0).all(), f"{what}: a rejected or non-finite point has a gradient"
    np.testing.assert_allclose(got_gw, ref["gw"], err_msg=f"{what}: grad_attn_weight", **gw_tol)
    np.testing.assert_allclose(got_gl, ref["gl"], err_msg=f"{what}: grad_sampling_loc", **gl_tol)


def check_grad_value_f32(got_gv, ref, what):
    """per element against the fp32 oracle (same cells by the index-exact contract): only the order of the fp32 sums differs"""
    err = np.abs(got_gv - ref["rv32"])
    print(f"{what}: grad_value max err {err.max():.3g}, worst excess over 2^-18 mag + 1e-7: {(err - 2.0 ** -18 * ref['mag'] - 1e-7).max():.3g}")
    assert (err <= 2.0 ** -18 * ref["mag"] + 1e-7).all(), what
