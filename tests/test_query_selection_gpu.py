"""GPU: the native query selection (include/vllm_hip.h, section f2e) -- its three kernels alone, the whole module through the class switch
against the module's own fp64 run, an exact guarded workspace, offset views, a caller stream, and the routes that keep the composed path.

Bounds.
  Scores: bounds.assert_bound against fp64, |err| <= 1 bf16 ulp(ref) + 2^-17 sum_c |q text| of the winning token (the GEMM tests' bound: the
  score is one bf16 rounding of an fp32-accumulated dot product, and the maximum of near-equal tokens errs by no more than its terms do).
  Top-k: exact index equality with torch's stable descending sort on the CPU.
  Tail: validity flags are the bits of torch's fp32 statements.  Finite coords_logits: |err| <= 2^-17 (sum_c |h w| + |b|) + 2^-22 / (p (1 - p))
  + 2^-20 -- the project's GEMM term bound; the proposal p carries one fp32 division's relative error 2^-24 and 1 - p one more rounding, which
  log(p / (1 - p)) turns into at most 3 * 2^-24 / (p (1 - p)); 2^-20 is the roundings of the logf, of the two sums and of a result below 16.
  reference_points: a quarter of that (sigmoid's slope) + 2^-22, as the box-refine test judges its own.  Filled rows: +inf and 1.0 exactly.
  Whole module: the decoder tests' criterion, rel_rms(native) <= max(1.05 rel_rms(composed bf16), 4e-3), both against
  query_selection_inputs.reference (fp64, CPU) gathered at the NATIVE indices, on finite entries; +-inf positions are equal exactly; and the
  indices are exactly the stable-sort top-k of the native scores."""
import dataclasses

import pytest
import torch

from visionllm_amd import _lib
from visionllm_amd import query_selection as Q
from visionllm_amd.deformable_decoder import GroundingDinoMLPPredictionHead

import query_selection_inputs as I
import workspace_guard as G
from bounds import DEV, P, assert_bound, rel_rms, stream

pytestmark = pytest.mark.gpu


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def calls():
    return _lib.lib().vllm_query_select_calls()


# ---- the score kernel alone -------------------------------------------------------------------------------------------------------------------
def run_scores(q, text, tmask):
    B, S, C = q.shape
    out = torch.full((B, S), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().vllm_rowmax_dot_bf16(P(q), P(text), P(tmask), B, S, text.shape[1], C, P(out), stream()), "vllm_rowmax_dot_bf16")
    torch.cuda.synchronize()
    return out


def check_scores(B, S, Lt, C, seed, what):
    """image 0: the first token masked (Lt > 1); image 1: every token real; the last image: every token masked"""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, C, generator=g).to(torch.bfloat16)
    text = torch.randn(B, Lt, C, generator=g).to(torch.bfloat16)
    tmask = torch.ones(B, Lt, dtype=torch.bool)
    if Lt > 1:
        tmask[0, 0] = False
    tmask[B - 1] = False
    got = run_scores(q.to(DEV), text.to(DEV), tmask.to(torch.uint8).to(DEV))
    q64, t64 = q.double(), text.double()
    logits = (q64 @ t64.transpose(1, 2)).masked_fill(~tmask[:, None, :], float("-inf"))
    truth, win = logits.max(-1)
    mag = torch.gather(q64.abs() @ t64.abs().transpose(1, 2), 2, win[..., None])[..., 0]
    gc = got.cpu()
    assert torch.isinf(gc[B - 1]).all() and (gc[B - 1] < 0).all(), f"{what}: an all-masked image must score -inf everywhere"
    assert torch.isfinite(gc[:B - 1]).all(), what
    assert torch.equal(gc, gc.to(torch.bfloat16).float()), f"{what}: scores are bf16 values"
    assert_bound(gc[:B - 1], truth[:B - 1], mag[:B - 1], what)
    again = run_scores(q.to(DEV), text.to(DEV), tmask.to(torch.uint8).to(DEV))
    assert torch.equal(bits(again), bits(got)), f"{what}: two runs differ"


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("Lt", [1, 5, 256])
@pytest.mark.parametrize("S", [1, 37, 130])
def test_score_kernel_against_fp64(S, Lt, C):
    check_scores(3, S, Lt, C, S * 1000 + Lt * 10 + C, f"scores S {S} Lt {Lt} C {C}")


def test_score_kernel_walks_three_trips_with_a_ragged_last_one():
    """a workgroup walks its image's tiles of 128 rows, and two images share the compute units, cus / 2 workgroups each: cus + 1 tiles are
    three trips, the last one a single tile of 37 rows"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    check_scores(2, 128 * cus + 37, 5, 64, 77, f"scores over {cus} compute units")


def test_score_kernel_chunks_a_text_beyond_its_lds_budget_and_propagates_nan():
    check_scores(2, 70, 256, 512, 78, "scores C 512 Lt 256 (two chunks of the text)")
    g = torch.Generator().manual_seed(79)
    q = torch.randn(1, 40, 64, generator=g).to(torch.bfloat16)
    text = torch.randn(1, 5, 64, generator=g).to(torch.bfloat16)
    q[0, 3, 7] = float("nan")
    tmask = torch.ones(1, 5, dtype=torch.uint8)
    got = run_scores(q.to(DEV), text.to(DEV), tmask.to(DEV)).cpu()
    assert torch.isnan(got[0, 3]) and torch.isfinite(got[0, :3]).all() and torch.isfinite(got[0, 4:]).all()


# ---- the top-k kernel alone -------------------------------------------------------------------------------------------------------------------
def run_topk(scores, k):
    B, S = scores.shape
    out = torch.full((B, k), -1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().vllm_topk_rows_f32(P(scores), B, S, k, P(out), stream()), "vllm_topk_rows_f32")
    torch.cuda.synchronize()
    return out


def score_set(kind, S, g):
    if kind == "random":
        return torch.randn(2, S, generator=g)
    if kind == "four_values":          # heavy ties; -0.0 and 0.0 are one value
        return torch.tensor([0.0, -0.0, 1.5, -2.0, 0.25])[torch.randint(0, 5, (2, S), generator=g)]
    if kind == "all_equal":
        return torch.full((2, S), 0.375)
    if kind == "all_minus_inf":
        return torch.full((2, S), float("-inf"))
    s = torch.randn(2, S, generator=g).to(torch.bfloat16).float()          # bf16 values tie often
    for v in (float("inf"), float("nan"), float("-inf"), float("nan"), float("inf")):
        s[torch.randint(0, 2, (1,), generator=g), torch.randint(0, S, (1,), generator=g)] = v
    s[1, S - 1] = float("nan")
    return s


@pytest.mark.parametrize("kind", ["random", "four_values", "all_equal", "all_minus_inf", "inf_and_nan"])
@pytest.mark.parametrize("S", [1, 37, 1025, 4099])
def test_topk_kernel_is_the_stable_descending_sort(S, kind):
    g = torch.Generator().manual_seed(S * 10 + len(kind))
    scores = score_set(kind, S, g)
    dev = scores.to(DEV)
    for k in sorted({1, min(S, 900), min(S, 2048)} | ({S} if S <= 2048 else set())):
        got = run_topk(dev, k)
        want = I.stable_topk(scores, k)
        assert torch.equal(got.cpu(), want), f"top-k S {S} k {k} {kind}: first difference at {int((got.cpu() != want).flatten().nonzero()[0])}"
        assert torch.equal(run_topk(dev, k), got), f"top-k S {S} k {k} {kind}: two runs differ"


# ---- the tail kernel alone --------------------------------------------------------------------------------------------------------------------
def torch_valid_flags(padding_mask, maps):
    """the reference's fp32 statements (:2244-2266) on the device -> output_proposals_valid [B, S]"""
    B = padding_mask.shape[0]
    proposals, pos = [], 0
    for level, (height, width) in enumerate(maps):
        m = padding_mask[:, pos:pos + height * width].view(B, height, width, 1)
        valid_height = torch.sum(~m[:, :, 0, 0], 1)
        valid_width = torch.sum(~m[:, 0, :, 0], 1)
        grid_y, grid_x = torch.meshgrid(torch.linspace(0, height - 1, height, dtype=torch.float32, device=DEV),
                                        torch.linspace(0, width - 1, width, dtype=torch.float32, device=DEV), indexing="ij")
        grid = torch.cat([grid_x.unsqueeze(-1), grid_y.unsqueeze(-1)], -1)
        scale = torch.cat([valid_width.unsqueeze(-1), valid_height.unsqueeze(-1)], 1).view(B, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(B, -1, -1, -1) + 0.5) / scale
        width_heigth = torch.ones_like(grid) * 0.05 * (2.0**level)
        proposals.append(torch.cat((grid, width_heigth), -1).view(B, -1, 4))
        pos += height * width
    p = torch.cat(proposals, 1)
    return ((p > 0.01) & (p < 0.99)).all(-1)


def threshold_geometry():
    """maps whose extents reach 50 and 60 cells, so that proposals land on and around 0.01 and 0.99: (0.5 / 50, 49.5 / 50, 0.5 / 60, ...).
    Image 0 is unpadded, image 1 padded to 2 x 37 and 41 x 2."""
    maps = [(2, 50), (60, 3)]
    S = 100 + 180
    real = torch.ones(2, S, dtype=torch.bool)
    ys, xs = torch.meshgrid(torch.arange(2), torch.arange(50), indexing="ij")
    real[1, :100] = (xs < 37).flatten()
    ys, xs = torch.meshgrid(torch.arange(60), torch.arange(3), indexing="ij")
    real[1, 100:] = ((ys < 41) & (xs < 2)).flatten()
    return maps, real


@pytest.mark.parametrize("C", [64, 256])
@pytest.mark.parametrize("geometry", ["inputs", "thresholds"])
def test_tail_kernel_against_fp64(geometry, C):
    maps, real = (I.MAPS, I.real_mask()) if geometry == "inputs" else threshold_geometry()
    B, S = real.shape
    k = S          # every row of every level: the padded ones and the invalid ones too, in a shuffled order
    g = torch.Generator().manual_seed(C + len(geometry))
    idx = torch.stack([torch.randperm(S, generator=g) for _ in range(B)])
    parent = torch.randn(B * k, C + 16, generator=g).relu().to(torch.bfloat16).to(DEV)          # rows wider than C
    h = parent[:, 8:8 + C]
    W = (0.1 * torch.randn(4, C, generator=g)).to(torch.bfloat16).to(DEV)
    b = (0.1 * torch.randn(4, generator=g)).to(torch.bfloat16).to(DEV)
    assert h.data_ptr() % 16 == 0 and h.stride(0) == C + 16
    pmask = (~real).to(torch.uint8).to(DEV)
    shapes = torch.tensor(maps, dtype=torch.int64, device=DEV)
    hw = shapes[:, 0] * shapes[:, 1]
    lsi = torch.cumsum(hw, 0) - hw
    idx_dev = idx.to(DEV)
    what = f"tail {geometry} C {C}"

    def run():
        ext = torch.full((B, len(maps), 2), -7, dtype=torch.int32, device=DEV)
        coords = torch.full((B, k, 4), float("nan"), dtype=torch.float32, device=DEV)
        ref = torch.full((B, k, 4), float("nan"), dtype=torch.float32, device=DEV)
        valid = torch.full((B, k), 9, dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib().vllm_query_select_tail_f32(P(h), h.stride(0), P(W), P(b), P(idx_dev), P(pmask), P(shapes), P(lsi), B, S, len(maps), k,
                                                         C, P(ext), P(coords), P(ref), P(valid), stream()), "vllm_query_select_tail_f32")
        torch.cuda.synchronize()
        return ext, coords, ref, valid
    ext, coords, ref, valid = run()
    # extents: the counts of column 0 and row 0
    want_ext = torch.tensor([[[int(real[i, s0:s0 + H * Wd].view(H, Wd)[:, 0].sum()), int(real[i, s0:s0 + H * Wd].view(H, Wd)[0].sum())]
                              for (H, Wd), s0 in zip(maps, lsi.tolist())] for i in range(B)], dtype=torch.int32)
    assert torch.equal(ext.cpu(), want_ext), what
    # validity flags: torch's own fp32 statements, bit for bit
    flags = torch_valid_flags(~real.to(DEV), maps).cpu()
    assert torch.equal(valid.cpu().bool(), torch.gather(flags, 1, idx)), f"{what}: validity flags differ from torch's fp32 statements"
    if geometry == "thresholds":
        assert (~flags & real).any() and (flags & real).any()
    logit, _ = I.closed_form_proposals(real, maps)
    logit = torch.gather(logit, 1, idx[..., None].expand(-1, -1, 4))
    filled = torch.gather(~flags | ~real, 1, idx)
    assert filled.any() and (~filled).any() and (torch.gather(~real, 1, idx)).any() and (torch.gather(~flags & real, 1, idx)).any()
    cg, rg = coords.cpu(), ref.cpu()
    assert torch.equal(torch.isinf(cg), filled[..., None].expand(-1, -1, 4)) and (cg[filled] > 0).all(), f"{what}: +inf exactly at filled rows"
    assert (rg[filled] == 1.0).all(), f"{what}: sigmoid(+inf) is 1.0"
    h64, W64, b64 = h.double().cpu().view(B, k, C), W.double().cpu(), b.double().cpu()
    fin = ~filled
    z = (h64 @ W64.T + b64)[fin] + logit[fin]
    p = torch.sigmoid(logit[fin])
    bound = 2.0 ** -17 * (h64.abs() @ W64.abs().T + b64.abs())[fin] + 2.0 ** -22 / (p * (1 - p)) + 2.0 ** -20
    err = (cg[fin].double() - z).abs()
    rerr = (rg[fin].double() - torch.sigmoid(z)).abs()
    print(f"{what}: coords max |err| {err.max().item():.3e}, err / bound {(err / bound).max().item():.3f}; reference points err / bound "
          f"{(rerr / (0.25 * bound + 2.0 ** -22)).max().item():.3f}")
    assert torch.isfinite(cg[fin]).all() and (err <= bound).all(), what
    assert (rerr <= 0.25 * bound + 2.0 ** -22).all(), what
    for a, c in zip(run(), (ext, coords, ref, valid)):
        assert torch.equal(bits(a), bits(c)), f"{what}: two runs differ"


# ---- the whole module --------------------------------------------------------------------------------------------------------------------------
def judged(native, composed, truth, what):
    """the decoder tests' rule on the finite entries; +-inf positions equal exactly"""
    native, composed, truth = native.float().cpu(), composed.float().cpu(), truth.cpu()
    inf = torch.isinf(truth)
    assert torch.equal(torch.isinf(native), inf) and torch.equal(native[inf].double(), truth[inf].double()), f"{what}: +-inf positions differ"
    assert torch.equal(torch.isinf(composed), inf), f"{what}: the composed bf16 run's +-inf positions differ"
    assert torch.isfinite(native[~inf]).all() and (~inf).any()
    e, ec = rel_rms(native[~inf], truth[~inf]), rel_rms(composed[~inf], truth[~inf])
    print(f"{what}: rel rms native {e:.3e}, composed bf16 {ec:.3e}")
    assert e <= max(1.05 * ec, 4e-3), (what, e, ec)


def at(full, idx):
    return torch.gather(full.cpu(), 1, idx.cpu()[..., None].expand(-1, -1, full.shape[-1]))


@pytest.mark.parametrize("with_query_embeds", [False, True], ids=["gathered_target", "query_embeds"])
@pytest.mark.parametrize("k", I.KS)
def test_module_through_the_switch_against_its_own_fp64_run(k, with_query_embeds, monkeypatch):
    m = I.as_bf16(I.make_module(), DEV)
    t = I.to(I.make_inputs(), DEV)
    truth = I.reference()
    what = f"k {k} {'query_embeds' if with_query_embeds else 'gathered'}"
    with torch.no_grad():
        before = calls()
        composed = I.call(m, t, k, with_query_embeds)
        assert calls() == before and m.native_selection is False
        monkeypatch.setattr(Q.GroundingDinoQuerySelection, "native_selection", True)
        assert I.reasons(m, t, k, with_query_embeds) == []
        scores = torch.full((I.B, I.S), float("nan"), dtype=torch.float32, device=DEV)
        native = I.call(m, t, k, with_query_embeds, scores_out=scores)
        assert calls() == before + 1
        again = I.call(m, t, k, with_query_embeds)
        assert calls() == before + 2
    assert isinstance(native, Q.QuerySelectionOutput)
    assert native.enc_outputs_class is None and native.enc_outputs_coord_logits is None and native.object_query_embedding is None
    idx = native.topk_proposals
    assert idx.dtype == torch.int64 and idx.shape == (I.B, k)
    assert native.target.dtype == torch.bfloat16 and native.target.shape == (I.B, k, I.C)
    assert native.enc_topk_class_logits.dtype == torch.float32 and native.enc_topk_class_logits.shape == (I.B, k, I.MTL)
    assert native.enc_topk_coords_logits.dtype == torch.float32 and native.enc_topk_coords_logits.shape == (I.B, k, 4)
    assert native.reference_points.dtype == torch.float32 and native.reference_points is native.init_reference_points
    for f in dataclasses.fields(native):
        a, b = getattr(native, f.name), getattr(again, f.name)
        assert (a is None and b is None) or torch.equal(bits(a), bits(b)), f"{what}: two runs differ in {f.name}"
    # the scores the selection was made from, and the selection itself: exactly the stable-sort top-k of those scores
    judged(scores, composed.enc_outputs_class.max(-1)[0], truth.enc_outputs_class.max(-1)[0], f"{what} scores")
    assert torch.equal(idx.cpu(), I.stable_topk(scores, k)), f"{what}: topk_proposals is not the stable-sort top-k of the native scores"
    if k == I.S:
        assert torch.equal(idx.cpu().sort(-1).values, torch.arange(I.S).expand(I.B, -1))
    # everything else at the native indices
    if with_query_embeds:
        assert native.target_undetach is None and torch.equal(native.target, t["query_embeds"][:k][None].expand(I.B, -1, -1))
    else:
        assert native.target_undetach is not None and torch.equal(native.target, native.target_undetach)
        judged(native.target, at(composed.object_query_embedding, idx), at(truth.object_query_embedding, idx), f"{what} target")
    judged(native.enc_topk_class_logits, at(composed.enc_outputs_class, idx), at(truth.enc_outputs_class, idx), f"{what} class logits")
    judged(native.enc_topk_coords_logits, at(composed.enc_outputs_coord_logits, idx), at(truth.enc_outputs_coord_logits, idx), f"{what} coords logits")
    tc = at(truth.enc_outputs_coord_logits, idx)
    judged(native.reference_points, at(composed.enc_outputs_coord_logits, idx).sigmoid(), tc.sigmoid(), f"{what} reference points")
    assert (native.reference_points.cpu()[torch.isinf(tc)] == 1.0).all()
    if k == I.S:
        assert torch.isinf(tc).any()          # invalid and padded rows were selected


@pytest.mark.parametrize("fill", [G.HOSTILE, G.PLAUSIBLE], ids=["hostile", "plausible"])
def test_exact_workspace_with_guards(fill, monkeypatch):
    """The C entry with exactly the queried bytes, 16-byte aligned and no better, whatever they held: the bits of a clean run, guards intact."""
    m = I.as_bf16(I.make_module(), DEV)
    t = I.to(I.make_inputs(), DEV)
    monkeypatch.setattr(Q.GroundingDinoQuerySelection, "native_selection", True)
    with torch.no_grad():
        want = I.call(m, t, I.S)
    checks = []

    def exact(device, nbytes, what, slot=0):
        _lib.check(0 if nbytes >= 0 else -1, what)
        assert nbytes > 0 and what == "vllm_query_select_workspace_bytes"
        _, n, check = G.guarded(nbytes, fill, skew=16, widest_row_bytes=I.C * 2)
        checks.append(check)
        return check.workspace, n
    monkeypatch.setattr(_lib, "sized_workspace", exact)
    with torch.no_grad():
        before = calls()
        got = I.call(m, t, I.S)
        assert calls() == before + 1
    assert len(checks) == 1 and checks[0].workspace.data_ptr() % 32 == 16
    checks[0]()
    for f in dataclasses.fields(got):
        a, b = getattr(got, f.name), getattr(want, f.name)
        assert (a is None and b is None) or torch.equal(bits(a), bits(b)), f.name


def test_offset_views_and_a_caller_stream(monkeypatch):
    """inputs that are views 2 bytes (masks: 1 byte) into their parents, on a side stream: the same bits"""
    m = I.as_bf16(I.make_module(), DEV)
    t = I.to(I.make_inputs(), DEV)
    monkeypatch.setattr(Q.GroundingDinoQuerySelection, "native_selection", True)
    off = {}
    for key in ("memory", "text", "mask_flatten", "text_token_mask"):
        parent = torch.zeros(t[key].numel() + 8, dtype=t[key].dtype, device=DEV)
        parent[1:1 + t[key].numel()] = t[key].reshape(-1)
        off[key] = parent[1:1 + t[key].numel()].view_as(t[key])
        assert off[key].data_ptr() % 16 != 0
    with torch.no_grad():
        want = I.call(m, t, 9)
        before = calls()
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = I.call(m, dict(t, **off), 9)
        s.synchronize()
        assert calls() == before + 1
    for f in dataclasses.fields(got):
        a, b = getattr(got, f.name), getattr(want, f.name)
        assert (a is None and b is None) or torch.equal(bits(a), bits(b)), f.name


def test_routes_that_keep_the_composed_path(monkeypatch):
    t = I.to(I.make_inputs(), DEV)
    cls = Q.GroundingDinoQuerySelection

    def composed_only(m, tt, grad=False, **kw):
        """switch on: no native call, and the result of the switch off"""
        with torch.enable_grad() if grad else torch.no_grad():
            monkeypatch.setattr(cls, "native_selection", False)
            off = I.call(m, tt, 9, **kw)
            monkeypatch.setattr(cls, "native_selection", True)
            before = calls()
            assert I.reasons(m, tt, 9, **kw) != []
            on = I.call(m, tt, 9, **kw)
            assert calls() == before
        for f in dataclasses.fields(on):
            a, b = getattr(on, f.name), getattr(off, f.name)
            assert (a is None and b is None) or torch.equal(bits(a.detach()), bits(b.detach())), f.name
        assert on.enc_outputs_class is not None and on.enc_outputs_coord_logits is not None and on.object_query_embedding is not None
        return on

    m = I.as_bf16(I.make_module(), DEV)
    monkeypatch.setattr(cls, "native_selection", True)
    with torch.no_grad():
        before = calls()
        assert I.call(m, t, 9).enc_outputs_class is None
        assert calls() == before + 1                        # the baseline: this module and these inputs do take the native call
    full = composed_only(m, t, full_outputs=True)                            # a caller who asks for the full tensors
    assert full.enc_outputs_class.shape == (I.B, I.S, I.MTL)
    assert composed_only(m, t, grad=True).target_undetach.requires_grad      # grad enabled, trainable parameters
    m.train()
    composed_only(m, t)                                                      # training mode
    m.eval()
    f32 = I.make_module().to(DEV)
    assert composed_only(f32, I.to(I.make_inputs(), DEV, torch.float32)).target.dtype == torch.float32
    two = I.as_bf16(I.make_module(), DEV)
    two.encoder_output_bbox_embed = GroundingDinoMLPPredictionHead(I.C, I.C, 4, 2).to(DEV).to(torch.bfloat16)          # a two-layer head
    composed_only(two, t)
    short = I.as_bf16(I.make_module(), DEV)
    short.encoder_output_class_embed.max_text_len = 300                                                                  # beyond the kernel's 256 columns
    composed_only(short, t)
    with torch.no_grad():
        before = calls()
        I.call(m, t, 9)
        assert calls() == before + 1                        # and the module still takes the native call afterwards
