"""GPU: the native inputs of the Grounding-DINO encoder (include/vllm_hip.h, section f2h) -- the five new kernels alone (GroupNorm against
fp64 on the same bf16 input, the transpose against ``permute``, the patch matrix against ``F.unfold``, the mask pyramid against the
module's statements, the sine embedding against the module's statement on the CPU), and the whole module through its switch for both
memory formats and 1, 3, 4 and 5 levels, with a guarded workspace, offset views, a side stream, two runs, and the encoder taking the
outputs as they are.

No kernel of this section walks rows in a grid-stride loop (a thread's work is fixed by its index: csrc/gdino_inputs.hip), so there is
no multi-trip case here; the shapes below cover more than one workgroup, ragged tiles and slabs, and every path (the 16-byte and the
2-byte loads of the transpose)."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from visionllm_amd import _lib
from visionllm_amd import gdino_inputs as G

import gdino_inputs_inputs as I
from bounds import DEV, P, assert_bound, rel_rms, stream
from workspace_guard import HOSTILE, guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def randn(*shape, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (shift + scale * torch.randn(*shape, generator=g)).to(BF).to(DEV)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------------------
def groupnorm(x, gamma, beta, eps, B, HW, C, out, out_bs, ldo):
    """x: a 2-d view [B HW, C] (row stride = ldx); out: the tensor whose data pointer is the first output row"""
    L = _lib.lib()
    need = L.vllm_groupnorm_rows_workspace_bytes(B, HW, C)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    _lib.check(L.vllm_groupnorm_rows_bf16(P(x), x.stride(0), P(gamma), P(beta), eps, B, HW, C, P(out), out_bs, ldo, P(ws), need, stream()),
               "vllm_groupnorm_rows_bf16")


def groupnorm_ref(x, gamma, beta, eps, B, HW, C):
    """fp64 on the same bf16 values -> (reference [B, HW, C], the bound's magnitude |gamma| (|x| + |mean|) / std + |beta|)"""
    xd = x.double().cpu().reshape(B, HW, 32, C // 32)
    mean = xd.mean(dim=(1, 3), keepdim=True)
    var = (xd - mean).pow(2).mean(dim=(1, 3), keepdim=True)
    std = (var + eps).sqrt()
    g, b = gamma.double().cpu().view(1, 1, 32, -1), beta.double().cpu().view(1, 1, 32, -1)
    ref = (xd - mean) / std * g + b
    mag = g.abs() * (xd.abs() + mean.abs()) / std + b.abs()
    return ref.reshape(B, HW, C), mag.reshape(B, HW, C)


@pytest.mark.parametrize("C", [64, 256, 512])
def test_groupnorm_against_fp64(C):
    """2, 8 and 16 channels per group; one row, 35 rows (two slabs, the second ragged) and 70 rows (three slabs, the last ragged).  The
    bound is the project's: one bf16 ulp of the reference + 2^-17 of the summed magnitudes.  The fp32 statistics stay inside it: a group
    has at most 70 x 16 = 1120 elements, summed in slabs of at most 512 and combined pairwise, an error of a few 2^-24 of the mean."""
    B, eps = 2, 1e-5
    gamma, beta = randn(C, seed=1, scale=0.3, shift=1.0), randn(C, seed=2, scale=0.5)
    for HW in (1, 35, 70):
        x = randn(B * HW, C, seed=10 + HW, scale=1.5, shift=0.25)
        out = torch.full((B, HW, C), float("nan"), dtype=BF, device=DEV)
        groupnorm(x, gamma, beta, eps, B, HW, C, out, HW * C, C)
        ref, mag = groupnorm_ref(x, gamma, beta, eps, B, HW, C)
        assert_bound(out.cpu(), ref, mag, f"groupnorm C={C} HW={HW}")
    # a constant map, and one row whose groups are constant: x - mean is exactly 0, so the output is beta exactly
    x = torch.full((B * 35, C), 1.375, dtype=BF, device=DEV)
    out = torch.empty((B, 35, C), dtype=BF, device=DEV)
    groupnorm(x, gamma, beta, eps, B, 35, C, out, 35 * C, C)
    assert torch.equal(out, beta.view(1, 1, C).expand(B, 35, C)), "a constant map must give beta exactly"
    x1 = randn(B, 32, seed=5).repeat_interleave(C // 32, dim=1).contiguous()          # one row, every group constant
    out1 = torch.empty((B, 1, C), dtype=BF, device=DEV)
    groupnorm(x1, gamma, beta, eps, B, 1, C, out1, C, C)
    assert torch.equal(out1, beta.view(1, 1, C).expand(B, 1, C)), "HW == 1 with constant groups must give beta exactly"


def test_groupnorm_cancellation_strides_and_row_offset():
    C, B, HW, eps = 256, 2, 70, 1e-5
    gamma, beta = randn(C, seed=1, scale=0.3, shift=1.0), randn(C, seed=2, scale=0.5)
    # mean 32, sigma 1: E[x^2] - E[x]^2 would lose the variance's digits in fp32; bf16 values near 32 are 0.25 apart
    x = randn(B * HW, C, seed=3, scale=1.0, shift=32.0)
    out = torch.empty((B, HW, C), dtype=BF, device=DEV)
    groupnorm(x, gamma, beta, eps, B, HW, C, out, HW * C, C)
    ref, mag = groupnorm_ref(x, gamma, beta, eps, B, HW, C)
    assert_bound(out.cpu(), ref, mag, "groupnorm mean 32 sigma 1")
    # a row-strided input (columns 64 .. 64 + C of a wider tensor) and an output at row offset 11 of a wider NaN-prefilled parent
    wide = randn(B * HW, C + 128, seed=4, scale=1.5)
    xs = wide[:, 64:64 + C]
    S, off = HW + 30, 11
    parent = torch.full((B, S, C), float("nan"), dtype=BF, device=DEV)
    groupnorm(xs, gamma, beta, eps, B, HW, C, parent[:, off:], S * C, C)
    ref, mag = groupnorm_ref(xs, gamma, beta, eps, B, HW, C)
    assert_bound(parent[:, off:off + HW].cpu(), ref, mag, "groupnorm strided input, offset output")
    assert bool(parent[:, :off].isnan().all()) and bool(parent[:, off + HW:].isnan().all()), "rows outside the level were written"
    dense = torch.empty((B, HW, C), dtype=BF, device=DEV)
    groupnorm(xs.contiguous(), gamma, beta, eps, B, HW, C, dense, HW * C, C)
    assert torch.equal(dense, parent[:, off:off + HW]), "the strides changed the bits"


# ---- the transpose ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", [64, 192])
def test_transpose_equals_permute(Cin):
    """one pixel; 35 (one ragged tile, 2-byte loads); 130 (past a tile, 2-byte loads); 136 (past a tile, 16-byte loads); Cin 192 is three
    channel tiles; an offset view (8 elements: the least alignment the entry takes)"""
    L = _lib.lib()
    B = 2
    for HW in (1, 35, 130, 136):
        store = randn(8 + B * Cin * HW, seed=HW)
        for x in (store[:B * Cin * HW].view(B, Cin, HW), store[8:].view(B, Cin, HW)):
            out = torch.full((B * HW, Cin + 8), float("nan"), dtype=BF, device=DEV)
            _lib.check(L.vllm_nchw_to_rows_bf16(P(x), B, Cin, HW, P(out), Cin + 8, stream()), "vllm_nchw_to_rows_bf16")
            assert torch.equal(out[:, :Cin], x.permute(0, 2, 1).reshape(B * HW, Cin)), (Cin, HW)
            assert bool(out[:, Cin:].isnan().all())


# ---- im2col ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (2, 2), (5, 7), (8, 8)])
def test_im2col_equals_unfold(size):
    L = _lib.lib()
    B, Cin = 2, 64
    Hi, Wi = size
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    nchw = randn(B, Cin, Hi, Wi, seed=Hi * 10 + Wi)
    unf = F.unfold(nchw.float(), 3, padding=1, stride=2)                                  # [B, Cin 9, Ho Wo] in (c, ky, kx) order
    want = unf.view(B, Cin, 3, 3, Ho * Wo).permute(0, 4, 2, 3, 1).reshape(B * Ho * Wo, 9 * Cin).to(BF)
    rows = nchw.permute(0, 2, 3, 1).reshape(B, Hi * Wi, Cin).contiguous()
    wide = torch.full((B, Hi * Wi + 3, Cin + 64), float("nan"), dtype=BF, device=DEV)     # a level's rows inside a wider [B, S, C']
    wide[:, 2:2 + Hi * Wi, 32:32 + Cin] = rows
    for src, bs, ld in ((rows, Hi * Wi * Cin, Cin), (wide[:, 2:, 32:], wide.stride(0), wide.stride(1))):
        out = torch.full((B * Ho * Wo, 9 * Cin), float("nan"), dtype=BF, device=DEV)
        _lib.check(L.vllm_im2col3x3s2_bf16(P(src), bs, ld, B, Hi, Wi, Cin, P(out), stream()), "vllm_im2col3x3s2_bf16")
        assert torch.equal(out, want), (size, ld)


# ---- the mask pyramid and the sine embedding ---------------------------------------------------------------------------------------------------------
def five_masks():
    """the golden's two images, an all-valid image, an image with one valid column, a fully masked image"""
    m = torch.zeros((5,) + I.MASK_SIZE, dtype=torch.int64)
    m[:2] = I.pixel_mask()
    m[2] = 1
    m[3, :, 0] = 1
    return m


def mask_levels(pm, sizes):
    L = _lib.lib()
    B, H, W = pm.shape
    S = sum(h * w for h, w in sizes)
    om = torch.full((B, S), 7, dtype=torch.uint8, device=DEV)
    yc, xc = torch.full((B, S), -1, dtype=torch.int32, device=DEV), torch.full((B, S), -1, dtype=torch.int32, device=DEV)
    vr = torch.full((B, len(sizes), 2), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(L.vllm_pixel_mask_levels_u8(P(pm), pm.element_size(), B, H, W, ints(*(h for h, _ in sizes)), ints(*(w for _, w in sizes)), len(sizes),
                                           P(om), P(yc), P(xc), P(vr), stream()), "vllm_pixel_mask_levels_u8")
    return om, yc, xc, vr


@pytest.fixture(scope="module")
def mask_statements():
    """the module's statements on the device for five_masks(): masks, cumsums, valid_ratios per level"""
    m = I.make_module(dtype=torch.float32)
    pm = five_masks().to(DEV)
    masks = [m.downsample_mask(pm, s) for s in I.LEVEL_SIZES]
    return dict(mask=torch.cat([x.flatten(1) for x in masks], 1),
                ycnt=torch.cat([x.cumsum(1, dtype=torch.float32).flatten(1) for x in masks], 1),
                xcnt=torch.cat([x.cumsum(2, dtype=torch.float32).flatten(1) for x in masks], 1),
                vr=torch.stack([m.get_valid_ratio(x) for x in masks], 1).float(), masks=masks)


@pytest.mark.parametrize("dtype", [torch.int64, torch.bool, torch.uint8])
def test_mask_kernel_equals_the_modules_statements(mask_statements, dtype):
    """29 x 19 -> 7 x 5, 4 x 3, 2 x 2, 1 x 1: no size divides"""
    pm = five_masks().to(dtype).to(DEV)
    om, yc, xc, vr = mask_levels(pm, I.LEVEL_SIZES)
    want = mask_statements
    assert torch.equal(om.bool(), want["mask"]) and bool((om <= 1).all())
    assert torch.equal(yc.float(), want["ycnt"]) and torch.equal(xc.float(), want["xcnt"])
    print("valid_ratios", vr.flatten().tolist(), want["vr"].flatten().tolist())
    assert torch.equal(vr, want["vr"])
    assert float(vr[2].min()) > 0.99 and float(vr[4].max()) == 0 and float(vr[3, 0, 0]) == pytest.approx(0.2)


def test_sine_embedding_against_the_modules_statement(mask_statements):
    """against GroundingDinoSinePositionEmbedding.forward evaluated in fp32 on the CPU + level_embed, under the project's bound with
    magnitude 1 + |level_embed|; the fully masked image is 0 / (0 + 1e-6) in every cell"""
    L = _lib.lib()
    C, B = 64, 5
    pe = G.GroundingDinoSinePositionEmbedding(C // 2, I.TEMPERATURE, normalize=True)
    level_embed = randn(len(I.LEVEL_SIZES), C, seed=9)
    pm = five_masks().to(DEV)
    _, yc, xc, _ = mask_levels(pm, I.LEVEL_SIZES)
    S = yc.shape[1]
    out = torch.full((B, S, C), float("nan"), dtype=BF, device=DEV)
    dim_t = pe.dim_t(DEV).contiguous()
    _lib.check(L.vllm_sine_pos_embed_rows_bf16(P(yc), P(xc), ints(*(h for h, _ in I.LEVEL_SIZES)), ints(*(w for _, w in I.LEVEL_SIZES)),
                                               len(I.LEVEL_SIZES), B, C, P(level_embed), P(dim_t), P(out), stream()), "vllm_sine_pos_embed_rows_bf16")
    refs, mags = [], []
    for l, mask in enumerate(mask_statements["masks"]):
        pos = pe(torch.empty(1), mask.cpu())                                               # [B, C, h, w] fp32
        le = level_embed[l].double().cpu().view(1, 1, C)
        refs.append(pos.flatten(2).transpose(1, 2).double() + le)
        mags.append((1 + le.abs()).expand(B, pos.shape[2] * pos.shape[3], C))
    ref, mag = torch.cat(refs, 1), torch.cat(mags, 1)
    assert_bound(out.cpu(), ref, mag, "sine position embedding + level_embed")
    assert bool(out.isfinite().all())
    masked = out[4].float().cpu()                                                          # sin(0) + le on even channels, cos(0) + le on odd ones
    want = torch.cat([(torch.arange(C) % 2).float().view(1, C) + level_embed[l].float().cpu().view(1, C).expand(h * w, C)
                      for l, (h, w) in enumerate(I.LEVEL_SIZES)]).to(BF).float()
    assert torch.equal(masked, want)


# ---- the whole module through the switch ---------------------------------------------------------------------------------------------------------------
CASES = {1: ((128,), ((7, 5),)), 3: ((64, 128, 192), ((7, 5), (4, 3), (3, 2))), 4: (I.IN_CHANNELS, I.MAP_SIZES), 5: ((64, 128, 192), ((7, 5), (4, 3), (3, 2)))}


def build(n_levels):
    """-> (fp64 module on the CPU, its bf16 copy on the GPU, fp64 maps, level sizes, depth of each level in the conv chain)"""
    in_channels, sizes = CASES[n_levels]
    m64 = I.make_module(n_levels, in_channels, I.D_MODEL, seed=40 + n_levels)
    mbf = copy.deepcopy(m64).to(BF).to(DEV).eval()
    for p in mbf.parameters():
        p.requires_grad_(False)
    maps = I.make_maps(sizes, in_channels, seed=50 + n_levels)
    extra = I.extra_sizes(sizes[-1], n_levels - len(sizes))
    depth = [1] * len(sizes) + [2 + i for i in range(len(extra))]
    return m64, mbf, maps, list(sizes) + extra, depth


def on_gpu(maps, fmt):
    maps = [m.to(BF).to(DEV) for m in maps]
    return [m.contiguous(memory_format=torch.channels_last) for m in maps] if fmt == "channels_last" else maps


def run(m, maps, pm, native):
    m.native_inputs = native
    before = _lib.lib().vllm_gdino_inputs_calls()
    with torch.no_grad():
        out = m(maps, pm)
    assert _lib.lib().vllm_gdino_inputs_calls() - before == (1 if native else 0), m.native_inputs_reasons(maps, pm)
    m.native_inputs = False
    return out


@pytest.mark.parametrize("fmt", ["nchw", "channels_last"])
@pytest.mark.parametrize("n_levels", [1, 3, 4, 5])
def test_module_through_the_switch(n_levels, fmt):
    m64, mbf, maps64, sizes, depth = build(n_levels)
    pm = I.pixel_mask().to(DEV)
    maps = on_gpu(maps64, fmt)
    assert mbf.native_inputs_reasons(maps, pm) == []
    with torch.no_grad():
        ref = m64(maps64, I.pixel_mask())
    composed, native = run(mbf, maps, pm, False), run(mbf, maps, pm, True)
    for name in ("mask_flatten", "spatial_shapes", "level_start_index", "valid_ratios"):
        got, want = getattr(native, name), getattr(composed, name)
        assert got.dtype == want.dtype and got.device == want.device and torch.equal(got, want), name
    assert native.spatial_shapes.tolist() == [list(s) for s in sizes]
    start = 0
    for level, ((h, w), n) in enumerate(zip(sizes, depth)):
        sl = slice(start, start + h * w)
        for name in ("source_flatten", "lvl_pos_embed_flatten"):
            r = getattr(ref, name)[:, sl]
            e_native, e_composed = rel_rms(getattr(native, name)[:, sl].cpu(), r), rel_rms(getattr(composed, name)[:, sl].cpu(), r)
            print(f"levels {n_levels} {fmt} level {level} {name}: native {e_native:.3e} composed {e_composed:.3e}")
            assert e_native <= max(1.05 * e_composed, 4e-3 * n), (level, name, e_native, e_composed)
        start += h * w
    again = run(mbf, maps, pm, True)
    for name in ("source_flatten", "lvl_pos_embed_flatten", "mask_flatten", "valid_ratios"):
        assert torch.equal(getattr(again, name), getattr(native, name)), f"{name}: two runs differ"


def native_call(m, maps, pm, ws_ptr, ws_bytes):
    """vllm_gdino_inputs_forward on the module's own descriptor with the caller's workspace -> (source, pos, mask, valid_ratios)"""
    L = _lib.lib()
    d = m._native_state(pm.device)["desc"]
    n = d.n_maps
    B, H, W = pm.shape
    sizes = [(x.shape[2], x.shape[3]) for x in maps]
    sizes += I.extra_sizes(sizes[-1], d.n_levels - n)
    S, C = sum(h * w for h, w in sizes), d.d_model
    out = (torch.empty((B, S, C), dtype=BF, device=DEV), torch.empty((B, S, C), dtype=BF, device=DEV),
           torch.empty((B, S), dtype=torch.bool, device=DEV), torch.empty((B, d.n_levels, 2), dtype=torch.float32, device=DEV))
    ptrs = (ctypes.c_void_p * n)(*(x.data_ptr() for x in maps))
    h, w, f = ints(*(x.shape[2] for x in maps)), ints(*(x.shape[3] for x in maps)), ints(*(G._map_format(x) for x in maps))
    need = L.vllm_gdino_inputs_workspace_bytes(ctypes.byref(d), B, h, w, f)
    assert need == ws_bytes or ws_bytes is None
    _lib.check(L.vllm_gdino_inputs_forward(ctypes.byref(d), ptrs, h, w, f, P(pm), pm.element_size(), B, H, W, P(out[0]), P(out[1]), P(out[2]), P(out[3]),
                                           ctypes.c_void_p(ws_ptr), need, stream()), "vllm_gdino_inputs_forward")
    return out, need


@pytest.mark.parametrize("fmt", ["nchw", "channels_last"])
def test_exact_guarded_workspace(fmt):
    """exactly the bytes the query answers, 16-byte aligned and no better, NaN-filled, between guard bytes: the bits of a clean run"""
    _, mbf, maps64, _, _ = build(4)
    pm = I.pixel_mask().to(DEV)
    maps = on_gpu(maps64, fmt)
    clean = run(mbf, maps, pm, True)
    L = _lib.lib()
    d = mbf._native_state(pm.device)["desc"]
    need = L.vllm_gdino_inputs_workspace_bytes(ctypes.byref(d), pm.shape[0], ints(*(x.shape[2] for x in maps)), ints(*(x.shape[3] for x in maps)),
                                               ints(*(G._map_format(x) for x in maps)))
    ptr, nbytes, check = guarded(need, HOSTILE, skew=16, widest_row_bytes=9 * 128 * 2)
    (source, pos, mask, vr), _ = native_call(mbf, maps, pm, ptr, nbytes)
    check()
    assert torch.equal(source, clean.source_flatten) and torch.equal(pos, clean.lvl_pos_embed_flatten)
    assert torch.equal(mask, clean.mask_flatten) and torch.equal(vr, clean.valid_ratios)


def test_offset_views_a_side_stream_and_mask_dtypes():
    _, mbf, maps64, _, _ = build(4)
    pm = I.pixel_mask().to(DEV)
    clean = {fmt: run(mbf, on_gpu(maps64, fmt), pm, True) for fmt in ("nchw", "channels_last")}

    def same(out, fmt, what):
        for name in ("source_flatten", "lvl_pos_embed_flatten", "mask_flatten", "valid_ratios"):
            assert torch.equal(getattr(out, name), getattr(clean[fmt], name)), (what, fmt, name)

    for fmt in ("nchw", "channels_last"):
        for shift in (1, 8):          # batch-offset views whose data pointer is 2 bytes / 16 bytes past an aligned address
            views = []
            for x in on_gpu(maps64, fmt):
                store = torch.zeros(shift + x.numel(), dtype=BF, device=DEV)
                v = store[shift:].as_strided(x.shape, x.stride())
                v.copy_(x)
                assert G._map_format(v) == G._map_format(x) and v.data_ptr() % 16 == (2 * shift) % 16
                views.append(v)
            pmv = torch.zeros((pm.shape[0] + 1,) + tuple(pm.shape[1:]), dtype=pm.dtype, device=DEV)[1:]
            pmv.copy_(pm)
            assert mbf.native_inputs_reasons(views, pmv) == []
            same(run(mbf, views, pmv, True), fmt, f"offset views, shift {shift}")
        for dt in (torch.bool, torch.uint8):
            same(run(mbf, on_gpu(maps64, fmt), pm.to(dt), True), fmt, str(dt))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = run(mbf, on_gpu(maps64, "nchw"), pm, True)
    side.synchronize()
    same(out, "nchw", "side stream")
    # a non-contiguous pixel mask is made contiguous by the binding; arbitrary map strides keep the composed path
    wide_pm = torch.zeros((pm.shape[0], pm.shape[1], pm.shape[2] + 3), dtype=pm.dtype, device=DEV)
    wide_pm[:, :, :pm.shape[2]] = pm
    same(run(mbf, on_gpu(maps64, "nchw"), wide_pm[:, :, :pm.shape[2]], True), "nchw", "strided pixel mask")
    bad = [x.transpose(2, 3).contiguous().transpose(2, 3) for x in on_gpu(maps64, "nchw")]
    assert any("arbitrary strides are not" in r for r in mbf.native_inputs_reasons(bad, pm))


def test_encoder_takes_the_native_outputs_as_they_are():
    """GroundingDinoEncoder.native_encoder_reasons is empty on the native outputs: the two calls chain with no copy in between"""
    import gdino_encoder_inputs as E
    c = E.CONFIGS["a"]
    enc = E.as_bf16(E.make_encoder("a"), DEV)
    for p in enc.parameters():
        p.requires_grad_(False)
    t = E.to(E.make_inputs("a", 5), DEV)
    m = copy.deepcopy(I.make_module(len(c["maps"]), (64, 128), c["C"], seed=60)).to(BF).to(DEV).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    maps = on_gpu(I.make_maps(c["maps"], (64, 128), batch=c["B"], seed=61), "channels_last")
    pm = torch.ones((c["B"], 23, 17), dtype=torch.bool, device=DEV)
    pm[1, :, 12:] = False
    out = run(m, maps, pm, True)
    why = enc.native_encoder_reasons(out.source_flatten, ~out.mask_flatten, out.lvl_pos_embed_flatten, out.spatial_shapes, out.level_start_index,
                                     out.valid_ratios, t["text"], t["text_mask"], None, t["text_self_attention_masks"], t["text_position_ids"])
    assert why == []
    assert out.source_flatten.data_ptr() % 16 == 0 and out.lvl_pos_embed_flatten.data_ptr() % 16 == 0 and out.source_flatten.is_contiguous()
