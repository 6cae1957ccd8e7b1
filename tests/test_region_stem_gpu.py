"""GPU: the native region-encoder route (RegionEncoder.native_branch; vllm_region_encoder_forward / _backward and their building blocks)
at the smallest shapes at which each kernel can still go wrong.  Inputs and fp64 references: region_stem_inputs.py."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

import region_stem_inputs as I
import region_train_inputs as RT
import test_region_train_gpu as TR
import test_workspace_contract_gpu as WC
from bounds import P, assert_bound, bf16_ulp, rel_rms, stream
from visionllm_amd import _lib
from visionllm_amd import region_encoder as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
bf = lambda t: t.to(torch.bfloat16)  # noqa: E731


def nan_bf16(*shape):
    return torch.full(shape, NAN, device=DEV).to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- im2col ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("patch,H,W,kpad", [(14, 56, 84, 256), (16, 64, 96, 256)], ids=["patch14", "patch16"])
def test_im2col_equals_the_unfold_restatement(patch, H, W, kpad, dtype):
    """Two images, not square (a transposed row order shows); patch 14: 196 live columns and 60 exact-zero pad columns, patch 16: 256
    and none (64 x 96 there: 56 x 84 is no multiple of 16).  Output prefilled with NaN: every element is written, bit for bit."""
    gen = torch.Generator().manual_seed(patch)
    images = torch.randn(2, 3, H, W, generator=gen).to(dtype)
    masks = (torch.rand(2, 1, H, W, generator=gen) > 0.5).to(dtype)
    ref = I.im2col_ref(images, masks, patch, kpad)
    rows = 2 * (2 * H // patch) * (2 * W // patch)
    out = nan_bf16(rows, kpad)
    im, mk = images.to(DEV), masks.to(DEV)
    _lib.check(_lib.lib().vllm_region_im2col_bf16(P(im), P(mk), int(dtype == torch.float32), P(out), 2, H, W, patch, kpad, stream()), "im2col")
    torch.cuda.synchronize()
    assert ref.shape == out.shape
    assert torch.equal(bits(out.cpu()), bits(ref))
    assert torch.equal(bits(out[:, patch * patch:].cpu()), torch.zeros(rows, kpad - patch * patch, dtype=torch.int16))


# ---- LayerNorm + GELU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 96 * 7 + 5])
@pytest.mark.parametrize("C", [64, 256])
def test_layernorm_gelu_on_short_rows(C, rows):
    """pre against fp64 of LayerNorm2d's statements by vllm_layernorm_bf16's bound (test_vit_gpu.test_norms: one rounding of an fp32
    evaluation, 1 bf16 ulp + 2^-20 (|n w| + |b|)); y within 1 bf16 ulp of the fp64 GELU of the STORED pre; with pre_out = NULL the same y
    bits.  The input is an offset view (row stride C + 16, 16 bytes into its parent); 96 * 7 + 5 rows leave the last wave's row group
    ragged at both widths (8 rows per wave at C = 64, 2 at C = 256)."""
    torch.manual_seed(C + rows)
    parent = bf(torch.randn(rows, C + 16, device=DEV) * 2 + 0.3)
    x = parent[:, 8:8 + C]
    assert x.data_ptr() % 16 == 0 and x.data_ptr() != parent.data_ptr()
    w, b = bf(1 + 0.2 * torch.randn(C, device=DEV)), bf(0.1 * torch.randn(C, device=DEV))
    pre, y, y2 = nan_bf16(rows, C), nan_bf16(rows, C), nan_bf16(rows, C)
    L = _lib.lib()
    _lib.check(L.vllm_layernorm_gelu_bf16(P(x), C + 16, P(w), P(b), P(pre), P(y), rows, C, 1e-6, stream()), "layernorm_gelu")
    _lib.check(L.vllm_layernorm_gelu_bf16(P(x), C + 16, P(w), P(b), None, P(y2), rows, C, 1e-6, stream()), "layernorm_gelu")
    torch.cuda.synchronize()
    xd, wd, bd = x.double().cpu(), w.double().cpu(), b.double().cpu()
    ref_pre, _ = I.ln_gelu_ref(xd, wd, bd, 1e-6)
    nw = (ref_pre - bd).abs()
    err = (pre.double().cpu() - ref_pre).abs()
    u = ((err - 2.0 ** -20 * (nw + bd.abs())).clamp_min(0) / bf16_ulp(ref_pre)).max().item()
    print(f"layernorm_gelu C{C} rows{rows}: pre max excess {u:.3f} bf16 ulp")
    assert u <= 1.0
    ref_y = F.gelu(pre.double().cpu())
    uy = ((y.double().cpu() - ref_y).abs() / bf16_ulp(ref_y)).max().item()
    print(f"layernorm_gelu C{C} rows{rows}: y against gelu(stored pre) {uy:.3f} bf16 ulp")
    assert uy <= 1.0
    assert torch.equal(bits(y2), bits(y))


# ---- pooling weights ------------------------------------------------------------------------------------------------------------------------
def _weights(coords, valid, h, w):
    L_, n, Pn = valid.shape
    c, v = coords.to(DEV).contiguous(), valid.to(torch.uint8).to(DEV).contiguous()
    out = torch.full((L_, n, h * w), NAN, device=DEV)
    _lib.check(_lib.lib().vllm_region_pool_weights_f32(P(c), P(v), P(out), n, L_, h, w, Pn, stream()), "region_pool_weights")
    torch.cuda.synchronize()
    return out


def _weight_bound(coords, valid, h, w):
    """One level's A / cnt against fp64 (region_train_inputs.mean_bound with grad_out = 1): 4 * 2^-24 |ref| + (d + 2^-40) hits / cnt."""
    L_, n, Pn = valid.shape
    out = []
    for l in range(L_):
        hits = RT.scatter_per_pixel(torch.ones(n, 1, Pn), coords[l], h, w, select=valid[l])[:, 0]
        out.append((RT.weight_error(h, w) + 2.0 ** -40) * hits / valid[l].sum(1).clamp(min=1).double()[:, None])
    return torch.stack(out)


@pytest.mark.parametrize("h,w", [(4, 6), (24, 24)])
def test_pool_weights_one_level_are_the_masked_means(h, w):
    """L = 1: w_0 = A_0 / cnt_0, the weights of vllm_point_sample_mean_*: bit for bit what the existing backward writes for grad_out = 1,
    and inside the existing bound against fp64; exact zeros for the region without a valid point."""
    n, Pn = 3, 37
    coords, valid = I.make_points(1, n, Pn, h, w, 7 * h, short=1, empty=2)
    got = _weights(coords, valid, h, w)
    ones = torch.ones(n, 1)
    old = TR._mean_abi(coords[0], valid[0], ones, 1, h, w, torch.full((n, 1, h, w), NAN, device=DEV))
    assert torch.equal(got[0], old.reshape(n, h * w))
    ref = I.pool_weights_ref(coords, valid, h, w)
    bound = 4 * RT.EPS * ref.abs() + _weight_bound(coords, valid, h, w)
    err = (got.double().cpu() - ref).abs()
    print(f"pool weights L=1 {h}x{w}: max |err| {err.max().item():.3e}, max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert (err <= bound).all()
    assert torch.equal(got[0, 2], torch.zeros(h * w, device=DEV))


def test_pool_weights_follow_the_suffix_rule():
    """L = 3: w_k = ((A_2 / cnt_2 + A_1 / cnt_1) + ... + A_k / cnt_k) / 3 in exactly that fp32 order from the one-level weights, and inside
    the summed bound against fp64."""
    n, Pn, h, w = 3, 37, 4, 6
    coords, valid = I.make_points(3, n, Pn, h, w, 5, short=1, empty=2)
    valid[1, 0] = False                                          # one level of a live region without a point: it adds 0
    got = _weights(coords, valid, h, w)
    single = [_weights(coords[l:l + 1], valid[l:l + 1], h, w)[0] for l in range(3)]
    run, three = torch.zeros_like(single[0]), torch.full_like(single[0], 3.0)   # (a tensor divisor: a true division, no reciprocal multiply)
    for k in (2, 1, 0):
        run = run + single[k]
        assert torch.equal(got[k], run / three), k
    assert torch.equal(single[1][0], torch.zeros(h * w, device=DEV))
    ref = I.pool_weights_ref(coords, valid, h, w)
    per_level = _weight_bound(coords, valid, h, w) + 4 * RT.EPS * I.level_weights_ref(coords, valid, h, w).abs()
    bound = per_level.flip(0).cumsum(0).flip(0) / 3 + 6 * RT.EPS * ref.abs()
    err = (got.double().cpu() - ref).abs()
    print(f"pool weights L=3: max |err| {err.max().item():.3e}, max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
    assert (err <= bound).all()


# ---- fused pooling and outer product --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(4, 6), (24, 24)])
@pytest.mark.parametrize("C", [64, 192])
def test_fused_pooling_and_outer_product(C, h, w):
    """Three levels given as hidden[:, 1:] views of [n, 1 + T, C] tensors (their own row and image strides, never copied), P = 37, region 1
    with fewer valid points than P, region 2 with none.  Pooling: tests/bounds.assert_bound against fp64 of sum w x with the kernel's own
    fp32 weights, magnitude sum |w x|; a NaN in the empty region's data does not get through its zero weights.  Outer product: each element
    within 1 bf16 ulp of fp64, every element written (NaN prefill), two runs bit-identical."""
    n, Pn, L_, T = 3, 37, 3, h * w
    coords, valid = I.make_points(L_, n, Pn, h, w, C + h, short=1, empty=2)
    wk = _weights(coords, valid, h, w)
    torch.manual_seed(C * h)
    stem = bf(torch.randn(n, T, C, device=DEV))
    hidden = [bf(torch.randn(n, 1 + T, C, device=DEV)) for _ in range(L_)]
    hidden[1][2, 5, 3] = NAN                                     # region 2 has no valid point: weight 0 everywhere
    levels = [hs[:, 1:] for hs in hidden]
    assert all(not lv.is_contiguous() and lv.data_ptr() % 16 == 0 for lv in levels)
    ptrs = (ctypes.c_void_p * L_)(*[lv.data_ptr() for lv in levels])
    rs = (ctypes.c_long * L_)(*[lv.stride(1) for lv in levels])
    ims = (ctypes.c_long * L_)(*[lv.stride(0) for lv in levels])
    pooled = nan_bf16(n, C)
    Lb = _lib.lib()
    _lib.check(Lb.vllm_region_pool_bf16(P(wk), P(stem), ptrs, rs, ims, n, L_, T, C, P(pooled), stream()), "region_pool")
    torch.cuda.synchronize()
    wd = wk.double().cpu()
    maps = [stem.double().cpu()] + [lv.double().cpu().nan_to_num(0.0) for lv in levels]
    wts = [wd[0]] + [wd[k] for k in range(L_)]
    terms = torch.stack([wt[:, :, None] * m for wt, m in zip(wts, maps)])
    assert_bound(pooled.cpu(), terms.sum((0, 2)), terms.abs().sum((0, 2)), f"region_pool C{C} {h}x{w}")
    assert torch.equal(pooled[2], torch.zeros(C, device=DEV, dtype=torch.bfloat16))
    g = bf(torch.randn(n, C, device=DEV))
    for k in (0, 2):
        a, b = nan_bf16(n, T, C), nan_bf16(n, T, C)
        _lib.check(Lb.vllm_region_outer_bf16(P(wk[k]), P(g), P(a), n, T, C, stream()), "region_outer")
        _lib.check(Lb.vllm_region_outer_bf16(P(wk[k]), P(g), P(b), n, T, C, stream()), "region_outer")
        torch.cuda.synchronize()
        ref = wd[k][:, :, None] * g.double().cpu()[:, None, :]
        u = ((a.double().cpu() - ref).abs() / bf16_ulp(ref)).max().item()
        print(f"region_outer C{C} {h}x{w} level {k}: {u:.3f} bf16 ulp")
        assert bool(torch.isfinite(a.float()).all()) and u <= 1.0
        assert torch.equal(bits(a), bits(b))


# ---- the whole module -----------------------------------------------------------------------------------------------------------------------
HID, EMB, OUT, NPTS = 256, 64, 64, 37


def _encoder(native=True, seed=0):
    torch.manual_seed(seed)
    enc = A.RegionEncoder(hidden_dim=HID, embed_dim=EMB, out_dim=OUT, patch_size=14, mask_pool_type="grid_sample")
    with torch.no_grad():                                        # LayerNorm parameters off their 1 / 0 defaults, so their gradients mean something
        for i in (1, 4):
            enc.mask_embedding[i].weight.add_(0.2 * torch.randn_like(enc.mask_embedding[i].weight))
            enc.mask_embedding[i].bias.add_(0.1 * torch.randn_like(enc.mask_embedding[i].bias))
    enc = enc.to(DEV).to(torch.bfloat16).train()
    enc.num_points = NPTS
    enc.native_branch = native
    return enc


def _module_inputs():
    gen = torch.Generator().manual_seed(4)
    images = bf(torch.randn(3, 3, 56, 84, generator=gen)).to(DEV)
    masks = torch.zeros(3, 1, 56, 84)
    masks[0, 0, 10:30, 5:70] = 1
    masks[1, 0] = 1
    masks[2, 0, 40:50, 3:20] = 1                                 # every region non-empty (an empty one makes the fp64 twin NaN)
    hidden = [bf(torch.randn(3, 1 + 24, EMB, generator=gen)).to(DEV) for _ in range(3)]
    weight = torch.randn(3, OUT, generator=gen).to(DEV)
    return images, bf(masks).to(DEV), hidden, weight


def _step(enc, images, masks, hidden, weight, seed=1):
    """One training step; the middle level's parent requires grad.  -> {name: tensor}: out, every parameter's gradient, the level's."""
    enc.zero_grad(set_to_none=True)
    hid = [t.detach().clone() for t in hidden]
    hid[1].requires_grad_(True)
    torch.manual_seed(seed)
    out = enc(images, masks, [t[:, 1:] for t in hid])
    (out.to(weight.dtype) * weight).sum().backward()
    res = {"out": out.detach()}
    res.update({k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in enc.named_parameters()})
    res["level1"] = hid[1].grad[:, 1:].detach().clone()
    assert torch.equal(hid[1].grad[:, 0], torch.zeros_like(hid[1].grad[:, 0]))
    return res


def test_module_native_against_the_switch_off_module_and_fp64(monkeypatch):
    """hidden_dim 256, embed 64, out 64, 3 regions of 56 x 84, 37 points, 3 levels, bf16.  Forward, every parameter gradient and the
    gradient of a level, each against an fp64 CPU run of today's module statements with the same (replayed) points: native's relative
    rms error at most 1.25 x that of the same module with the switch off, in bf16, on the GPU -- per output and per parameter, each
    scaled by the rms of its fp64 value."""
    images, masks, hidden, weight = _module_inputs()
    enc = _encoder(native=True)
    recorded, real = [], A.rand_sample

    def record(x, divisor, max_len):
        recorded.append(real(x, divisor, max_len))
        return recorded[-1]

    monkeypatch.setattr(A, "rand_sample", record)
    calls = _lib.lib().vllm_region_encoder_calls()
    native = _step(enc, images, masks, hidden, weight)
    assert _lib.lib().vllm_region_encoder_calls() == calls + 2 and len(recorded) == 9
    points = list(recorded)

    def replay_on(device):
        it = iter(points)
        return lambda x, divisor, max_len: next(it).to(device)

    off = _encoder(native=False)
    off.load_state_dict(enc.state_dict())
    monkeypatch.setattr(A, "rand_sample", replay_on(DEV))
    composed = _step(off, images, masks, hidden, weight)
    twin = TR._TwinEncoder(hidden_dim=HID, embed_dim=EMB, out_dim=OUT, patch_size=14, mask_pool_type="grid_sample")
    twin.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    twin = twin.double().train()
    twin.num_points = NPTS
    monkeypatch.setattr(A, "rand_sample", replay_on("cpu"))
    ref = _step(twin, images.double().cpu(), masks.double().cpu(), [t.double().cpu() for t in hidden], weight.double().cpu())
    assert sorted(native) == sorted(ref) and len(ref) == 14
    worse = []
    for k in sorted(ref):
        assert native[k].dtype == torch.bfloat16 and native[k].shape == ref[k].shape and bool(torch.isfinite(native[k].float()).all()), k
        en, eo = rel_rms(native[k].cpu(), ref[k]), rel_rms(composed[k].cpu(), ref[k])
        print(f"region encoder {k}: native {en:.4g}  switch off {eo:.4g}  ratio {en / max(eo, 1e-300):.3f}")
        if not en <= 1.25 * eo:
            worse.append((k, en, eo))
    assert not worse, worse


def test_module_forward_bits_determinism_and_the_dummy_call():
    images, masks, hidden, weight = _module_inputs()
    enc = _encoder()
    levels = [t[:, 1:] for t in hidden]
    torch.manual_seed(1)
    with torch.no_grad():
        quiet = enc(images, masks, levels)
    torch.manual_seed(1)
    loud = enc(images, masks, levels)
    assert quiet.dtype == torch.bfloat16 and quiet.shape == (3, OUT) and not quiet.requires_grad
    assert loud.requires_grad and torch.equal(bits(loud.detach()), bits(quiet))
    torch.manual_seed(1)
    with torch.no_grad():                                        # fp32 images are rounded on the way in; a 4-D NCHW level is accepted
        nchw = [lv.reshape(3, 4, 6, EMB).permute(0, 3, 1, 2) for lv in levels]
        assert torch.equal(bits(enc(images.float(), masks.float(), nchw)), bits(quiet))
    a, b = _step(enc, images, masks, hidden, weight), _step(enc, images, masks, hidden, weight)
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), k
    # the reference's dummy forward when a batch has no regions (modeling_visionllmv2.py:699-715)
    enc.zero_grad(set_to_none=True)
    zeros = [torch.zeros(2, 16, EMB, device=DEV, dtype=torch.bfloat16)] * 3
    out = enc(torch.zeros(2, 3, 56, 56, device=DEV, dtype=torch.bfloat16), torch.ones(2, 1, 56, 56, device=DEV, dtype=torch.bfloat16), zeros)
    (out * 0.).sum().backward()
    for k, p in enc.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, torch.zeros_like(p.grad)), k


def test_a_frozen_subset_gets_no_gradient_and_no_weight_gradient_launch():
    images, masks, hidden, weight = _module_inputs()
    enc = _encoder()
    L = _lib.lib()
    before = L.vllm_region_encoder_wgrad_launches()
    full = _step(enc, images, masks, hidden, weight)
    assert L.vllm_region_encoder_wgrad_launches() == before + 4
    frozen = ("mask_embedding.0.weight", "mask_embedding.0.bias", "mask_embedding.1.weight", "mask_embedding.1.bias", "up_dim.weight",
              "up_dim.bias", "mask_embedding.6.bias")
    for k, p in enc.named_parameters():
        p.requires_grad_(k not in frozen)
    before = L.vllm_region_encoder_wgrad_launches()
    part = _step(enc, images, masks, hidden, weight)
    assert L.vllm_region_encoder_wgrad_launches() == before + 2  # conv2 and conv3 only
    for k in full:
        if k in frozen:
            assert part[k] is None, k
        else:
            assert torch.equal(bits(part[k]), bits(full[k])), k
    # a trained bias beside a frozen weight: the bias comes out of the weight gradient's launch, the weight's buffer is dropped
    for k, p in enc.named_parameters():
        p.requires_grad_(k == "mask_embedding.3.bias")
    before = L.vllm_region_encoder_wgrad_launches()
    only = _step(enc, images, masks, hidden, weight)
    assert L.vllm_region_encoder_wgrad_launches() == before + 1
    for k in full:
        if k in ("out", "level1", "mask_embedding.3.bias"):
            assert torch.equal(bits(only[k]), bits(full[k])), k
        else:
            assert only[k] is None, k


def test_caller_workspace_contract(monkeypatch):
    """The three entries through tests/workspace_guard.py (test_workspace_contract_gpu.three_runs: exact size, least alignment, hostile
    content, guard bytes, bit identity to a clean run): the size query is asked once per call, the forward and the backward each get a
    fresh workspace with the run's fill."""
    images, masks, hidden, weight = _module_inputs()
    enc = _encoder()

    def run(W):
        return _step(enc, images, masks, hidden, weight)

    outs, spaces = WC.three_runs(run, widest_row_bytes=256 * 2, patch=monkeypatch)
    d = _lib.VllmRegionEncoder(hidden=HID, embed=EMB, out_dim=OUT, patch=14, n=3, H=56, W=84, levels=3, points=NPTS, pixel_is_f32=0, eps=1e-6)
    need = _lib.lib().vllm_region_encoder_workspace_bytes(ctypes.byref(d))
    assert spaces[0].sizes == [need, need] and need > 0
    assert all(bool(torch.isfinite(v.float()).all()) for v in outs[0].values())


def test_model_shaped_encoder_runs_the_native_entry():
    """hidden_dim 256 as modeling_visionllmv2.py builds it, ViT-L sized levels (embed 1024) with a CLS row in front, 448 x 448: the
    switch reaches vllm_region_encoder_forward (one call under no-grad) and agrees with the switch-off module to bf16 accuracy."""
    torch.manual_seed(2)
    enc = A.RegionEncoder(hidden_dim=256, embed_dim=1024, out_dim=4096, patch_size=14, mask_pool_type="grid_sample").to(DEV).to(torch.bfloat16)
    images = bf(torch.randn(2, 3, 448, 448, device=DEV))
    masks = torch.zeros(2, 1, 448, 448, device=DEV, dtype=torch.bfloat16)
    masks[0, 0, 100:300, 50:400] = 1
    masks[1, 0, 10:60, 10:60] = 1
    levels = [bf(torch.randn(2, 1 + 1024, 1024, device=DEV))[:, 1:] for _ in range(3)]
    torch.manual_seed(3)
    with torch.no_grad():
        ref = enc(images, masks, levels)
    enc.native_branch = True
    calls = _lib.lib().vllm_region_encoder_calls()
    torch.manual_seed(3)
    with torch.no_grad():
        out = enc(images, masks, levels)
    assert _lib.lib().vllm_region_encoder_calls() == calls + 1
    assert out.shape == ref.shape == (2, 4096) and out.dtype == torch.bfloat16
    r = rel_rms(out, ref)
    print(f"model-shaped region encoder: native against switch off, relative rms {r:.4g}")
    assert r < 3e-2                                              # two bf16 evaluations of the same function (bf16 resolution 2^-8 per rounding)
