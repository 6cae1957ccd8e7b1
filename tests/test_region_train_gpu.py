"""Region encoder under autograd: the native backward of the point pooling (vllm_point_sample_mean_backward_f32 / _bf16,
vllm_point_sample_backward_f32) against torch's fp64 autograd of the oracle expression masked_mean(point_sample(x, c), v).
Inputs, references and the derived bounds: region_train_inputs.py."""
import copy

import pytest
import torch

import region_train_inputs as RT
from oracle import region as O
from visionllm_amd import _lib
from visionllm_amd import region_encoder as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

MEAN_SHAPES = [(16, 384, 24, 24, 2304),      # region-encoder shape, 16-byte stores
               (3, 100, 5, 7, 300),          # odd map: single-element stores
               (2, 9, 80, 80, 500),          # too large for the LDS accumulators: A through the workspace
               (2, 200, 24, 24, 64), (3, 8, 6, 4, 0), (1, 3, 1, 1, 7)]
UNFUSED_SHAPES = [(4, 256, 24, 24, 2304), (1, 3, 1, 1, 7), (2, 17, 5, 9, 1), (2, 9, 80, 80, 500)]


def _seed(N, C, H, W, P):
    return N * 1000 + C + H + P


def _native_mean_grad(c, v, g, C, H, W, dtype=torch.float32):
    x = torch.zeros(c.shape[0], C, H, W, device=DEV, dtype=dtype, requires_grad=True)
    out = A.point_sample_masked_mean(x, c.to(DEV), v.to(DEV))
    assert out.dtype == dtype and out.requires_grad
    out.backward(g.to(DEV).to(dtype))
    return x.grad


def _mean_abi(c, v, g, C, H, W, grad_in, name="vllm_point_sample_mean_backward_f32"):
    """Straight through the C ABI into ``grad_in`` (pre-filled by the caller)."""
    N, P = v.shape
    L = _lib.lib()
    nbytes = L.vllm_point_sample_backward_workspace_bytes(N, C, H, W, P)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    cd, vd, gd = c.to(DEV), v.to(torch.uint8).to(DEV), g.to(DEV)
    _lib.check(getattr(L, name)(_lib.ptr(cd), _lib.ptr(vd), _lib.ptr(gd), N, C, H, W, P, _lib.ptr(grad_in), _lib.ptr(ws), nbytes,
                                _lib.current_stream(DEV)), name)
    torch.cuda.synchronize()
    return grad_in


@pytest.mark.parametrize("N,C,H,W,P", MEAN_SHAPES)
def test_masked_mean_grad_vs_fp64_autograd(N, C, H, W, P):
    """grad_in of the fused masked mean, fp32, element-wise inside the derived bound (region_train_inputs.mean_bound).  A region
    without a valid point and the P == 0 case give exact zeros; the reference's autograd gives NaN there on every pixel one of the
    region's (invalid) points touches -- asserted too, so the departure stays visible."""
    c, v, g = RT.make_case(N, C, H, W, P, _seed(N, C, H, W, P))
    ref = RT.mean_reference(c, v, g, C, H, W)
    out = _native_mean_grad(c, v, g, C, H, W).cpu()
    assert out.shape == (N, C, H, W) and out.dtype == torch.float32
    live = v.sum(1) > 0
    assert not live[N - 1]
    assert torch.equal(out[~live], torch.zeros_like(out[~live]))
    for n in (~live).nonzero().flatten().tolist():
        touched = RT.scatter_per_pixel(torch.ones(N, 1, P), c, H, W)[n, 0] > 0
        assert torch.equal(torch.isnan(ref[n]).reshape(C, H * W), touched[None].expand(C, -1))
    if live.any():
        err = (out.double() - ref)[live].abs()
        bound = RT.mean_bound(ref, c, v, g, H, W)[live]
        worst = (err / bound.clamp(min=1e-300)).max().item()
        print(f"masked-mean grad {(N, C, H, W, P)}: max |err| {err.max().item():.3e}, max err / bound {worst:.3f}")
        assert (err <= bound).all(), f"{int((err > bound).sum())} elements outside the bound, worst err / bound {worst:.3f}"


@pytest.mark.parametrize("N,C,H,W,P", MEAN_SHAPES)
def test_masked_mean_grad_fully_written_and_deterministic(N, C, H, W, P):
    """Through the C ABI with grad_in pre-filled with NaN: no NaN survives; three repeated calls are bit-identical; grad_in does not
    depend on the map, so a NaN placed in the feature map does not reach it."""
    c, v, g = RT.make_case(N, C, H, W, P, _seed(N, C, H, W, P))
    first = _mean_abi(c, v, g, C, H, W, torch.full((N, C, H, W), float("nan"), device=DEV))
    assert torch.isfinite(first).all()
    for _ in range(3):
        again = _mean_abi(c, v, g, C, H, W, torch.full((N, C, H, W), float("nan"), device=DEV))
        assert torch.equal(again, first)
    assert torch.equal(_native_mean_grad(c, v, g, C, H, W), first)
    x = torch.randn(N, C, H, W, device=DEV)
    x[:, :, 0, 0] = float("nan")
    x.requires_grad_(True)
    A.point_sample_masked_mean(x, c.to(DEV), v.to(DEV)).backward(g.to(DEV))
    assert torch.equal(x.grad, first)


@pytest.mark.parametrize("N,C,H,W,P", MEAN_SHAPES)
def test_masked_mean_grad_bf16_is_the_rounded_fp32(N, C, H, W, P):
    """The bf16 entry point writes the fp32 value rounded to nearest even once; through Python a bf16 map gets a bf16 .grad."""
    c, v, g = RT.make_case(N, C, H, W, P, _seed(N, C, H, W, P))
    f32 = _mean_abi(c, v, g, C, H, W, torch.full((N, C, H, W), float("nan"), device=DEV))
    b16 = _mean_abi(c, v, g, C, H, W, torch.full((N, C, H, W), float("nan"), device=DEV, dtype=torch.bfloat16),
                    name="vllm_point_sample_mean_backward_bf16")
    assert torch.equal(b16, f32.to(torch.bfloat16))
    gb = g.to(torch.bfloat16)                                  # (what autograd hands a bf16 output's backward)
    grad = _native_mean_grad(c, v, gb.float(), C, H, W, dtype=torch.bfloat16)
    assert grad.dtype == torch.bfloat16 and grad.shape == (N, C, H, W)
    assert torch.equal(grad, _mean_abi(c, v, gb.float(), C, H, W, torch.empty((N, C, H, W), device=DEV)).to(torch.bfloat16))


@pytest.mark.parametrize("grid_form", [False, True])
@pytest.mark.parametrize("N,C,H,W,P", UNFUSED_SHAPES)
def test_point_sample_grad_vs_fp64_autograd(N, C, H, W, P, grid_form):
    """grad_in of the unfused point_sample, (N, P, 2) and (N, Hg, Wg, 2) forms, inside region_train_inputs.unfused_bound; fully
    written (NaN pre-fill through the C ABI).  The kernel sums with float atomics in arrival order, so repeats are compared inside the
    same bound, not bit for bit."""
    c, _, g = RT.make_case(N, C, H, W, P, _seed(N, C, H, W, P) + 1, unfused=True)
    ref = RT.unfused_reference(c, g, H, W)
    bound = RT.unfused_bound(c, g, H, W)
    x = torch.zeros(N, C, H, W, device=DEV, requires_grad=True)
    if grid_form:
        hg = 2 if P % 2 == 0 else 1
        out = A.point_sample(x, c.reshape(N, hg, P // hg, 2).to(DEV))
        assert out.shape == (N, C, hg, P // hg)
        out.backward(g.reshape(N, C, hg, P // hg).to(DEV))
    else:
        out = A.point_sample(x, c.to(DEV))
        assert out.shape == (N, C, P)
        out.backward(g.to(DEV))
    err = (x.grad.cpu().double() - ref).abs()
    worst = (err / bound.clamp(min=1e-300)).max().item()
    print(f"point_sample grad {(N, C, H, W, P)}: max |err| {err.max().item():.3e}, max err / bound {worst:.3f}")
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements outside the bound, worst err / bound {worst:.3f}"
    filled = torch.full((N, C, H, W), float("nan"), device=DEV)
    cd, gd = c.to(DEV), g.to(DEV)
    _lib.check(_lib.lib().vllm_point_sample_backward_f32(_lib.ptr(cd), _lib.ptr(gd), N, C, H, W, P, _lib.ptr(filled), None, 0,
                                                         _lib.current_stream(DEV)), "vllm_point_sample_backward_f32")
    torch.cuda.synchronize()
    assert torch.isfinite(filled).all()
    assert ((filled.cpu().double() - ref).abs() <= bound).all()


class _TwinEncoder(A.RegionEncoder):
    """The same module with the point pooling composed from the oracle's point_sample + masked_mean under torch autograd."""

    def _pool_points(self, feat, masks):
        H, W = masks.shape[-2:]
        divisor = torch.tensor([1, H, W], device=masks.device)[None,]
        pts = torch.nn.utils.rnn.pad_sequence([A.rand_sample(m, divisor, self.num_points) for m in masks], padding_value=-1)
        pts = pts.permute(1, 0, 2)
        valid = pts.sum(dim=-1) >= 0
        return O.masked_mean(O.point_sample(feat, pts[:, :, -2:].flip(dims=[-1]).to(feat.dtype)), valid)


def _module_case():
    torch.manual_seed(0)
    enc = A.RegionEncoder(hidden_dim=32, embed_dim=16, out_dim=24, patch_size=14, mask_pool_type="grid_sample").to(DEV).train()
    images = torch.randn(3, 3, 56, 56, device=DEV)
    masks = torch.zeros(3, 1, 56, 56, device=DEV)
    masks[0, 0, 10:30, 5:40] = 1
    masks[1, 0, 0:56, 0:56] = 1
    masks[2, 0, 40:50, 3:20] = 1                  # every region non-empty (an empty one makes the reference twin NaN)
    feats = [torch.randn(3, 16, 4, 4, device=DEV), torch.randn(3, 16, 16, device=DEV)]
    weight = torch.randn(3, 24, device=DEV)
    return enc, images, masks, feats, weight


def _grads(enc, images, masks, feats, weight):
    enc.zero_grad(set_to_none=True)
    torch.manual_seed(1)                          # rand_sample draws the same points
    (enc(images, masks, feats) * weight).sum().backward()
    return {k: p.grad.detach().double().cpu() for k, p in enc.named_parameters()}


def test_module_trains_and_matches_the_autograd_twin(monkeypatch):
    """RegionEncoder in train mode: loss.backward() fills a finite .grad for every parameter.  Judged by the error of a twin that
    pools through torch autograd (grid_sample -> mask -> sum -> div) in fp32 on the GPU, both against the same twin in fp64 on the
    CPU with the same parameters and points: relative rms and worst element of (native - fp64) at most 4x those of (twin32 - fp64),
    over all parameters, each parameter's differences scaled by the rms of its fp64 gradient.  Native and twin differ only in the
    summation order inside the pooling, so the ratios scatter around 1; the cap is there to catch a systematic error.
    Measured on an MI355X (two runs): rms ratio 0.59 / 0.60, worst-element ratio 0.42 / 0.62 (native 1.5e-7 rms, 0.8-1.1e-6 worst;
    twin32 2.6-2.8e-7 rms, 1.8-1.9e-6 worst, in units of each parameter's rms gradient)."""
    enc, images, masks, feats, weight = _module_case()
    recorded = []
    real = A.rand_sample

    def record(x, divisor, max_len):
        recorded.append(real(x, divisor, max_len))
        return recorded[-1]

    monkeypatch.setattr(A, "rand_sample", record)
    native = _grads(enc, images, masks, feats, weight)
    assert sorted(native) == sorted(k for k, _ in enc.named_parameters()) and len(native) == 12
    assert all(k.startswith(("mask_embedding.", "up_dim.")) for k in native)
    assert all(torch.isfinite(gr).all() and gr.abs().max() > 0 for gr in native.values())
    points = list(recorded)

    def replay_on(device):
        it = iter(points)
        return lambda x, divisor, max_len: next(it).to(device)

    twin32 = _TwinEncoder(hidden_dim=32, embed_dim=16, out_dim=24, patch_size=14, mask_pool_type="grid_sample").to(DEV).train()
    twin32.load_state_dict(enc.state_dict())
    monkeypatch.setattr(A, "rand_sample", replay_on(DEV))
    g32 = _grads(twin32, images, masks, feats, weight)
    twin64 = copy.deepcopy(twin32).double().cpu()
    monkeypatch.setattr(A, "rand_sample", replay_on("cpu"))
    g64 = _grads(twin64, images.double().cpu(), masks.double().cpu(), [f.double().cpu() for f in feats], weight.double().cpu())

    def scaled(a):
        return torch.cat([((a[k] - g64[k]) / g64[k].pow(2).mean().sqrt()).flatten() for k in sorted(g64)])

    dn, dt = scaled(native), scaled(g32)
    rms_ratio = (dn.pow(2).mean().sqrt() / dt.pow(2).mean().sqrt()).item()
    worst_ratio = (dn.abs().max() / dt.abs().max()).item()
    print(f"module grads: native rms {dn.pow(2).mean().sqrt().item():.3e} worst {dn.abs().max().item():.3e}; twin32 rms "
          f"{dt.pow(2).mean().sqrt().item():.3e} worst {dt.abs().max().item():.3e}; ratios rms {rms_ratio:.2f} worst {worst_ratio:.2f}")
    assert rms_ratio <= 4.0 and worst_ratio <= 4.0, (rms_ratio, worst_ratio)


def test_module_forward_under_grad_equals_no_grad_and_the_dummy_call_trains():
    enc, images, masks, feats, _ = _module_case()
    torch.manual_seed(1)
    with torch.no_grad():
        quiet = enc(images, masks, feats)
    torch.manual_seed(1)
    loud = enc(images, masks, feats)
    assert loud.requires_grad and torch.equal(loud.detach(), quiet)
    # the reference's dummy forward when a batch has no regions (modeling_visionllmv2.py:699-715)
    enc.zero_grad(set_to_none=True)
    zeros = [torch.zeros(2, 16, 16, device=DEV)] * 3
    out = enc(torch.zeros(2, 3, 56, 56, device=DEV), torch.ones(2, 1, 56, 56, device=DEV), zeros)
    (out * 0.).sum().backward()
    for k, p in enc.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, torch.zeros_like(p.grad)), k


def test_coordinate_gradients_still_raise():
    x = torch.randn(2, 4, 6, 6, device=DEV, requires_grad=True)
    c = torch.rand(2, 5, 2, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="point_coords"):
        A.point_sample(x, c)
    with pytest.raises(NotImplementedError, match="point_coords"):
        A.point_sample_masked_mean(x.detach(), c, torch.ones(2, 5, dtype=torch.bool, device=DEV))
    with torch.no_grad():                                      # (the no-grad path is the forward kernel it always was)
        assert A.point_sample(x, c).shape == (2, 4, 5)
    h = x.detach().half().requires_grad_(True)                 # another dtype is converted outside the Function, under autograd
    A.point_sample_masked_mean(h, c.detach(), torch.ones(2, 5, dtype=torch.bool, device=DEV)).sum().backward()
    assert h.grad.dtype == torch.float16 and h.grad.shape == h.shape and torch.isfinite(h.grad).all()


def test_bf16_module_step():
    """The model runs the region encoder in bf16: a training step gives finite bf16 gradients for every parameter."""
    enc, images, masks, feats, weight = _module_case()
    enc = enc.to(torch.bfloat16)
    torch.manual_seed(1)
    (enc(images.bfloat16(), masks.bfloat16(), [f.bfloat16() for f in feats]).float() * weight).sum().backward()
    for k, p in enc.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.bfloat16 and torch.isfinite(p.grad).all(), k


# ---- operand placement: offset views and a caller's stream ----------------------------------------------------------------
def _offset(t):
    """``t``'s values as a contiguous view one element into a larger allocation (4-byte aligned only for fp32)."""
    parent = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = parent[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0
    return view


def _both_grads(x, c, v, gm, gp):
    xm = x.detach().requires_grad_(True)
    A.point_sample_masked_mean(xm, c, v).backward(gm)
    xp = x.detach().requires_grad_(True)
    A.point_sample(xp, c).backward(gp)
    return xm.grad, xp.grad


@pytest.mark.parametrize("N,C,H,W,P", [(4, 256, 24, 24, 2304), (2, 17, 5, 9, 300), (2, 9, 80, 80, 500)])
def test_differentiable_calls_on_offset_views_and_a_side_stream(N, C, H, W, P):
    """The two differentiable calls with the map, the coordinates and grad_out as offset views give the bits they give on fresh
    tensors (the unfused gradient: inside its bound, it sums in arrival order), and so do they under a non-default stream."""
    c, v, gm = RT.make_case(N, C, H, W, P, _seed(N, C, H, W, P) + 2)
    gp = torch.randn(N, C, P, generator=torch.Generator().manual_seed(5))
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)
    c, v, gm, gp = c.to(DEV), v.to(DEV), gm.to(DEV), gp.to(DEV)
    bound = RT.unfused_bound(c.cpu(), gp.cpu(), H, W)
    base_m, base_p = _both_grads(x, c, v, gm, gp)
    ref_p = RT.unfused_reference(c.cpu(), gp.cpu(), H, W)
    assert ((base_p.cpu().double() - ref_p).abs() <= bound).all()
    off_m, off_p = _both_grads(_offset(x), _offset(c), v, _offset(gm), _offset(gp))
    assert torch.equal(off_m, base_m)
    assert ((off_p.cpu().double() - ref_p).abs() <= bound).all()
    # grad_in itself at an offset (through the C ABI): the single-element store path, same bits
    parent = torch.full((N * C * H * W + 1,), float("nan"), device=DEV)
    _mean_abi(c.cpu(), v.cpu(), gm.cpu(), C, H, W, parent[1:])
    assert torch.equal(parent[1:].view(N, C, H, W), base_m)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        st_m, st_p = _both_grads(x, c, v, gm, gp)
    side.synchronize()
    assert torch.equal(st_m, base_m)
    assert ((st_p.cpu().double() - ref_p).abs() <= bound).all()
