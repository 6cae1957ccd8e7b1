"""Inputs, yardstick and bounds of the InternViT layer training tests (test_vit_layer_train_cpu.py, test_vit_layer_train_gpu.py).

A torch RESTATEMENT of the reference's statements (VisionLLMv2/visionllmv2/model/internvit/modeling_intern_vit.py), written for any
floating dtype so that the same statements give
  * the yardstick: torch fp64 autograd on the bf16-rounded parameters, input and grad_out, and
  * torch's own bf16 autograd of the same statements (the other side of DESIGN section 5's assembled-bf16 rule).
It never calls the code under test.  Statements and their lines:
  rms_norm     :39-44   InternRMSNorm.forward (statistics in at least fp32, cast back, THEN times weight)
  naive_attn   :118-140 InternAttention._naive_attn (qkv Linear, unbind, q_norm / k_norm over the flattened heads :131-134, softmax, proj)
  mlp          :175-179 InternMLP.forward (fc1, erf GELU, fc2)
  layer        :206-208 InternVisionEncoderLayer.forward (x + attn(norm1 x) ls1; x + mlp(norm2 x) ls2; drop_path = identity)

Parameter init (no gradient tensor degenerate): Linear weights randn / sqrt(K), biases 0.1 randn, norm weights 1 + 0.1 randn,
ls1 / ls2 0.1 (1 + 0.1 randn), x randn, grad_out randn / sqrt(C).

Bounds of the two row-wise kernels, the form and constants of test_layernorm_backward_against_fp64 (|err| <= 1 bf16 ulp(ref) + 2^-17 mag):
  RMSNorm  grad_x: mag = 4 r (|g| + |xhat| mean|g xhat|) [+ |grad_res|], g = grad_y w;   grad_w: mag = sum_rows |grad_y xhat|
  LayerScale  grad_y: 1 ulp;   grad_ls: mag = sum_rows |grad_out y|
``emulate_*`` walk the kernels' arithmetic in fp32 on the CPU (statistics, products and sums in fp32, one rounding to bf16):
test_vit_layer_train_cpu.py keeps them inside the bounds at the GPU tests' shapes, so the bounds are ones a faithful implementation meets.
Nothing here touches torch.cuda at import."""
import math

import torch

from bounds import bf16_ulp, excess_ulp, rel_rms  # noqa: F401  (the project's bound, re-exported)

EPS = 1e-6
NORM_SHAPES = [(300, 128), (77, 1024), (64, 3200), (33, 200)]          # (rows, C) of the row-wise kernels' tests
# (hidden, heads, inter, B, S, qk_normalization, qkv_bias)
LAYER_CONFIGS = [(128, 2, 256, 2, 37, True, False),
                 (256, 2, 512, 3, 65, False, True),                     # head_dim 128
                 (1024, 16, 4096, 2, 577, True, False),                 # the 8-phase GEMM and split-wgrad routes
                 (3200, 25, 12800, 1, 130, True, False)]                # InternViT-6B widths


# ---- the reference's statements -------------------------------------------------------------------------------------------------------
def rms_norm(x, weight, eps=EPS):
    """:39-44 (``.to(torch.float32)`` widens a 16-bit input; an fp64 input stays fp64)"""
    input_dtype = x.dtype
    h = x.to(torch.promote_types(input_dtype, torch.float32))
    variance = h.pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(variance + eps)
    return weight * h.to(input_dtype)


def naive_attn(p, x, heads, eps=EPS):
    """:118-140 with attn_drop / proj_drop the identity"""
    B, N, C = x.shape
    qkv = torch.nn.functional.linear(x, p["attn.qkv.weight"], p.get("attn.qkv.bias"))
    qkv = qkv.reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    if "attn.q_norm.weight" in p:
        B_, H_, N_, D_ = q.shape
        q = rms_norm(q.transpose(1, 2).flatten(-2, -1), p["attn.q_norm.weight"], eps).view(B_, N_, H_, D_).transpose(1, 2)
        k = rms_norm(k.transpose(1, 2).flatten(-2, -1), p["attn.k_norm.weight"], eps).view(B_, N_, H_, D_).transpose(1, 2)
    scale = (C // heads) ** -0.5
    attn = ((q * scale) @ k.transpose(-2, -1))
    attn = attn.softmax(dim=-1)
    y = (attn @ v).transpose(1, 2).reshape(B, N, C)
    return torch.nn.functional.linear(y, p["attn.proj.weight"], p["attn.proj.bias"])


def sdpa_attn(p, x, heads, eps=EPS):
    """the same block with F.scaled_dot_product_attention in place of :136-140 (what the flash path computes; benchmarks only)"""
    B, N, C = x.shape
    qkv = torch.nn.functional.linear(x, p["attn.qkv.weight"], p.get("attn.qkv.bias"))
    qkv = qkv.reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    if "attn.q_norm.weight" in p:
        B_, H_, N_, D_ = q.shape
        q = rms_norm(q.transpose(1, 2).flatten(-2, -1), p["attn.q_norm.weight"], eps).view(B_, N_, H_, D_).transpose(1, 2)
        k = rms_norm(k.transpose(1, 2).flatten(-2, -1), p["attn.k_norm.weight"], eps).view(B_, N_, H_, D_).transpose(1, 2)
    y = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, C)
    return torch.nn.functional.linear(y, p["attn.proj.weight"], p["attn.proj.bias"])


def mlp(p, x):
    """:175-179 (ACT2FN['gelu'] is the erf GELU)"""
    h = torch.nn.functional.linear(x, p["mlp.fc1.weight"], p["mlp.fc1.bias"])
    h = torch.nn.functional.gelu(h)
    return torch.nn.functional.linear(h, p["mlp.fc2.weight"], p["mlp.fc2.bias"])


def layer(p, x, heads, eps=EPS, attn=naive_attn):
    """:206-208"""
    x = x + attn(p, rms_norm(x, p["norm1.weight"], eps), heads, eps) * p["ls1"]
    x = x + mlp(p, rms_norm(x, p["norm2.weight"], eps)) * p["ls2"]
    return x


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_params(hidden, inter, qk_norm=True, qkv_bias=False, seed=0, device="cpu"):
    """-> {state-dict key of InternVisionEncoderLayer: bf16 tensor}"""
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    C, I = hidden, inter
    p = {"norm1.weight": 1 + 0.1 * rn(C), "attn.qkv.weight": rn(3 * C, C) / math.sqrt(C)}
    if qkv_bias:
        p["attn.qkv.bias"] = 0.1 * rn(3 * C)
    if qk_norm:
        p["attn.q_norm.weight"] = 1 + 0.1 * rn(C)
        p["attn.k_norm.weight"] = 1 + 0.1 * rn(C)
    p.update({"attn.proj.weight": rn(C, C) / math.sqrt(C), "attn.proj.bias": 0.1 * rn(C), "ls1": 0.1 * (1 + 0.1 * rn(C)),
              "norm2.weight": 1 + 0.1 * rn(C), "mlp.fc1.weight": rn(I, C) / math.sqrt(C), "mlp.fc1.bias": 0.1 * rn(I),
              "mlp.fc2.weight": rn(C, I) / math.sqrt(I), "mlp.fc2.bias": 0.1 * rn(C), "ls2": 0.1 * (1 + 0.1 * rn(C))})
    return {k: v.to(torch.bfloat16) for k, v in p.items()}


def make_io(B, S, hidden, seed=0, device="cpu"):
    """-> (x, grad_out) bf16 [B, S, hidden]"""
    g = torch.Generator(device=device).manual_seed(2000 + seed)
    x = torch.randn(B, S, hidden, generator=g, device=device)
    go = torch.randn(B, S, hidden, generator=g, device=device) / math.sqrt(hidden)
    return x.to(torch.bfloat16), go.to(torch.bfloat16)


def autograd_layer(params, x, grad_out, heads, dtype, eps=EPS, attn=naive_attn):
    """torch autograd of ``layer`` in ``dtype`` on copies of the bf16 values -> (out, {name: grad}, x.grad)"""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().to(dtype).requires_grad_(True)
    out = layer(p, xx, heads, eps, attn)
    out.backward(grad_out.to(dtype))
    return out.detach(), {k: v.grad for k, v in p.items()}, xx.grad


def autograd_rms_norm(x, weight, grad_y, dtype, eps=EPS):
    xx, ww = x.detach().to(dtype).requires_grad_(True), weight.detach().to(dtype).requires_grad_(True)
    y = rms_norm(xx, ww, eps)
    y.backward(grad_y.to(dtype))
    return y.detach(), xx.grad, ww.grad


def norm_case(rows, C, seed=0, device="cpu"):
    """-> x, grad_y, grad_res [rows, C], w [C] (bf16) for the row-wise kernels"""
    g = torch.Generator(device=device).manual_seed(3000 + seed + rows + C)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    bf = lambda t: t.to(torch.bfloat16)
    return bf(rn(rows, C) * 1.5), bf(rn(rows, C)), bf(rn(rows, C)), bf(1 + 0.1 * rn(C))


# ---- the row-wise kernels: fp64 reference, bounds, fp32 emulation ---------------------------------------------------------------------
def rms_bwd_ref(x, gy, w, gres=None, eps=EPS):
    """fp64 backward of y = w * (x r) (the forward's intermediate rounding has no derivative) -> (grad_x, grad_w, mag_x, mag_w)"""
    x, gy, w = x.double(), gy.double(), w.double()
    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    xh, g = x * r, gy * w
    gx = r * (g - xh * (g * xh).mean(-1, keepdim=True))
    mag_x = 4 * r * (g.abs() + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    if gres is not None:
        gx = gx + gres.double()
        mag_x = mag_x + gres.double().abs()
    return gx, (gy * xh).sum(0), mag_x, (gy * xh).abs().sum(0)


def emulate_rms_bwd(x, gy, w, gres=None, eps=EPS):
    """the kernel's arithmetic in fp32 -> bf16 (grad_x, grad_w)"""
    x, gy, w = x.float(), gy.float(), w.float()
    r = torch.rsqrt(x.pow(2).sum(-1, keepdim=True) / x.shape[-1] + eps)
    xh = x * r
    g = gy * w
    gx = r * (g - xh * ((g * xh).sum(-1, keepdim=True) / x.shape[-1]))
    if gres is not None:
        gx = gx + gres.float()
    return gx.to(torch.bfloat16), (gy * xh).sum(0).to(torch.bfloat16)


def ls_bwd_ref(go, y, ls):
    go, y, ls = go.double(), y.double(), ls.double()
    return go * ls, (go * y).sum(0), (go * y).abs().sum(0)


def emulate_ls_bwd(go, y, ls):
    return (go.float() * ls.float()).to(torch.bfloat16), (go.float() * y.float()).sum(0).to(torch.bfloat16)
