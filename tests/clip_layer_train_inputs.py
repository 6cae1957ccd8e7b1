"""Inputs, yardstick and bounds of the CLIP layer training tests (test_clip_layer_train_cpu.py, test_clip_layer_train_gpu.py).

A torch RESTATEMENT of transformers 4.34's statements (models/clip/modeling_clip.py), written for any floating dtype so that the same
statements give
  * the yardstick: torch fp64 autograd on the bf16-rounded parameters, input and grad_out, and
  * torch's own bf16 autograd of the same statements (the other side of DESIGN section 5's assembled-bf16 rule).
It never calls the code under test.  Statements:
  clip_attention   CLIPAttention.forward without masks and dropout: separate q / k / v Linears, ``q_proj(x) * scale``, bmm, softmax, bmm,
                   ``out_proj``
  clip_mlp         CLIPMLP.forward: fc1, ACT2FN[hidden_act] (``quick_gelu`` = x * sigmoid(1.702 x), ``gelu`` = erf GELU), fc2
  layer            CLIPEncoderLayer.forward: x + attn(layer_norm1 x); x + mlp(layer_norm2 x)   (nn.LayerNorm = F.layer_norm)
  tower            CLIPVisionTransformer.forward: embeddings (embed_train_inputs.embeddings without a conv bias), pre_layrnorm, the layers;
                   post_layernorm(last[:, 0]) -> (hidden_states, pooler_output)
test_clip_layer_train_cpu.py chains ``layer`` over the state dicts of tests/golden/clip_tiny.npz and clip_small_d64.npz (made with the HF class)
and reproduces their hidden states, which ties this yardstick to the reference's own run.

Parameter init, as vit_layer_train_inputs.py (no gradient tensor degenerate): Linear weights randn / sqrt(K), biases 0.1 randn, LayerNorm
weights 1 + 0.1 randn, LayerNorm biases 0.1 randn, x randn, grad_out randn / sqrt(C).

Bound of the row-wise kernel, the form and constants of test_layernorm_backward_against_fp64 (|err| <= 1 bf16 ulp(ref) + 2^-17 mag):
  grad_x: mag = 4 r (|g| + mean|g| + |xhat| mean|g xhat|) [+ |grad_res|], g = grad_y gamma;   grad_w: mag = sum_rows |grad_y xhat|;
  grad_b: mag = sum_rows |grad_y|
``emulate_*`` walk the kernels' arithmetic in fp32 on the CPU (statistics, products and sums in fp32, one rounding to bf16):
test_clip_layer_train_cpu.py keeps them inside the bounds at the GPU tests' shapes, so the bounds are ones a faithful implementation meets.
Nothing here touches torch.cuda at import."""
import math

import torch
import torch.nn.functional as F

from bounds import bf16_ulp, excess_ulp, rel_rms  # noqa: F401  (the project's bound, re-exported)
from embed_train_inputs import embeddings

EPS = 1e-5
NORM_SHAPES = [(300, 128), (77, 1024), (64, 1280), (33, 192)]          # (rows, C) of the row-wise kernel's tests
# (hidden, heads, inter, B, S, act)
LAYER_CONFIGS = [(128, 2, 256, 2, 37, "quick_gelu"),
                 (256, 2, 512, 3, 65, "gelu"),                          # head_dim 128, and the other activation
                 (1024, 16, 4096, 2, 577, "quick_gelu")]                # 1154 rows: the 8-phase GEMM and the split weight-gradient route
QUICK_GELU_GRAD_MAX = 1.0999                                            # sup |q'|  (checked on a dense grid by the CPU tests)


# ---- the reference's statements -------------------------------------------------------------------------------------------------------
def quick_gelu(x):
    """transformers.activations.QuickGELUActivation"""
    return x * torch.sigmoid(1.702 * x)


ACT = {"quick_gelu": quick_gelu, "gelu": F.gelu}


def clip_attention(p, x, heads):
    """CLIPAttention.forward (attention_mask = causal_attention_mask = None, dropout 0)"""
    bsz, tgt_len, embed_dim = x.shape
    head_dim = embed_dim // heads
    scale = head_dim ** -0.5
    shape = lambda t: t.view(bsz, tgt_len, heads, head_dim).transpose(1, 2).contiguous()
    query_states = F.linear(x, p["self_attn.q_proj.weight"], p["self_attn.q_proj.bias"]) * scale
    key_states = shape(F.linear(x, p["self_attn.k_proj.weight"], p["self_attn.k_proj.bias"]))
    value_states = shape(F.linear(x, p["self_attn.v_proj.weight"], p["self_attn.v_proj.bias"]))
    proj_shape = (bsz * heads, -1, head_dim)
    query_states = shape(query_states).view(*proj_shape)
    key_states = key_states.view(*proj_shape)
    value_states = value_states.view(*proj_shape)
    attn_weights = torch.bmm(query_states, key_states.transpose(1, 2))
    attn_weights = F.softmax(attn_weights, dim=-1)
    attn_output = torch.bmm(attn_weights, value_states)
    attn_output = attn_output.view(bsz, heads, tgt_len, head_dim).transpose(1, 2).reshape(bsz, tgt_len, embed_dim)
    return F.linear(attn_output, p["self_attn.out_proj.weight"], p["self_attn.out_proj.bias"])


def sdpa_attention(p, x, heads):
    """the same block with F.scaled_dot_product_attention in place of the bmm / softmax / bmm statements (benchmarks only)"""
    B, N, C = x.shape
    sp = lambda t: t.view(B, N, heads, C // heads).transpose(1, 2)
    q = sp(F.linear(x, p["self_attn.q_proj.weight"], p["self_attn.q_proj.bias"]))
    k = sp(F.linear(x, p["self_attn.k_proj.weight"], p["self_attn.k_proj.bias"]))
    v = sp(F.linear(x, p["self_attn.v_proj.weight"], p["self_attn.v_proj.bias"]))
    y = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, C)
    return F.linear(y, p["self_attn.out_proj.weight"], p["self_attn.out_proj.bias"])


def clip_mlp(p, x, act):
    """CLIPMLP.forward"""
    h = F.linear(x, p["mlp.fc1.weight"], p["mlp.fc1.bias"])
    h = ACT[act](h)
    return F.linear(h, p["mlp.fc2.weight"], p["mlp.fc2.bias"])


def layer(p, x, heads, act="quick_gelu", eps=EPS, attn=clip_attention):
    """CLIPEncoderLayer.forward"""
    C = x.shape[-1]
    residual = x
    h = F.layer_norm(x, (C,), p["layer_norm1.weight"], p["layer_norm1.bias"], eps)
    h = residual + attn(p, h, heads)
    residual = h
    m = F.layer_norm(h, (C,), p["layer_norm2.weight"], p["layer_norm2.bias"], eps)
    return residual + clip_mlp(p, m, act)


def tower(sd, pix, heads, n_layers, patch, act="quick_gelu", eps=EPS, prefix=""):
    """CLIPVisionTransformer.forward on a state dict with HF's names -> (hidden_states tuple of n_layers + 1, pooler_output)"""
    g = lambda k: sd[prefix + k]
    C = g("embeddings.class_embedding").numel()
    pos = g("embeddings.position_embedding.weight")
    h = embeddings(pix, g("embeddings.patch_embedding.weight"), None, g("embeddings.class_embedding").view(1, 1, C), pos.view(1, -1, C), patch)
    h = F.layer_norm(h, (C,), g("pre_layrnorm.weight"), g("pre_layrnorm.bias"), eps)
    hs = (h,)
    for i in range(n_layers):
        pre = f"{prefix}encoder.layers.{i}."
        h = layer({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, h, heads, act, eps)
        hs = hs + (h,)
    pooled = F.layer_norm(h[:, 0, :], (C,), g("post_layernorm.weight"), g("post_layernorm.bias"), eps)
    return hs, pooled


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def make_params(hidden, inter, seed=0, device="cpu"):
    """-> {state-dict key of CLIPEncoderLayer: bf16 tensor}"""
    g = torch.Generator(device=device).manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    C, I = hidden, inter
    p = {"layer_norm1.weight": 1 + 0.1 * rn(C), "layer_norm1.bias": 0.1 * rn(C)}
    for n in ("q", "k", "v", "out"):
        p[f"self_attn.{n}_proj.weight"] = rn(C, C) / math.sqrt(C)
        p[f"self_attn.{n}_proj.bias"] = 0.1 * rn(C)
    p.update({"layer_norm2.weight": 1 + 0.1 * rn(C), "layer_norm2.bias": 0.1 * rn(C),
              "mlp.fc1.weight": rn(I, C) / math.sqrt(C), "mlp.fc1.bias": 0.1 * rn(I),
              "mlp.fc2.weight": rn(C, I) / math.sqrt(I), "mlp.fc2.bias": 0.1 * rn(C)})
    return {k: v.to(torch.bfloat16) for k, v in p.items()}


def make_io(B, S, hidden, seed=0, device="cpu"):
    """-> (x, grad_out) bf16 [B, S, hidden]"""
    g = torch.Generator(device=device).manual_seed(2000 + seed)
    x = torch.randn(B, S, hidden, generator=g, device=device)
    go = torch.randn(B, S, hidden, generator=g, device=device) / math.sqrt(hidden)
    return x.to(torch.bfloat16), go.to(torch.bfloat16)


def autograd_layer(params, x, grad_out, heads, act, dtype, eps=EPS, attn=clip_attention):
    """torch autograd of ``layer`` in ``dtype`` on copies of the bf16 values -> (out, {name: grad}, x.grad)"""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = x.detach().to(dtype).requires_grad_(True)
    out = layer(p, xx, heads, act, eps, attn)
    out.backward(grad_out.to(dtype))
    return out.detach(), {k: v.grad for k, v in p.items()}, xx.grad


def autograd_layer_norm(x, w, b, grad_y, dtype, eps=EPS):
    xx, ww, bb = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    y = F.layer_norm(xx, (x.shape[-1],), ww, bb, eps)
    y.backward(grad_y.to(dtype))
    return y.detach(), xx.grad, ww.grad, bb.grad


def norm_case(rows, C, seed=0, device="cpu"):
    """-> x, grad_y, grad_res [rows, C], w [C] (bf16) for the row-wise kernel"""
    g = torch.Generator(device=device).manual_seed(3000 + seed + rows + C)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    bf = lambda t: t.to(torch.bfloat16)
    return bf(rn(rows, C) * 1.5), bf(rn(rows, C)), bf(rn(rows, C)), bf(1 + 0.1 * rn(C))


# ---- the row-wise kernel: fp64 reference, bounds, fp32 emulation ----------------------------------------------------------------------
def ln_bwd_ref(x, gy, w, gres=None, eps=EPS):
    """fp64 backward of y = w xhat + b -> (grad_x, grad_w, grad_b, mag_x, mag_w, mag_b)"""
    x, gy, w = x.double(), gy.double(), w.double()
    mean = x.mean(-1, keepdim=True)
    r = torch.rsqrt((x - mean).pow(2).mean(-1, keepdim=True) + eps)
    xh, g = (x - mean) * r, gy * w
    gx = r * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    mag_x = 4 * r * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    if gres is not None:
        gx = gx + gres.double()
        mag_x = mag_x + gres.double().abs()
    return gx, (gy * xh).sum(0), gy.sum(0), mag_x, (gy * xh).abs().sum(0), gy.abs().sum(0)


def emulate_ln_bwd(x, gy, w, gres=None, eps=EPS):
    """the kernel's arithmetic in fp32 -> bf16 (grad_x, grad_w, grad_b)"""
    x, gy, w = x.float(), gy.float(), w.float()
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    d = x - mean
    r = torch.rsqrt(d.pow(2).sum(-1, keepdim=True) / C + eps)
    xh = d * r
    g = gy * w
    gx = r * (g - g.sum(-1, keepdim=True) / C - xh * ((g * xh).sum(-1, keepdim=True) / C))
    if gres is not None:
        gx = gx + gres.float()
    return gx.to(torch.bfloat16), (gy * xh).sum(0).to(torch.bfloat16), gy.sum(0).to(torch.bfloat16)


def quick_gelu_grad_ref(h):
    """fp64 q'(h) = s (1 + 1.702 h (1 - s)), s = sigmoid(1.702 h)"""
    h = h.double()
    s = torch.sigmoid(1.702 * h)
    return s * (1 + 1.702 * h * (1 - s))


def emulate_quick_gelu_grad(h):
    """the epilogue's arithmetic in fp32: s = 1 / (1 + 2^(-1.702 log2(e) h)), s * fma(1.702 h, 1 - s, 1)"""
    h = h.float()
    s = 1.0 / (1.0 + torch.exp2(torch.tensor(-1.702 * 1.4426950408889634, dtype=torch.float32) * h))
    return s * (1.702 * h * (1.0 - s) + 1.0)
