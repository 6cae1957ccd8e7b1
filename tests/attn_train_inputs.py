"""Inputs, yardstick and bounds of the attention training tests (test_attn_train_cpu.py, test_attn_train_gpu.py).

The yardstick is torch's fp64 autograd of the reference's ``_naive_attn`` statements (modeling_intern_vit.py:136-140:
``((q * scale) @ k^T).softmax(-1) @ v``) on the 16-bit-rounded inputs; it never calls the code under test.  The bounds have the form
and the constants of the forward's tests (eps = 2^-8 bf16 / 2^-10 fp16, ``ulp`` = the format's spacing at the fp64 value):

    |d dV_j| <= ulp + eps sum_i p_ij |dO_i|
    |d dQ_i| <= ulp + scale sum_j (eps |dS_ij| + p_ij e_i) |k_j|,   e_i = eps sum_d |dO_id| |O_id|   (delta reads the rounded out)
    |d dK_j| <= ulp + scale sum_i (eps |dS_ij| + p_ij e_i) |q_i|
    |d lse_i| <= 2^-8 (bf16) / 2^-11 (fp16)    (the row sum adds terms rounded to 2^-9 / 2^-12 relative; x 2 for fp32 exp2 / log2)

``emulate`` walks the algorithm's rounding points on the CPU (row sum over rounded probabilities, rounded ``out`` in delta, P and dS
rounded as operands -- in IEEE half times 2^14 / 2^4, an exact scale that keeps a probability of e^-18 out of half's subnormals,
where rounding stops being relative and the eps form of the bounds stops describing it -- one final rounding):
test_attn_train_cpu.py keeps it inside the bounds on every case, so the bounds are ones a faithful implementation meets.
Nothing here touches torch.cuda at import."""
import functools

import torch

import bounds

CASES = ("random", "spiked_key", "key0_dominant", "key0_far_below", "near_one_hot")


def eps_of(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -10


def lse_bound(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


def ulp_of(ref, dtype):
    """Spacing of ``dtype`` at the fp64 value (normal range; floored at the smallest normal's spacing)."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))) - mant)


def round16(x, dtype):
    return x.to(torch.float32).to(dtype).to(torch.float64)


def case(name, B, S, H, D, dtype, seed=0):
    """-> (qkv [B, S, 3, H, D], grad_out [B, S, H, D]) in ``dtype`` on the CPU."""
    g = torch.Generator().manual_seed(seed * 7919 + S * 31 + D)
    qkv = torch.randn(B, S, 3, H, D, generator=g) * 0.5
    dout = torch.randn(B, S, H, D, generator=g)
    u = torch.nn.functional.normalize(torch.randn(B, 1, H, D, generator=g), dim=-1) * (3.0 * D ** 0.25)   # (q . u) d^-1/2 = +-9
    if name == "random":
        pass
    elif name == "spiked_key":          # a key in a middle tile aligned with the direction every query shares
        qkv[:, :, 0] += u
        qkv[:, S // 2, 1] = u[:, 0]
    elif name == "key0_dominant":       # the class-token extremes of test_attention_class_token_as_initial_state_extremes
        qkv[:, :, 0] += u
        qkv[:, 0, 1] = u[:, 0]
    elif name == "key0_far_below":
        qkv[:, :, 0] += u
        qkv[:, 0, 1] = -u[:, 0]
    elif name == "near_one_hot":        # query i points along key (7 i) % S with scale q.k ~ 20: p is one-hot to ~e^-12, dS -> 0
        idx = (torch.arange(S) * 7) % S
        qkv[:, :, 0] = 40.0 * torch.nn.functional.normalize(qkv[:, idx, 1], dim=-1)
    else:
        raise KeyError(name)
    return qkv.to(dtype), dout.to(dtype)


def _split(qkv):
    """[B, S, 3, H, D] -> q, k, v as [B, H, S, D] fp64."""
    return qkv.double().permute(2, 0, 3, 1, 4).unbind(0)


def naive_attn(q, k, v, scale):
    """modeling_intern_vit.py:136-140 (attn_drop is the identity), [B, H, S, D] -> [B, S, H, D]."""
    attn = ((q * scale) @ k.transpose(-2, -1))
    attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2)


def autograd_grads(qkv, dout, scale, dtype):
    """-> (out, grad_qkv) by torch's autograd of ``naive_attn`` in ``dtype`` (fp64: the yardstick; bf16 / fp16: torch's own 16-bit
    training path, the other side of the whole-tensor parity contract)."""
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
    out = naive_attn(q, k, v, scale)
    out.backward(dout.to(dtype))
    return out.detach(), x.grad


def closed_form(qkv, dout, scale, out_for_delta=None):
    """The flash backward's expressions in fp64 -> dict(p, lse, out, delta, dS, dqkv).  ``out_for_delta``: the (rounded) out delta reads."""
    q, k, v = _split(qkv)
    do = dout.double().permute(0, 2, 1, 3)
    s = scale * (q @ k.transpose(-2, -1))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = p @ v
    o = out if out_for_delta is None else out_for_delta.double().permute(0, 2, 1, 3)
    delta = (do * o).sum(-1)
    dS = p * (do @ v.transpose(-2, -1) - delta[..., None])
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-2, -1) @ q), p.transpose(-2, -1) @ do
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4)
    return dict(p=p, lse=lse, out=out.transpose(1, 2), delta=delta, dS=dS, dqkv=dqkv)


def grad_bounds(qkv, dout, scale, dtype):
    """-> (ref fp64 grad_qkv [B, S, 3, H, D], per-element bound of the same shape, lse fp64 [B, H, S])."""
    eps = eps_of(dtype)
    c = closed_form(qkv, dout, scale)
    q, k, v = _split(qkv)
    do = dout.double().permute(0, 2, 1, 3)
    p, dS = c["p"], c["dS"]
    e = eps * (do.abs() * c["out"].transpose(1, 2).abs()).sum(-1)          # [B, H, S]
    w = eps * dS.abs() + p * e[..., None]
    bq = scale * (w @ k.abs())
    bk = scale * (w.transpose(-2, -1) @ q.abs())
    bv = eps * (p.transpose(-2, -1) @ do.abs())
    ref = c["dqkv"]
    mag = torch.stack([bq, bk, bv], 0).permute(1, 3, 0, 2, 4)
    return ref, ulp_of(ref, dtype) + mag, c["lse"]


def emulate(qkv, dout, scale, dtype):
    """The algorithm with its rounding points, in fp64 between them -> (out, lse, grad_qkv), out and grad_qkv rounded to ``dtype``."""
    q, k, v = _split(qkv)
    do = dout.double().permute(0, 2, 1, 3)
    s = scale * (q @ k.transpose(-2, -1))
    m = s.max(-1, keepdim=True).values
    pr = round16(torch.exp(s - m), dtype)
    l = pr.sum(-1, keepdim=True)                     # the forward's row sum: over the ROUNDED probabilities
    lse = (m + torch.log(l))[..., 0]
    out = round16((pr @ v) / l, dtype)
    p = torch.exp(s - lse[..., None])
    delta = (do * out).sum(-1)                       # delta from the rounded out
    kp, ks = (2.0 ** 14, 2.0 ** 4) if dtype == torch.float16 else (1.0, 1.0)     # half: the operands' exact power-of-two scales
    dv = (round16(p * kp, dtype) / kp).transpose(-2, -1) @ do    # P rounded as an operand
    dS = round16(p * (do @ v.transpose(-2, -1) - delta[..., None]) * ks, dtype) / ks   # dS rounded as an operand
    dq, dk = scale * (dS @ k), scale * (dS.transpose(-2, -1) @ q)
    dqkv = round16(torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4), dtype)   # one final rounding
    return out.transpose(1, 2), lse, dqkv


def worst_factor(got, ref, bound):
    """max over elements of |got - ref| / bound (<= 1 passes) and where."""
    r = ((got.double() - ref).abs() / bound)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.flatten()[i]), i


rel_rms = functools.partial(bounds.rel_rms, clamp=True)
