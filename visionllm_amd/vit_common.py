"""Shared host logic of the two vision-encoder mirrors (InternViT, CLIP): parameter packing into the C ABI
descriptor, hidden-state allocation, the forward call."""
import ctypes

import torch

from . import _lib


def _require_bf16_cuda(name, t):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor: the native vision encoder has no CPU path")
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"{name} must be bfloat16 (got {t.dtype}); load the model with torch_dtype=torch.bfloat16 "
                           "as the reference does (train/train.py:375)")


class EncoderPlan:
    """Device pointers of every parameter, packed once and refreshed when a parameter changes."""

    def __init__(self):
        self.key = None
        self.desc = None
        self.layers = None
        self.keep = []  # tensors owned by the plan (padded / fused copies)

    @staticmethod
    def signature(params):
        return tuple((p.data_ptr(), p._version, p.dtype, p.device) for p in params)


def plan_ptr(plan):
    """-> P(t): device pointer of parameter ``t`` for the descriptor.  The kernels read parameters as 16-byte vectors; a parameter
    that is a view at another storage offset (weights loaded into one packed buffer) is copied once into an aligned tensor that
    the plan keeps (the plan is rebuilt when a parameter's pointer or version changes)."""
    def P(t):
        if t is None:
            return None
        a = _lib.aligned(t.detach())
        if a.data_ptr() != t.data_ptr():
            plan.keep.append(a)
        return _lib.ptr(a)
    return P


def padded_patch_weight(conv_weight, kpad):
    """Conv2d weight [C,3,ps,ps] -> [C, kpad] (k = c*ps*ps + ky*ps + kx, zero padded)."""
    C = conv_weight.shape[0]
    w = conv_weight.detach().reshape(C, -1)
    out = torch.zeros((C, kpad), dtype=w.dtype, device=w.device)
    out[:, : w.shape[1]] = w
    return out


def fold_norm_into_linear(w, b, gamma, beta, layernorm):
    """Operands of a linear layer with the norm in front of it folded in (vllm_gemm_bf16_ln, consumer side):
        linear(norm(x)) = r (x W'^T) - r mean colsum + bias'      W' = W diag(gamma)  (bf16),
        colsum_n = sum_k W'[n, k]  (fp32, from the ROUNDED W': the mean shift then cancels exactly for the weights in use),
        bias'_n = b_n + sum_k beta_k W[n, k]  (fp32).
    RMSNorm (layernorm=False) has no mean and no beta: colsum is None, bias' is b.  -> (w_ln, colsum, bias_ln)"""
    w32 = w.detach().float()
    w_ln = (w32 * gamma.detach().float()[None, :]).to(torch.bfloat16).contiguous()
    colsum = w_ln.float().sum(1).contiguous() if layernorm else None
    bias_ln = b.detach().float().clone() if b is not None else None
    if beta is not None:
        shift = w32 @ beta.detach().float()
        bias_ln = shift if bias_ln is None else bias_ln + shift
    return w_ln, colsum, (bias_ln.contiguous() if bias_ln is not None else None)


def norm_folding_applies(hidden_size, intermediate_size, rms=False):
    """The encoder folds its norms into the GEMMs around them
      * at hidden size 1024 (ViT-L, InternViT-300M: rows of exactly four 256-column tiles, LayerNorm or RMSNorm), and
      * round 5: for RMSNorm at any hidden size of up to 16 column tiles that is a multiple of 8 (InternViT-6B: 3200 = 12.5 tiles;
        `rms=True`), where the C side keeps the launched norms for batches too small for the persistent GEMM schedule.
    The C side also asks for >= 1024 tokens per call; VLLM_LN_FOLD=0 keeps the norm launches (A/B).  The prepared operands are one
    more bf16 copy of the qkv and fc1 weights (InternViT-6B: 6.9 GB over 48 layers)."""
    import os
    if os.environ.get("VLLM_LN_FOLD", "1") == "0" or intermediate_size < 1024:
        return False
    return hidden_size == 1024 or (rms and hidden_size % 8 == 0 and hidden_size <= 4096 and os.environ.get("VLLM_LN_FOLD_WIDE", "1") != "0")


def kpad_for(patch):
    k = 3 * patch * patch
    return (k + 63) // 64 * 64


def _embed_desc(pix, w, b, cls, pos, keep):
    """VllmVitEmbed for the parameters as the modules store them: conv weight [C, 3, ps, ps], bias [C] or None, class embedding
    (C elements), position table ([1 + P, C] elements).  The tile size is the position table's (resize_pos_embeddings may have
    changed it, as in _build_plan)."""
    C, ps = w.shape[0], w.shape[-1]
    S = pos.numel() // C
    g = int(round((S - 1) ** 0.5))
    if g * g != S - 1:
        raise ValueError(f"position table of {S} rows is not 1 + a square grid")
    fields = {}
    for name, t in (("patch_w", w), ("patch_b", b), ("cls", cls), ("pos", pos)):
        if t is None:
            fields[name] = None
            continue
        _require_bf16_cuda(name, t)
        a = _lib.aligned(t.detach())
        keep.append(a)
        fields[name] = a.data_ptr()
    return _lib.VllmVitEmbed(hidden=C, patch=ps, image=g * ps, pixel_is_f32=1 if pix.dtype == torch.float32 else 0, **fields), S


def _embed_workspace(L, d, n, dev):
    return _lib.sized_workspace(dev, L.vllm_vit_embed_workspace_bytes(ctypes.byref(d), n), "vllm_vit_embed_workspace_bytes")


def _embed_forward(pix, w, b, cls, pos):
    keep = []
    d, S = _embed_desc(pix, w, b, cls, pos, keep)
    if pix.dim() != 4 or pix.shape[1] != 3 or pix.shape[2] != d.image or pix.shape[3] != d.image:
        raise ValueError(f"pixel_values must be [n, 3, {d.image}, {d.image}], got {tuple(pix.shape)}")
    L = _lib.lib()
    n, dev = pix.shape[0], pix.device
    out = torch.empty((n, S, d.hidden), dtype=torch.bfloat16, device=dev)
    with torch.cuda.device(dev):
        ws, wsb = _embed_workspace(L, d, n, dev)
        _lib.check(L.vllm_vit_embed_forward(ctypes.byref(d), _lib.ptr(pix), n, _lib.ptr(out), _lib.ptr(ws), wsb, _lib.current_stream(dev)),
                   "vllm_vit_embed_forward")
    return out


class _EmbedTrain(torch.autograd.Function):
    """The embeddings of a vision tower as one autograd node: vllm_vit_embed_forward (the no-grad call's bits) /
    vllm_vit_embed_backward.  Pixels and parameters go through save_for_backward, so an in-place update between forward and backward
    fails autograd's version check; a parameter that does not need its gradient is a NULL pointer (that work is skipped)."""

    @staticmethod
    def forward(ctx, pix, w, b, cls, pos):
        ctx.save_for_backward(pix, w, b, cls, pos)
        return _embed_forward(pix, w, b, cls, pos)

    @staticmethod
    def backward(ctx, gout):
        pix, w, b, cls, pos = ctx.saved_tensors
        keep = []
        d, _ = _embed_desc(pix, w, b, cls, pos, keep)
        n, dev = pix.shape[0], pix.device
        g = _lib.aligned(gout.to(torch.bfloat16))
        need = ctx.needs_input_grad
        grads = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) if (k and p is not None) else None
                 for k, p in zip(need[1:], (w, b, cls, pos))]
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws, wsb = _embed_workspace(L, d, n, dev)
            _lib.check(L.vllm_vit_embed_backward(ctypes.byref(d), _lib.ptr(pix), n, _lib.ptr(g), *[_lib.ptr(t) for t in grads], _lib.ptr(ws), wsb,
                                                 _lib.current_stream(dev)), "vllm_vit_embed_backward")
        return (None,) + tuple(grads)


class LayerTrainABI:
    """What the autograd nodes of the two encoder-layer families share: the calls of vllm_<family>_layer_forward_train /
    vllm_<family>_layer_backward around the family's three structs.  ``params`` / ``saved``: the member names of the descriptor's
    parameter pointers (= those of the gradient table) and of the saved table, in the structs' order.  ``scalars`` of a call are the
    descriptor's remaining members but ``hidden`` (heads, inter, eps, CLIP: act)."""

    _BIAS_RIDES_ON = (("qkv_b", "qkv_w"), ("proj_b", "proj_w"), ("fc1_b", "fc1_w"), ("fc2_b", "fc2_w"))

    def __init__(self, family, desc_cls, saved_cls, grads_cls, params, saved):
        self.desc_cls, self.saved_cls, self.grads_cls, self.params, self.saved = desc_cls, saved_cls, grads_cls, params, saved
        self.ws_query, self.fwd, self.bwd = (f"vllm_{family}_layer_{n}" for n in ("backward_workspace_bytes", "forward_train", "backward"))

    def desc(self, scalars, params, keep):
        """The descriptor for bf16 CUDA parameters in ``self.params`` order (None: the layer has none); ``keep`` receives the 16-byte
        aligned tensors whose pointers it holds."""
        fields = {}
        for name, t in zip(self.params, params):
            if t is None:
                fields[name] = None
                continue
            _require_bf16_cuda(name, t)
            a = _lib.aligned(t.detach())
            keep.append(a)
            fields[name] = a.data_ptr()
        return self.desc_cls(hidden=params[0].shape[0], **scalars, **fields)

    def _call(self, entry, d, x, *args):
        B, S, _ = x.shape
        dev = x.device
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws, wsb = _lib.sized_workspace(dev, getattr(L, self.ws_query)(ctypes.byref(d), B, S), self.ws_query)
            _lib.check(getattr(L, entry)(ctypes.byref(d), _lib.ptr(x), B, S, *args, _lib.ptr(ws), wsb, _lib.current_stream(dev)), entry)

    def _saved_table(self, saved):
        return ctypes.byref(self.saved_cls(**{n: t.data_ptr() for n, t in zip(self.saved, saved)}))

    def forward(self, scalars, x, params):
        """The training forward on x [B, S, C] (16-byte aligned) -> (out, the saved tensors in ``self.saved`` order)."""
        keep = []
        d = self.desc(scalars, params, keep)
        B, S, C = x.shape
        M, dev = B * S, x.device
        shapes = {"qkv": (M, 3 * C), "lse": (B, scalars["heads"], S), "h1": (M, scalars["inter"]), "a1": (M, scalars["inter"])}   # others: [M, C]
        out = torch.empty((B, S, C), dtype=torch.bfloat16, device=dev)
        saved = [torch.empty(shapes.get(n, (M, C)), dtype=torch.float32 if n == "lse" else torch.bfloat16, device=dev) for n in self.saved]
        self._call(self.fwd, d, x, _lib.ptr(out), self._saved_table(saved))
        return out, saved

    def backward(self, scalars, x, saved, params, gout, need_x, need):
        """-> (grad_x or None, the parameter gradients in ``self.params`` order: None where ``need`` is false or the layer has no such
        parameter)."""
        keep = []
        d = self.desc(scalars, params, keep)
        idx = {n: i for i, n in enumerate(self.params)}
        ask = list(need)
        for b, w in self._BIAS_RIDES_ON:   # a bias gradient rides on its weight's launch
            ask[idx[w]] = ask[idx[w]] or (ask[idx[b]] and params[idx[b]] is not None)
        g = _lib.aligned(gout.to(torch.bfloat16))
        grads = [torch.empty(p.shape, dtype=torch.bfloat16, device=x.device) if (a and p is not None) else None for a, p in zip(ask, params)]
        gx = torch.empty_like(x) if need_x else None
        gs = self.grads_cls(**{n: (t.data_ptr() if t is not None else None) for n, t in zip(self.params, grads)})
        self._call(self.bwd, d, x, _lib.ptr(g), self._saved_table(saved), _lib.ptr(gx), ctypes.byref(gs))
        return gx, [t if n else None for t, n in zip(grads, need)]   # (a weight gradient computed only as its bias's carrier is dropped)


def embed_pixels(pixel_values, conv, class_embedding, position_table):
    """InternVisionEmbeddings.forward (modeling_intern_vit.py:82-90) / HF CLIPVisionEmbeddings.forward on a CUDA tensor
    [n, 3, image, image] (bf16 or fp32; other floating dtypes are cast to bf16 as run_encoder does) -> [n, 1 + P, C] bf16.  One
    autograd node when grad is enabled and a parameter requires grad, a plain call otherwise: the same bits."""
    if not pixel_values.is_cuda:
        raise RuntimeError("pixel_values must be a CUDA tensor: the native vision encoder has no CPU path")
    if pixel_values.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("gradients with respect to pixel_values are not implemented (nothing in the model asks for them); "
                                  "detach pixel_values")
    if pixel_values.dtype not in (torch.bfloat16, torch.float32):
        pixel_values = pixel_values.to(torch.bfloat16)
    pix = pixel_values.detach().contiguous()
    params = (conv.weight, conv.bias, class_embedding, position_table)
    if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in params):
        return _EmbedTrain.apply(pix, *params)
    return _embed_forward(pix, *[p.detach() if p is not None else None for p in params])


def run_encoder(desc, pixel_values, num_layers, hidden_size, keep=None):
    """Allocate hidden states and call vllm_vit_forward.  ``keep``: None = materialise all L+1 states (what the
    reference does with output_hidden_states=True), or an iterable of indices (negative allowed) to keep."""
    lib = _lib.lib()
    if pixel_values.dim() != 4 or pixel_values.shape[1] != 3:
        raise ValueError(f"wrong pixel_values size: {tuple(pixel_values.shape)}")
    if not pixel_values.is_cuda:
        raise RuntimeError("pixel_values must be a CUDA tensor: the native vision encoder has no CPU path")
    if pixel_values.shape[2] != desc.image or pixel_values.shape[3] != desc.image:
        raise ValueError(f"pixel_values must be {desc.image}x{desc.image}, got {tuple(pixel_values.shape[2:])}")
    if pixel_values.dtype not in (torch.bfloat16, torch.float32):
        pixel_values = pixel_values.to(torch.bfloat16)
    pixel_values = pixel_values.contiguous()
    desc.pixel_is_f32 = 1 if pixel_values.dtype == torch.float32 else 0
    n = pixel_values.shape[0]
    g = desc.image // desc.patch
    S = g * g + 1
    dev = pixel_values.device
    L = num_layers
    if keep is None:
        want = set(range(L + 1))
    else:
        want = {(i + L + 1) % (L + 1) for i in keep} | {L}
    states = [torch.empty((n, S, hidden_size), dtype=torch.bfloat16, device=dev) if i in want else None
              for i in range(L + 1)]
    # Tiles never interact inside the encoder, so a batch CAN be run as independent chunks on separate streams (opt-in:
    # set_encoder_chunks / VLLM_ENCODER_CHUNKS), the idea being that kernels of the other chunk fill the CUs a GEMM / attention
    # launch leaves idle in its last round of tiles.  Same kernels, same per-tile arithmetic: results are bit-identical
    # (tested).  Measured on the bench workload (40 tiles ViT-L): 24.08 ms per step with two half-batches against 22.65 ms
    # with one sequence -- the half-size GEMMs quantise worse than the overlap recovers -- so the default is ONE chunk.
    chunks = encoder_chunks(n)
    bounds = [n * c // chunks for c in range(chunks + 1)]
    row_bytes = S * hidden_size * 2
    px_bytes = 3 * desc.image * desc.image * pixel_values.element_size()
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        for c in range(chunks):
            lo, nc = bounds[c], bounds[c + 1] - bounds[c]
            if nc == 0:
                continue
            ptrs = (ctypes.c_void_p * (L + 1))(*[s.data_ptr() + lo * row_bytes if s is not None else None for s in states])
            ws, ws_bytes = _lib.sized_workspace(dev, lib.vllm_vit_workspace_bytes(ctypes.byref(desc), nc), "vllm_vit_workspace_bytes", slot=c)
            stream = main if c == 0 else _side_stream(dev, c)
            if c > 0:
                stream.wait_stream(main)   # inputs (and the workspace's previous users) are ordered on the caller's stream
            with torch.cuda.stream(stream):
                _lib.check(lib.vllm_vit_forward(ctypes.byref(desc), ctypes.c_void_p(pixel_values.data_ptr() + lo * px_bytes), nc,
                                                ptrs, _lib.ptr(ws), ws_bytes, _lib.current_stream(dev)), "vllm_vit_forward")
        for c in range(1, chunks):
            main.wait_stream(_side_stream(dev, c))
    return states


_ENCODER_CHUNKS = {"value": None}
_SIDE_STREAMS = {}


def set_encoder_chunks(k):
    """1 (default, also None): one launch sequence per batch; k: k chunks of tiles on k streams (measured slower)."""
    old = _ENCODER_CHUNKS["value"]
    _ENCODER_CHUNKS["value"] = k
    return old


def encoder_chunks(n):
    import os
    k = _ENCODER_CHUNKS["value"]
    if k is None:
        env = os.environ.get("VLLM_ENCODER_CHUNKS")
        k = int(env) if env else 1
    return max(1, min(int(k), n, 4))


def _side_stream(dev, c):
    key = (str(dev), c)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


class LazyHiddenStates(tuple):
    """Tuple of L+1 hidden states; entries that were not materialised are None (only with keep=...)."""


def model_output(last_hidden_state, pooler_output, hidden_states, return_dict=True):
    if not return_dict:
        return (last_hidden_state, pooler_output) + ((hidden_states,) if hidden_states is not None else ())
    try:
        from transformers.modeling_outputs import BaseModelOutputWithPooling
        return BaseModelOutputWithPooling(last_hidden_state=last_hidden_state, pooler_output=pooler_output,
                                          hidden_states=hidden_states, attentions=None)
    except Exception:  # transformers not importable: a minimal stand-in with the attributes the caller reads
        from types import SimpleNamespace
        return SimpleNamespace(last_hidden_state=last_hidden_state, pooler_output=pooler_output,
                               hidden_states=hidden_states, attentions=None)
