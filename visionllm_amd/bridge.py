"""Visual-token projector ("vl_bridge") + hidden-state select + pixel-shuffle: boundary B2.

Mirrors VisionLLMv2/visionllmv2/model/modeling_visionllmv2.py:157-190 (construction: ``linear``,
``internvl_mlp``/``internvl`` = LayerNorm, Linear, GELU, Linear; ``mlp{N}x_gelu``), :381-392 (``pixel_shuffle``)
and :569-579 (select ``hidden_states[vis_output_layer][:, 1:]``, optional pixel-shuffle, bridge).

``build_vl_bridge`` returns an ``nn.Linear`` / ``nn.Sequential`` subclass with the SAME child indices, so
``vl_bridge.{idx}.weight/bias`` state-dict keys (and ``vl_bridge.bin`` files, :185-190) load unchanged; its
``forward(x)`` takes what the reference passes (``image_features_ori`` [n, T, C_in]).  ``project_hidden_state`` is the
fused path used by our own pipeline: it reads the selected hidden state [n, 1+T, C] directly (CLS rows are skipped
inside the GEMM loader / pixel-shuffle gather) and writes [n, T', C_llm].
"""
import ctypes
import re

import torch
from torch import nn

from . import _lib


def pixel_shuffle(x, scale_factor=0.5):
    """[n, w, h, c] -> [n, w/2, h/2, 4c] (modeling_visionllmv2.py:381-392), one gather kernel."""
    if scale_factor != 0.5:
        raise NotImplementedError("only scale_factor=0.5 is used by VisionLLMv2")
    if not x.is_cuda or x.dtype != torch.bfloat16:
        raise RuntimeError("pixel_shuffle: bf16 CUDA tensor required (no CPU path)")
    n, w, h, c = x.shape
    if w != h:
        raise ValueError("pixel_shuffle: square token grid expected")
    x = _lib.aligned(x)   # (16-byte aligned rows: a view at another storage offset is copied)
    out = torch.empty((n, w // 2, h // 2, 4 * c), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vllm_pixel_shuffle_bf16(_lib.ptr(x), w * h * c, c, 0, _lib.ptr(out), n, w, c,
                                                      _lib.current_stream(x.device)), "vllm_pixel_shuffle_bf16")
    return out


def _desc_for(mod, kind, pixel_shuffle_flag, skip_cls, keep):
    """-> descriptor of the projector's parameters.  The GEMMs and the LayerNorm read them as 16-byte vectors: a parameter that is
    a view at another storage offset is passed as an aligned copy, appended to ``keep`` (alive until the launch is enqueued)."""
    def P(t):
        if t is None:
            return None
        a = _lib.aligned(t.detach())
        if a.data_ptr() != t.data_ptr():
            keep.append(a)
        return _lib.ptr(a)
    if kind == "linear":
        lin = [mod]
        ln = None
        k = _lib.BRIDGE_LINEAR
    elif kind in ("internvl_mlp", "internvl"):
        ln, lin, k = mod[0], [mod[1], mod[3]], _lib.BRIDGE_INTERNVL_MLP
    else:
        lin, ln, k = [m for m in mod if isinstance(m, nn.Linear)], None, _lib.BRIDGE_MLP_GELU
    for m in lin + ([ln] if ln is not None else []):
        for p in m.parameters():
            if not p.is_cuda or p.dtype != torch.bfloat16:
                raise RuntimeError("vl_bridge parameters must be bf16 CUDA tensors (no CPU path)")
    d = _lib.VllmBridgeDesc(kind=k, depth=len(lin), in_features=lin[0].in_features, out_features=lin[-1].out_features,
                            pixel_shuffle=int(pixel_shuffle_flag), skip_cls=int(skip_cls),
                            ln_eps=ln.eps if ln is not None else 0.0, ln_w=P(ln.weight) if ln is not None else None,
                            ln_b=P(ln.bias) if ln is not None else None)
    for i, m in enumerate(lin):
        d.w[i] = P(m.weight).value
        d.b[i] = P(m.bias).value if m.bias is not None else None
    return d


def _run(desc, hidden, n, T, C):
    lib = _lib.lib()
    T_out = T // 4 if desc.pixel_shuffle else T
    out = torch.empty((n, T_out, desc.out_features), dtype=torch.bfloat16, device=hidden.device)
    with torch.cuda.device(hidden.device):
        ws, wsb = _lib.sized_workspace(hidden.device, lib.vllm_bridge_workspace_bytes(ctypes.byref(desc), n, T), "vllm_bridge_workspace_bytes")
        _lib.check(lib.vllm_bridge_forward(ctypes.byref(desc), _lib.ptr(hidden), n, T, C, _lib.ptr(out), _lib.ptr(ws),
                                           wsb, _lib.current_stream(hidden.device)), "vllm_bridge_forward")
    return out


class _BridgeMixin:
    vl_bridge_type = "linear"

    def _native(self, x, pixel_shuffle_flag=False, skip_cls=False):
        if not x.is_cuda or x.dtype != torch.bfloat16:
            raise RuntimeError("vl_bridge: bf16 CUDA input required (no CPU path)")
        if _trains(self, x):
            # the fused select / CLS-skip / pixel-shuffle path has no backward and its output no grad_fn: refuse loudly instead of
            # silently cutting the gradient (forward(x) is the training entry, modeling_visionllmv2.py:579)
            raise RuntimeError("vl_bridge.project_hidden_state (native): the fused select / pixel-shuffle path is inference-only -- "
                               "call it under torch.no_grad() or with the projector and its input frozen; train the projector "
                               "through forward(x), which has a native backward")
        x = _lib.aligned(x)   # (the GEMM loaders need 16-byte aligned rows: a view at another storage offset is copied)
        n, rows, C = x.shape
        T = rows - 1 if skip_cls else rows
        keep = []
        return _run(_desc_for(self, self.vl_bridge_type, pixel_shuffle_flag, skip_cls, keep), x, n, T, C)

    def forward(self, x):  # what modeling_visionllmv2.py:579 calls
        if _trains(self, x):
            return self._train_forward(x)
        lead = x.shape[:-2] if x.dim() > 3 else None
        if x.dim() == 2:
            return self._native(x[None])[0]
        if lead is not None:
            x = x.reshape(-1, *x.shape[-2:])
        y = self._native(x)
        return y.reshape(*lead, *y.shape[-2:]) if lead is not None else y

    def project_hidden_state(self, hidden_state, use_pixelshuffle=False):
        """hidden_state [n, 1+T, C] (a hidden_states[vis_output_layer] entry) -> [n, T or T/4, C_llm]."""
        return self._native(hidden_state, use_pixelshuffle, True)

    def _train_forward(self, x):
        """forward(x) with grad: vllm_bridge_forward_train / vllm_bridge_backward through _BridgeTrain (same output bits as the
        no-grad call)."""
        if not x.is_cuda or x.dtype != torch.bfloat16:
            raise RuntimeError("vl_bridge: bf16 CUDA input required (no CPU path)")
        lin, ln = _modules(self, self.vl_bridge_type)
        params = [t for m in lin for t in (m.weight, m.bias)] + ([ln.weight, ln.bias] if ln is not None else [])
        C = x.shape[-1]
        x2 = _lib.aligned(x.reshape(-1, C))   # (16-byte aligned rows: a view at another storage offset is copied -- differentiably)
        y = _BridgeTrain.apply(self.vl_bridge_type, len(lin), ln.eps if ln is not None else 0.0, x2, *params)
        return y.reshape(*x.shape[:-1], y.shape[-1])


def _trains(mod, x):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in mod.parameters()))


def _modules(mod, kind):
    """-> (the Linear modules, the LayerNorm or None) of a projector built by build_vl_bridge."""
    if kind == "linear":
        return [mod], None
    if kind in ("internvl_mlp", "internvl"):
        return [mod[1], mod[3]], mod[0]
    return [m for m in mod if isinstance(m, nn.Linear)], None


def _ptr_array(ts):
    return (ctypes.c_void_p * 4)(*([t.data_ptr() if t is not None else None for t in ts] + [None] * (4 - len(ts))))


class _BridgeTrain(torch.autograd.Function):
    """The projector as one autograd node.  Inputs: x [rows, in_features] (16-byte aligned) and the parameters
    (weight_0, bias_0, ..., [ln_weight, ln_bias]; a missing bias is None).  The parameters are saved with save_for_backward, so an
    in-place update between forward and backward fails autograd's version check instead of producing wrong gradients."""

    @staticmethod
    def _desc(kind, depth, eps, params, keep):
        lin_w, lin_b = params[0:2 * depth:2], params[1:2 * depth:2]
        ln_w, ln_b = (params[2 * depth], params[2 * depth + 1]) if len(params) > 2 * depth else (None, None)

        def P(t):
            if t is None:
                return None
            if not t.is_cuda or t.dtype != torch.bfloat16:
                raise RuntimeError("vl_bridge parameters must be bf16 CUDA tensors (no CPU path)")
            a = _lib.aligned(t.detach())
            keep.append(a)
            return a.data_ptr()
        k = (_lib.BRIDGE_LINEAR if kind == "linear" else _lib.BRIDGE_INTERNVL_MLP if kind in ("internvl_mlp", "internvl")
             else _lib.BRIDGE_MLP_GELU)
        d = _lib.VllmBridgeDesc(kind=k, depth=depth, in_features=lin_w[0].shape[1], out_features=lin_w[-1].shape[0],
                                pixel_shuffle=0, skip_cls=0, ln_eps=eps, ln_w=P(ln_w), ln_b=P(ln_b))
        for i in range(depth):
            d.w[i] = P(lin_w[i])
            d.b[i] = P(lin_b[i])
        return d

    @staticmethod
    def forward(ctx, kind, depth, eps, x, *params):
        keep = []
        d = _BridgeTrain._desc(kind, depth, eps, params, keep)
        rows, cout, dev = x.shape[0], d.out_features, x.device
        L = _lib.lib()
        out = torch.empty((rows, cout), dtype=torch.bfloat16, device=dev)
        pre = [torch.empty((rows, cout), dtype=torch.bfloat16, device=dev) for _ in range(depth - 1)]
        act = [torch.empty((rows, cout), dtype=torch.bfloat16, device=dev) for _ in range(depth - 1)]
        ln = torch.empty((rows, d.in_features), dtype=torch.bfloat16, device=dev) if d.kind == _lib.BRIDGE_INTERNVL_MLP else None
        with torch.cuda.device(dev):
            ws, wsb = _lib.sized_workspace(dev, L.vllm_bridge_backward_workspace_bytes(ctypes.byref(d), rows, 0),
                                           "vllm_bridge_backward_workspace_bytes")
            _lib.check(L.vllm_bridge_forward_train(ctypes.byref(d), _lib.ptr(x), rows, _lib.ptr(out), _ptr_array(pre), _ptr_array(act),
                                                   _lib.ptr(ln), _lib.ptr(ws), wsb, _lib.current_stream(dev)), "vllm_bridge_forward_train")
        ctx.meta = (kind, depth, eps)
        ctx.save_for_backward(x, ln, *pre, *act, *params)
        return out

    @staticmethod
    def backward(ctx, gout):
        kind, depth, eps = ctx.meta
        saved = ctx.saved_tensors
        x, ln = saved[0], saved[1]
        pre, act = list(saved[2:1 + depth]), list(saved[1 + depth:2 * depth])
        params = list(saved[2 * depth:])
        keep = []
        d = _BridgeTrain._desc(kind, depth, eps, params, keep)
        rows, dev = x.shape[0], x.device
        need_x = ctx.needs_input_grad[3]
        ivl = d.kind == _lib.BRIDGE_INTERNVL_MLP
        need_ln = ivl and any(ctx.needs_input_grad[4 + 2 * depth:])
        g = _lib.aligned(gout.to(torch.bfloat16))
        gw = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) for p in params[0:2 * depth:2]]
        gb = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) if p is not None else None for p in params[1:2 * depth:2]]
        gln = [torch.empty(p.shape, dtype=torch.bfloat16, device=dev) for p in params[2 * depth:]] if need_ln else [None, None]
        gx = torch.empty((rows, d.in_features), dtype=torch.bfloat16, device=dev) if need_x else None
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws, wsb = _lib.sized_workspace(dev, L.vllm_bridge_backward_workspace_bytes(ctypes.byref(d), rows, int(need_x)),
                                           "vllm_bridge_backward_workspace_bytes")
            _lib.check(L.vllm_bridge_backward(ctypes.byref(d), _lib.ptr(x), rows, _lib.ptr(g), _ptr_array(pre), _ptr_array(act), _lib.ptr(ln),
                                              _lib.ptr(gx), _ptr_array(gw), _ptr_array(gb), _lib.ptr(gln[0]), _lib.ptr(gln[1]),
                                              _lib.ptr(ws), wsb, _lib.current_stream(dev)), "vllm_bridge_backward")
        grads = [t for i in range(depth) for t in (gw[i], gb[i])] + (gln if ivl else [])
        return (None, None, None, gx) + tuple(grads)


class NativeBridgeLinear(_BridgeMixin, nn.Linear):
    pass


class NativeBridgeSequential(_BridgeMixin, nn.Sequential):
    pass


def build_vl_bridge(vl_bridge_type, v_hidden_size, l_hidden_size, use_pixelshuffle=False):
    """Same construction logic as modeling_visionllmv2.py:160-184."""
    v = v_hidden_size * 4 if use_pixelshuffle else v_hidden_size
    if vl_bridge_type == "linear":
        m = NativeBridgeLinear(v, l_hidden_size)
    elif vl_bridge_type in ("internvl_mlp", "internvl"):
        m = NativeBridgeSequential(nn.LayerNorm(v), nn.Linear(v, l_hidden_size), nn.GELU(),
                                   nn.Linear(l_hidden_size, l_hidden_size))
    else:
        mm = re.match(r"^mlp(\d+)x_gelu*", vl_bridge_type)
        if not mm:
            raise NotImplementedError(f"{vl_bridge_type} not supported yet.")
        depth = int(mm.group(1))
        if depth > 4:
            raise NotImplementedError("mlp depth > 4")
        mods = [nn.Linear(v, l_hidden_size)]
        for _ in range(1, depth):
            mods += [nn.GELU(), nn.Linear(l_hidden_size, l_hidden_size)]
        m = NativeBridgeSequential(*mods)
    m.vl_bridge_type = vl_bridge_type
    return m


def select_and_project(hidden_states, vl_bridge, vis_output_layer=-2, use_pixelshuffle=False):
    """modeling_visionllmv2.py:569-579 in one call: hs[layer][:,1:] (-> pixel_shuffle) -> vl_bridge."""
    return vl_bridge.project_hidden_state(hidden_states[vis_output_layer], use_pixelshuffle)
