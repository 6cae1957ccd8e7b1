"""CLIP ViT (ViT-L/14-336 in the released 7B model) -- drop-in for ``transformers.CLIPVisionModel`` in the
``vis_encoder`` slot (VisionLLMv2/visionllmv2/model/modeling_visionllmv2.py:132-135; train/train.py:382-384).

The arithmetic is third-party (transformers, pinned ==4.34.0 in requirements.txt:22).  Parameter names follow the
HF 4.34 layout the reference's checkpoints use (``vision_model.embeddings.{class_embedding, patch_embedding.weight,
position_embedding.weight}``, ``vision_model.pre_layrnorm.*``, ``vision_model.encoder.layers.{i}.{self_attn.
{q,k,v,out}_proj.*, layer_norm1/2.*, mlp.fc1/fc2.*}``, ``vision_model.post_layernorm.*``); ``load_state_dict`` also
accepts the prefix-less layout newer transformers versions emit.  Inference (the default): ``CLIPVisionModel.forward``
calls ``vllm_vit_forward`` under ``torch.no_grad()`` (q/k/v projections run as ONE fused [3C,C] GEMM).

Training (``freeze_vis_encoder=False``, train/train.py:163, 534): ``_CLIPEncoderLayer.forward`` is ONE autograd node around
``vllm_clip_layer_forward_train`` / ``vllm_clip_layer_backward`` (hand-written HIP underneath; dropout and attention masks are not
implemented), ``_CLIPEncoder.forward(inputs_embeds)`` runs the layers as HF's CLIPEncoder does (each under ``torch.utils.checkpoint`` when
``gradient_checkpointing and self.training``), ``pre_layrnorm`` / ``post_layernorm`` have their own node (``vllm_layernorm_bf16`` /
``vllm_layernorm_backward_res_bf16``) and the embeddings theirs; ``CLIPVisionModel.forward`` with ``native_training = True`` chains them as
HF's CLIPVisionTransformer.forward does, so the tower trains from pixels.
"""
import ctypes

import torch
from torch import nn

from . import _lib
from .vit_common import (EncoderPlan, LayerTrainABI, _require_bf16_cuda, embed_pixels, fold_norm_into_linear, kpad_for, model_output, norm_folding_applies,
                         plan_ptr, padded_patch_weight, run_encoder)

try:
    from transformers import CLIPVisionConfig  # noqa: F401  (the reference passes this very config class)
except Exception:  # pragma: no cover
    CLIPVisionConfig = None


class _CLIPVisionEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.hidden_size
        self.image_size = config.image_size
        self.patch_size = config.patch_size
        self.class_embedding = nn.Parameter(torch.randn(self.embed_dim))
        self.patch_embedding = nn.Conv2d(3, self.embed_dim, kernel_size=self.patch_size, stride=self.patch_size,
                                         bias=False)
        self.num_patches = (self.image_size // self.patch_size) ** 2
        self.num_positions = self.num_patches + 1
        self.position_embedding = nn.Embedding(self.num_positions, self.embed_dim)
        self.register_buffer("position_ids", torch.arange(self.num_positions).expand((1, -1)), persistent=False)

    def forward(self, pixel_values):
        """HF CLIPVisionEmbeddings.forward (conv without bias, class embedding, the whole position table) through the entry the InternViT
        embeddings use: vllm_vit_embed_forward, one autograd node (vllm_vit_embed_backward) when a parameter requires grad."""
        return embed_pixels(pixel_values, self.patch_embedding, self.class_embedding, self.position_embedding.weight)


class _CLIPAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        C = config.hidden_size
        self.k_proj = nn.Linear(C, C)
        self.v_proj = nn.Linear(C, C)
        self.q_proj = nn.Linear(C, C)
        self.out_proj = nn.Linear(C, C)


class _CLIPMLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.fc1 = nn.Linear(config.hidden_size, config.intermediate_size)
        self.fc2 = nn.Linear(config.intermediate_size, config.hidden_size)


class _LayerNormTrain(torch.autograd.Function):
    """nn.LayerNorm as one autograd node: vllm_layernorm_bf16 forward (the no-grad call's bits), vllm_layernorm_backward_res_bf16
    backward.  x [rows, C], weight and bias [C], all 16-byte aligned; saved with save_for_backward (an in-place edit fails the version
    check)."""

    @staticmethod
    def forward(ctx, x, w, b, eps):
        ctx.eps = eps
        ctx.save_for_backward(x, w)
        return _layer_norm_forward(x, w, b, eps)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        rows, C = x.shape
        g = _lib.aligned(gy.to(torch.bfloat16))
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(w) if need_w else None
        gb = torch.empty_like(w) if need_b else None
        L = _lib.lib()
        with torch.cuda.device(x.device):
            ws, wsb = _lib.sized_workspace(x.device, L.vllm_layernorm_backward_res_workspace_bytes(rows, C),
                                           "vllm_layernorm_backward_res_workspace_bytes")
            _lib.check(L.vllm_layernorm_backward_res_bf16(_lib.ptr(x), C, _lib.ptr(g), C, _lib.ptr(w), ctx.eps, rows, C, _lib.ptr(gx), C, None, 0,
                                                          _lib.ptr(gw), _lib.ptr(gb), _lib.ptr(ws), wsb, _lib.current_stream(x.device)),
                       "vllm_layernorm_backward_res_bf16")
        return gx, gw, gb, None


def _layer_norm_forward(x, w, b, eps):
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vllm_layernorm_bf16(_lib.ptr(x), x.shape[1], _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), x.shape[1], x.shape[0],
                                                  x.shape[1], eps, _lib.current_stream(x.device)), "vllm_layernorm_bf16")
    return y


class _CLIPLayerNorm(nn.LayerNorm):
    """pre_layrnorm / post_layernorm: nn.LayerNorm's parameters and names; ``forward`` on a bf16 CUDA tensor [..., C] is
    vllm_layernorm_bf16, as one autograd node when grad is enabled and anything requires grad (the same bits either way)."""

    def forward(self, hidden_states):
        x = hidden_states
        _require_bf16_cuda("hidden_states", x)
        _require_bf16_cuda("weight", self.weight)
        x2 = _lib.aligned(x.reshape(-1, x.shape[-1]))   # (differentiable: a strided or offset view is copied by autograd ops)
        if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or self.bias.requires_grad):
            y = _LayerNormTrain.apply(x2, _lib.aligned(self.weight), _lib.aligned(self.bias), self.eps)
        else:
            y = _layer_norm_forward(x2.detach(), _lib.aligned(self.weight.detach()), _lib.aligned(self.bias.detach()), self.eps)
        return y.view(x.shape)


_LAYER_PARAMS = _lib.pointer_fields(_lib.VllmClipLayerGrads)   # the 12 of VllmClipLayerTrain too, in the same order
_SAVED = _lib.pointer_fields(_lib.VllmClipLayerSaved)
# the module's parameters as the autograd node receives them: q, k, v weights and biases apart (their gradients are slices of qkv's)
_MODULE_PARAMS = ("norm1_w", "norm1_b", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w",
                  "fc1_b", "fc2_w", "fc2_b")


def _fused_params(mp):
    """the 16 module parameters -> the 12 of _LAYER_PARAMS, detached; q / k / v concatenated on the host (a fresh [3C, C] / [3C] each call:
    nothing to go stale between optimizer steps)"""
    n1w, n1b, qw, qb, kw, kb, vw, vb = mp[:8]
    d = lambda t: t.detach()
    return (d(n1w), d(n1b), torch.cat([d(qw), d(kw), d(vw)], 0), torch.cat([d(qb), d(kb), d(vb)], 0)) + tuple(d(t) for t in mp[8:])


_TRAIN = LayerTrainABI("clip", _lib.VllmClipLayerTrain, _lib.VllmClipLayerSaved, _lib.VllmClipLayerGrads, _LAYER_PARAMS, _SAVED)


def _scalars(meta):
    heads, inter, act, eps = meta
    return dict(heads=heads, inter=inter, act=act, eps=eps)


def _layer_desc(meta, params, keep):
    return _TRAIN.desc(_scalars(meta), params, keep)


class _ClipLayerTrain(torch.autograd.Function):
    """One CLIP encoder layer as one autograd node.  Inputs: x [B, S, C] (16-byte aligned) and the module's parameters in _MODULE_PARAMS
    order.  Parameters and the kept activations go through save_for_backward, so an in-place update between forward and backward
    fails autograd's version check instead of producing wrong gradients."""

    @staticmethod
    def forward(ctx, meta, x, *mp):
        out, saved = _TRAIN.forward(_scalars(meta), x, _fused_params(mp))
        ctx.meta = meta
        ctx.save_for_backward(x, *saved, *mp)
        return out

    @staticmethod
    def backward(ctx, gout):
        t = ctx.saved_tensors
        x, saved, mp = t[0], t[1:1 + len(_SAVED)], t[1 + len(_SAVED):]
        C = x.shape[-1]
        nm = dict(zip(_MODULE_PARAMS, ctx.needs_input_grad[2:]))
        need = {n: nm.get(n, False) for n in _LAYER_PARAMS}
        need["qkv_w"] = nm["q_w"] or nm["k_w"] or nm["v_w"]
        need["qkv_b"] = nm["q_b"] or nm["k_b"] or nm["v_b"]
        gx, grads = _TRAIN.backward(_scalars(ctx.meta), x, saved, _fused_params(mp), gout, ctx.needs_input_grad[1],
                                    [need[n] for n in _LAYER_PARAMS])
        grads = dict(zip(_LAYER_PARAMS, grads))
        out = []
        for n in _MODULE_PARAMS:   # (a q / k / v slice nobody asked for is dropped)
            if not nm[n]:
                out.append(None)
            elif n[0] in "qkv" and n[1] == "_":
                i = "qkv".index(n[0])
                out.append(grads["qkv" + n[1:]][i * C:(i + 1) * C])
            else:
                out.append(grads[n])
        return (None, gx) + tuple(out)


class _CLIPEncoderLayer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.hidden_size
        self.self_attn = _CLIPAttention(config)
        self.layer_norm1 = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.mlp = _CLIPMLP(config)
        self.layer_norm2 = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        act = getattr(config, "hidden_act", "quick_gelu")
        self._dropout = float(getattr(config, "attention_dropout", 0.0) or 0.0)
        self._meta = (config.num_attention_heads, config.intermediate_size, _lib.EPI_QUICK_GELU if act == "quick_gelu" else _lib.EPI_GELU,
                      config.layer_norm_eps)

    def _params(self):
        a, m = self.self_attn, self.mlp
        return (self.layer_norm1.weight, self.layer_norm1.bias, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias,
                a.v_proj.weight, a.v_proj.bias, a.out_proj.weight, a.out_proj.bias, self.layer_norm2.weight, self.layer_norm2.bias,
                m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)

    def forward(self, hidden_states, attention_mask=None, causal_attention_mask=None, output_attentions=False):
        """HF 4.34 CLIPEncoderLayer.forward on a bf16 CUDA [B, S, C] tensor -> (out,): vllm_clip_layer_forward_train, as one autograd node
        when grad is enabled and anything in it requires grad (the same output bits either way)."""
        if attention_mask is not None or causal_attention_mask is not None:
            raise NotImplementedError("_CLIPEncoderLayer (native): attention masks are not implemented (the vision tower passes none)")
        if output_attentions:
            raise NotImplementedError("attention maps are never materialised by the fused attention kernel")
        if self.training and self._dropout > 0.0:
            raise NotImplementedError("_CLIPEncoderLayer (native): attention_dropout > 0 is not implemented for training; set it to 0 "
                                      "(the released configs do) or call .eval()")
        x = hidden_states
        _require_bf16_cuda("hidden_states", x)
        if x.dim() != 3 or x.shape[-1] != self.embed_dim:
            raise ValueError(f"hidden_states must be [batch, seq_len, {self.embed_dim}], got {tuple(x.shape)}")
        mp = self._params()
        x = _lib.aligned(x)   # (16-byte aligned rows: a view at another storage offset is copied -- differentiably)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in mp)):
            return (_ClipLayerTrain.apply(self._meta, x, *mp),)
        return (_TRAIN.forward(_scalars(self._meta), x.detach(), _fused_params(mp))[0],)


class _CLIPEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.layers = nn.ModuleList([_CLIPEncoderLayer(config) for _ in range(config.num_hidden_layers)])
        self.gradient_checkpointing = False   # (HF's default)

    def forward(self, inputs_embeds, output_hidden_states=None, return_dict=None):
        """HF 4.34 CLIPEncoder.forward without masks and attention maps: the training entry (gradients flow to ``inputs_embeds`` and
        every layer parameter)."""
        import torch.utils.checkpoint
        cfg = self.config
        output_hidden_states = output_hidden_states if output_hidden_states is not None else getattr(cfg, "output_hidden_states", False)
        return_dict = return_dict if return_dict is not None else getattr(cfg, "use_return_dict", True)
        encoder_states = () if output_hidden_states else None
        hidden_states = inputs_embeds
        for layer in self.layers:
            if output_hidden_states:
                encoder_states = encoder_states + (hidden_states,)
            if self.gradient_checkpointing and self.training:
                # (non-reentrant: the layer's parameters get their gradients even when inputs_embeds itself does not require grad)
                hidden_states = torch.utils.checkpoint.checkpoint(layer, hidden_states, use_reentrant=False)[0]
            else:
                hidden_states = layer(hidden_states)[0]
        if output_hidden_states:
            encoder_states = encoder_states + (hidden_states,)
        if not return_dict:
            return tuple(v for v in [hidden_states, encoder_states] if v is not None)
        try:
            from transformers.modeling_outputs import BaseModelOutput
            return BaseModelOutput(last_hidden_state=hidden_states, hidden_states=encoder_states)
        except Exception:  # transformers not importable: a minimal stand-in with the attributes the caller reads
            from types import SimpleNamespace
            return SimpleNamespace(last_hidden_state=hidden_states, hidden_states=encoder_states)


class _CLIPVisionTransformer(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.embeddings = _CLIPVisionEmbeddings(config)
        self.pre_layrnorm = _CLIPLayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.encoder = _CLIPEncoder(config)
        self.post_layernorm = _CLIPLayerNorm(config.hidden_size, eps=config.layer_norm_eps)


class CLIPVisionModel(nn.Module):
    main_input_name = "pixel_values"

    def __init__(self, config):
        super().__init__()
        act = getattr(config, "hidden_act", "quick_gelu")
        if act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"hidden_act {act!r}")
        self.config = config
        self.vision_model = _CLIPVisionTransformer(config)
        self._plan = EncoderPlan()
        self.keep_hidden_states = None
        #: False = ``forward(pixel_values)`` is the fused inference encoder under no_grad, whatever the grad mode (the default);
        #: True = with grad enabled and a parameter that requires grad, ``forward`` is differentiable: embeddings -> pre_layrnorm ->
        #: layer modules -> post_layernorm
        self.native_training = False

    def get_input_embeddings(self):
        return self.vision_model.embeddings.patch_embedding

    def load_state_dict(self, state_dict, strict=True, **kw):
        if not any(k.startswith("vision_model.") for k in state_dict):
            state_dict = {"vision_model." + k: v for k, v in state_dict.items()}
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _build_plan(self):
        cfg = self.config
        params = list(self.parameters())
        key = EncoderPlan.signature(params)
        plan = self._plan
        if plan.key == key:
            return plan.desc
        for n_, p in self.named_parameters():
            _require_bf16_cuda(n_, p)
        vm = self.vision_model
        emb = vm.embeddings
        kpad = kpad_for(cfg.patch_size)
        pw = padded_patch_weight(emb.patch_embedding.weight, kpad)
        plan.keep = [pw]
        L = len(vm.encoder.layers)
        layers = (_lib.VllmVitLayer * L)()
        P = plan_ptr(plan)
        for i, lyr in enumerate(vm.encoder.layers):
            a = lyr.self_attn
            qkv_w = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0).detach().contiguous()
            qkv_b = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], 0).detach().contiguous()
            plan.keep += [qkv_w, qkv_b]
            fold = {}
            if norm_folding_applies(cfg.hidden_size, cfg.intermediate_size):
                q_ln, q_cs, q_b = fold_norm_into_linear(qkv_w, qkv_b, lyr.layer_norm1.weight, lyr.layer_norm1.bias, True)
                f_ln, f_cs, f_b = fold_norm_into_linear(lyr.mlp.fc1.weight, lyr.mlp.fc1.bias, lyr.layer_norm2.weight,
                                                        lyr.layer_norm2.bias, True)
                plan.keep += [q_ln, q_cs, q_b, f_ln, f_cs, f_b]
                fold = dict(qkv_w_ln=P(q_ln), qkv_colsum=P(q_cs), qkv_bias_ln=P(q_b), fc1_w_ln=P(f_ln), fc1_colsum=P(f_cs),
                            fc1_bias_ln=P(f_b))
            layers[i] = _lib.VllmVitLayer(
                norm1_w=P(lyr.layer_norm1.weight), norm1_b=P(lyr.layer_norm1.bias), qkv_w=P(qkv_w), qkv_b=P(qkv_b),
                q_norm_w=None, k_norm_w=None, proj_w=P(a.out_proj.weight), proj_b=P(a.out_proj.bias), ls1=None,
                norm2_w=P(lyr.layer_norm2.weight), norm2_b=P(lyr.layer_norm2.bias), fc1_w=P(lyr.mlp.fc1.weight),
                fc1_b=P(lyr.mlp.fc1.bias), fc2_w=P(lyr.mlp.fc2.weight), fc2_b=P(lyr.mlp.fc2.bias), ls2=None, **fold)
        act = _lib.EPI_QUICK_GELU if getattr(cfg, "hidden_act", "quick_gelu") == "quick_gelu" else _lib.EPI_GELU
        desc = _lib.VllmVitDesc(
            arch=_lib.ARCH_CLIP, num_layers=L, hidden=cfg.hidden_size, heads=cfg.num_attention_heads,
            inter=cfg.intermediate_size, patch=cfg.patch_size, image=cfg.image_size, kpad=kpad, act=act, pixel_is_f32=0,
            eps=cfg.layer_norm_eps, patch_w=P(pw), patch_b=None, cls=P(emb.class_embedding),
            pos=P(emb.position_embedding.weight), pre_ln_w=P(vm.pre_layrnorm.weight), pre_ln_b=P(vm.pre_layrnorm.bias),
            layers=ctypes.cast(layers, ctypes.POINTER(_lib.VllmVitLayer)))
        plan.key, plan.desc, plan.layers = key, desc, layers
        return desc

    def forward(self, pixel_values=None, output_attentions=None, output_hidden_states=None, return_dict=None, **kw):
        """HF CLIPVisionModel.forward.  The fused inference encoder under ``torch.no_grad()`` unless ``native_training`` is set, grad is
        enabled and a parameter requires grad: then the embeddings, ``pre_layrnorm``, the encoder's layer modules and ``post_layernorm``
        run as autograd nodes (HF's own route), every hidden state is an autograd tensor and ``keep_hidden_states`` does not apply."""
        cfg = self.config
        if output_attentions:
            raise NotImplementedError("attention maps are never materialised by the fused attention kernel")
        output_hidden_states = (output_hidden_states if output_hidden_states is not None
                                else getattr(cfg, "output_hidden_states", False))
        return_dict = return_dict if return_dict is not None else getattr(cfg, "use_return_dict", True)
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        if self.native_training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            vm = self.vision_model
            hidden_states = vm.pre_layrnorm(vm.embeddings(pixel_values))
            enc = vm.encoder(inputs_embeds=hidden_states, output_hidden_states=output_hidden_states, return_dict=True)
            last = enc.last_hidden_state
            return model_output(last, vm.post_layernorm(last[:, 0, :]), enc.hidden_states, return_dict)
        with torch.no_grad():
            return self._forward_fused(pixel_values, output_hidden_states, return_dict)

    def _forward_fused(self, pixel_values, output_hidden_states, return_dict):
        cfg = self.config
        desc = self._build_plan()
        keep = self.keep_hidden_states if output_hidden_states else (-1,)
        states = run_encoder(desc, pixel_values, desc.num_layers, cfg.hidden_size, keep)
        last = states[-1]
        # pooler_output = post_layernorm(last[:, 0])  (HF CLIPVisionTransformer); unused by VisionLLMv2 but kept
        n, S, C = last.shape
        pooled = torch.empty((n, C), dtype=last.dtype, device=last.device)
        pl = self.vision_model.post_layernorm
        plw, plb = _lib.aligned(pl.weight.detach()), _lib.aligned(pl.bias.detach())   # (16-byte aligned: views are copied)
        with torch.cuda.device(last.device):
            _lib.check(_lib.lib().vllm_layernorm_bf16(_lib.ptr(last), S * C, _lib.ptr(plw), _lib.ptr(plb),
                                                      _lib.ptr(pooled), C, n, C, pl.eps,
                                                      _lib.current_stream(last.device)), "vllm_layernorm_bf16")
        hs = tuple(states) if output_hidden_states else None
        return model_output(last, pooled, hs, return_dict)
