"""Bring-up hook B4: drop-in for the reference's ``FlashAttention`` module
(VisionLLMv2/visionllmv2/model/internvit/flash_attention.py:14-76), backed by ``vllm_attn_fwd_qkvpacked_bf16`` / ``_f16``.

Only the call pattern the vision tower uses is supported -- ``forward(qkv[B,S,3,H,D], key_padding_mask=None,
causal=False)`` (``modeling_intern_vit.py:155-157``); anything else raises instead of silently computing something different.

Training (the reference's ``flash_attn_varlen_qkvpacked_func`` is an autograd function; ``freeze_vis_encoder=False`` trains the
tower, train/train.py:163, 534): when grad mode is on and ``qkv`` requires grad, the forward is ``vllm_attn_fwd_train_qkvpacked_*``
(the same kernel and the same ``out`` bits, plus the row log-sum-exp) and the node's backward is ``vllm_attn_bwd_qkvpacked_*``:
dense, non-causal, dropout 0, bf16 / fp16, D in {64, 128}.  Otherwise the call is the inference one: no node, no LSE buffer.
Still raising: ``causal``, ``key_padding_mask``, ``cu_seqlens`` (NotImplementedError) and training with ``attention_dropout > 0``."""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib


def _entry(name, dtype):
    return getattr(_lib.lib(), name + ("_f16" if dtype == torch.float16 else "_bf16"))


class _FlashAttnQKVPacked(torch.autograd.Function):
    """out = softmax(scale q k^T) v on packed qkv [B, S, 3, H, D] (16-byte aligned, contiguous); saves qkv, out and the LSE."""

    @staticmethod
    def forward(ctx, qkv, scale):
        B, S, _, H, D = qkv.shape
        out = torch.empty((B, S, H, D), dtype=qkv.dtype, device=qkv.device)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(_entry("vllm_attn_fwd_train_qkvpacked", qkv.dtype)(
                _lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), B, S, H, D, float(scale), _lib.current_stream(qkv.device)),
                "vllm_attn_fwd_train_qkvpacked")
        ctx.save_for_backward(qkv, out, lse)
        ctx.scale = float(scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        qkv, out, lse = ctx.saved_tensors
        B, S, _, H, D = qkv.shape
        grad_out = _lib.aligned(grad_out.to(qkv.dtype))   # (arrives as a view from the caller's rearrange)
        grad_qkv = torch.empty_like(qkv)                  # written completely by the call
        with torch.cuda.device(qkv.device):
            L = _lib.lib()
            need = L.vllm_attn_bwd_workspace_bytes(B, S, H, D)
            if need < 0:
                raise RuntimeError(f"native FlashAttention backward: head_dim {D} not supported (64 or 128)")
            ws, need = _lib.sized_workspace(qkv.device, need, "vllm_attn_bwd_workspace_bytes")
            _lib.check(_entry("vllm_attn_bwd_qkvpacked", qkv.dtype)(
                _lib.ptr(qkv), _lib.ptr(out), _lib.ptr(lse), _lib.ptr(grad_out), B, S, H, D, ctx.scale, _lib.ptr(grad_qkv),
                _lib.ptr(ws), need, _lib.current_stream(qkv.device)), "vllm_attn_bwd_qkvpacked")
        return grad_qkv, None


class FlashAttention(nn.Module):
    def __init__(self, softmax_scale=None, attention_dropout=0.0, device=None, dtype=None):
        super().__init__()
        self.softmax_scale = softmax_scale
        self.dropout_p = attention_dropout

    def forward(self, qkv, key_padding_mask=None, causal=False, cu_seqlens=None, max_s=None, need_weights=False):
        assert not need_weights
        if key_padding_mask is not None or causal or cu_seqlens is not None:
            raise NotImplementedError("native FlashAttention: only dense non-causal qkv[B,S,3,H,D] (the ViT tile case)")
        if self.training and self.dropout_p > 0:
            raise NotImplementedError("native FlashAttention: attention dropout is not implemented (inference path)")
        # the reference accepts fp16 and bf16 (flash_attention.py:39-41: `assert qkv.dtype in [torch.float16, torch.bfloat16]`)
        if qkv.dtype not in (torch.bfloat16, torch.float16) or not qkv.is_cuda or qkv.dim() != 5 or qkv.shape[2] != 3:
            raise RuntimeError("native FlashAttention: qkv must be a bf16 / fp16 CUDA tensor [B, S, 3, H, D] (flash_attention.py:39-41)")
        qkv = _lib.aligned(qkv)   # (the kernel needs 16-byte aligned q / k / v: a view at another storage offset is copied)
        B, S, _, H, D = qkv.shape
        scale = self.softmax_scale if self.softmax_scale is not None else D ** -0.5
        if torch.is_grad_enabled() and qkv.requires_grad:
            return _FlashAttnQKVPacked.apply(qkv, scale), None
        out = torch.empty((B, S, H, D), dtype=qkv.dtype, device=qkv.device)
        with torch.cuda.device(qkv.device):
            fn = _lib.lib().vllm_attn_fwd_qkvpacked_f16 if qkv.dtype == torch.float16 else _lib.lib().vllm_attn_fwd_qkvpacked_bf16
            _lib.check(fn(_lib.ptr(qkv), _lib.ptr(out), B, S, H, D, float(scale), _lib.current_stream(qkv.device)),
                       "vllm_attn_fwd_qkvpacked")
        return out, None
