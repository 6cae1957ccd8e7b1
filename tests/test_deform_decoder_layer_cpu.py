"""CPU: the boundary of the native deformable decoder layer (include/vllm_hip.h, section f2c) -- symbols, descriptor layout, the size
query, the argument gates of the layer entry and of the attention kernel (refused calls only, fake pointers: nothing is dereferenced,
no device is touched), and the module mirrors where no GPU is needed: parameter names, every reason ``native_layer_applies`` has to say
no, the masked cases' own conditions, and the composed forward of both flavours against a restatement written here."""
import ctypes
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import deformable_decoder as D

import deform_decoder_layer_inputs as I

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
NEW = ("vllm_deform_dec_layer_desc_sizeof", "vllm_deform_dec_layer_workspace_bytes", "vllm_deform_dec_layer_calls",
       "vllm_deform_dec_layer_forward", "vllm_mha_fwd_bf16")
ATTN_POINTERS = ("value_proj_w", "value_proj_b", "sampling_offsets_w", "sampling_offsets_b", "attention_weights_w", "attention_weights_b",
                 "output_proj_w", "output_proj_b")
SA_POINTERS = ("sa_in_proj_w", "sa_in_proj_b", "sa_out_proj_w", "sa_out_proj_b", "sa_norm_w", "sa_norm_b")
TEXT_POINTERS = ("text_in_proj_w", "text_in_proj_b", "text_out_proj_w", "text_out_proj_b", "text_norm_w", "text_norm_b")
POINTERS = ("ca_norm_w", "ca_norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ffn_norm_w", "ffn_norm_b")
MHA_NAMES = ["in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias"]
MSDA_NAMES = ["sampling_offsets.weight", "sampling_offsets.bias", "attention_weights.weight", "attention_weights.bias", "value_proj.weight",
              "value_proj.bias", "output_proj.weight", "output_proj.bias"]
WB = ["weight", "bias"]


def names(prefix, leaves):
    return [f"{prefix}.{n}" for n in leaves]


# the reference's parameter lists, in registration order (modeling_unipose.py:3196-3230; ...mask_dn.py:1293-1327)
UNIPOSE_NAMES = names("cross_attn", MSDA_NAMES) + names("norm1", WB) + names("ca_text", MHA_NAMES) + names("catext_norm", WB) + \
    names("self_attn", MHA_NAMES) + names("norm2", WB) + names("linear1", WB) + names("linear2", WB) + names("norm3", WB)
GDINO_NAMES = names("self_attn", MHA_NAMES) + names("self_attn_layer_norm", WB) + names("encoder_attn_text", MHA_NAMES) + \
    names("encoder_attn_text_layer_norm", WB) + names("encoder_attn", MSDA_NAMES) + names("encoder_attn_layer_norm", WB) + \
    names("fc1", WB) + names("fc2", WB) + names("final_layer_norm", WB)


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def desc(C=256, M=8, Lv=4, P=4, F=2048, act=0, ref_dim=4, heads=8, sa=1, text=1, **ptrs):
    d = _lib.VllmDeformDecLayerDesc()
    a = d.cross_attn
    a.d_model, a.n_heads, a.n_levels, a.n_points, a.ref_dim = C, M, Lv, P, ref_dim
    d.d_ffn, d.act, d.n_heads_sa, d.has_self_attn, d.has_text_attn = F, act, heads, sa, text
    d.sa_norm_eps = d.text_norm_eps = d.ca_norm_eps = d.ffn_norm_eps = 1e-5
    for n in ATTN_POINTERS:
        setattr(a, n, ptrs.get(n, PTR))
    for n in SA_POINTERS + TEXT_POINTERS + POINTERS:
        setattr(d, n, ptrs.get(n, PTR))
    return d


def last_error():
    return _lib.lib().vllm_last_error().decode()


def forward(d, B=2, Lq=130, Lt=9, S=161, tgt=PTR, pos=PTR, ref=PTR, text=PTR, memory=PTR + (1 << 30), shapes=PTR, lsi=PTR,
            out=PTR + (1 << 31), ws=PTR + (1 << 32), ws_bytes=1 << 40):
    return _lib.lib().vllm_deform_dec_layer_forward(ctypes.byref(d), vp(tgt), vp(pos), vp(ref), None, vp(text), None, vp(memory), None,
                                                    vp(shapes), vp(lsi), B, Lq, Lt, S, vp(out), vp(ws), ws_bytes, None)


def dec_calls():
    return _lib.lib().vllm_deform_dec_layer_calls()


def test_symbols_are_declared_and_exported_and_the_abi_version_stays_2():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T vllm_" in line}
    for n in NEW:
        assert n in protos, n
        assert n in exported, n
    assert _lib.header_abi_version() == 2 and _lib.lib().vllm_abi_version() == 2
    hdr = open(_lib.HEADER).read()
    assert "f2c. The whole deformable DECODER layer" in hdr
    for n in ("vllm_deform_dec_layer_forward", "vllm_mha_fwd_bf16"):
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + n + r"\s*\(", hdr, flags=re.S), f"no 'Alignment' line directly above {n}"


def test_descriptor_mirror_has_the_library_size_and_the_header_order():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.VllmDeformDecLayerDesc) == L.vllm_deform_dec_layer_desc_sizeof()
    _lib.check_struct_layouts()
    hdr = open(_lib.HEADER).read()
    body = hdr[hdr.index("typedef struct VllmDeformDecLayerDesc {"):hdr.index("} VllmDeformDecLayerDesc;")]
    order = [re.search(r"\b" + n + r"\b", body).start() for n, _ in _lib.VllmDeformDecLayerDesc._fields_]
    assert order == sorted(order), "field order differs from include/vllm_hip.h"
    assert _lib.VllmDeformDecLayerDesc._fields_[0] == ("cross_attn", _lib.VllmMsdaLayerDesc)
    assert dec_calls() >= 0


def test_workspace_query_is_positive_and_monotone():
    L = _lib.lib()
    d = desc()
    q = lambda b, lq, lt, s, dd=d: L.vllm_deform_dec_layer_workspace_bytes(ctypes.byref(dd), b, lq, lt, s)
    a256 = lambda x: (x + 255) & ~255
    base = q(2, 130, 9, 161)
    attn = L.vllm_msda_layer_workspace_bytes(ctypes.byref(d.cross_attn), 2, 130, 161)
    R, C = 260, 256
    # x + pos, the running x twice, [q | k], v, the attention output, the text's [k | v], the FFN intermediate, the attention layer's own
    assert attn > 0 and base == 5 * a256(R * C * 2) + a256(R * 2 * C * 2) + a256(18 * 2 * C * 2) + a256(R * 2048 * 2) + attn
    assert q(3, 130, 9, 161) > base and q(2, 131, 9, 161) > base and q(2, 130, 10, 161) > base and q(2, 130, 9, 162) > base
    assert q(2, 130, 9, 161) == base
    no_text, neither = desc(text=0), desc(text=0, sa=0)
    assert q(2, 130, 9, 161, no_text) == q(2, 130, 50, 161, no_text) == base - a256(18 * 2 * C * 2)
    assert q(2, 130, 9, 161, neither) == 3 * a256(R * C * 2) + a256(R * 2048 * 2) + attn
    assert q(0, 130, 9, 161) == 0 and q(2, 0, 9, 161) == 0
    assert q(-1, 130, 9, 161) < 0 and q(2, 130, -1, 161) < 0 and q(1 << 16, 1 << 15, 9, 161) < 0 and "2^31" in last_error()
    assert L.vllm_deform_dec_layer_workspace_bytes(None, 2, 130, 9, 161) < 0


@pytest.mark.parametrize("kw,word", [
    (dict(act=7), "unknown act"),
    (dict(act=2), "unknown act"),                 # quick-GELU is a GEMM epilogue, not an activation of these layers
    (dict(F=2000), "d_ffn"),
    (dict(F=0), "d_ffn"),
    (dict(C=576, M=9, heads=9), "multiple of 64 in 64 .. 512"),
    (dict(C=80, M=8), "multiple of 64"),
    (dict(heads=16), "head dim 32 or 64"),        # 256 / 16 = 16
    (dict(heads=2), "head dim 32 or 64"),         # 128
    (dict(heads=0), "head dim 32 or 64"),
    (dict(heads=7), "head dim 32 or 64"),
    (dict(ref_dim=3), "reference_points must be 2 or 4"),          # the attention layer's own gate
], ids=["act7", "act_quick_gelu", "d_ffn2000", "d_ffn0", "d_model576", "d_model80", "head_dim16", "head_dim128", "heads0", "heads7", "ref_dim3"])
def test_refused_descriptors_have_their_own_messages(kw, word):
    L = _lib.lib()
    d = desc(**kw)
    before = dec_calls()
    assert L.vllm_deform_dec_layer_workspace_bytes(ctypes.byref(d), 2, 130, 9, 161) < 0
    assert word in last_error(), last_error()
    assert forward(d) == EINVAL
    assert word in last_error() and "workspace" not in last_error(), last_error()
    assert dec_calls() == before


def test_the_head_count_is_not_looked_at_without_an_attention_block():
    d = desc(heads=0, sa=0, text=0)
    assert _lib.lib().vllm_deform_dec_layer_workspace_bytes(ctypes.byref(d), 2, 130, 9, 161) > 0


def test_null_misaligned_and_overlapping_operands_have_their_own_messages():
    d = desc()
    before = dec_calls()
    for kw in (dict(tgt=0), dict(ref=0), dict(text=0), dict(memory=0), dict(shapes=0), dict(lsi=0), dict(out=0)):
        assert forward(d, **kw) == EINVAL, kw
        assert "null pointer" in last_error() and "workspace" not in last_error(), (kw, last_error())
    assert forward(desc(text=0), text=0, ws_bytes=0) == EINVAL and "workspace" in last_error()          # memory_text is not read without the block
    for kw in (dict(tgt=PTR + 8), dict(pos=PTR + 8), dict(text=PTR + 8), dict(memory=PTR + 8), dict(out=PTR + (1 << 31) + 8), dict(ref=PTR + 8),
               dict(ref=PTR + 4)):
        assert forward(d, **kw) == EINVAL, kw
        assert "misaligned tgt" in last_error() and "workspace" not in last_error(), (kw, last_error())
    assert forward(desc(ref_dim=2), ref=PTR + 8, ws_bytes=0) == EINVAL and "workspace" in last_error()   # 2-d reference points: 8 bytes do
    for name in ATTN_POINTERS + SA_POINTERS + TEXT_POINTERS + POINTERS:
        assert forward(desc(**{name: PTR + 8})) == EINVAL, name
        assert "misaligned weight or bias" in last_error(), (name, last_error())
        assert forward(desc(**{name: 0})) == EINVAL, name
        assert "missing weights" in last_error() or "null" in last_error(), (name, last_error())
    # a block that is off does not need its weights
    assert forward(desc(sa=0, **{n: 0 for n in SA_POINTERS}), ws_bytes=0) == EINVAL and "workspace" in last_error()
    assert forward(desc(text=0, **{n: 0 for n in TEXT_POINTERS}), ws_bytes=0) == EINVAL and "workspace" in last_error()
    nbytes = 2 * 130 * 256 * 2
    for kw in (dict(out=PTR), dict(out=PTR + nbytes - 16), dict(out=PTR - nbytes + 16), dict(out=PTR + (1 << 30) + 4096), dict(tgt=PTR + (1 << 31)),
               dict(text=PTR + (1 << 31) - 16)):
        assert forward(d, **kw) == EINVAL, kw
        assert "overlaps" in last_error() and "workspace" not in last_error(), (kw, last_error())
    assert forward(d, B=1 << 16, Lq=1 << 15) == EINVAL and "2^31" in last_error()
    assert forward(d, B=-1) == EINVAL and "2^31" in last_error()
    assert forward(d, B=1 << 10, Lt=1 << 12) == EINVAL and "text's [k | v] reach 2^31" in last_error()          # 2^22 rows x 1024 bytes
    assert _lib.lib().vllm_deform_dec_layer_workspace_bytes(ctypes.byref(d), 1 << 10, 130, 1 << 12, 161) < 0
    assert _lib.lib().vllm_deform_dec_layer_workspace_bytes(ctypes.byref(desc(text=0)), 1 << 10, 130, 1 << 12, 161) > 0
    assert forward(d, S=0) == EINVAL and "empty" in last_error()
    assert forward(d, Lt=0) == EINVAL and "empty" in last_error()
    # B Lq == 0: nothing to do, whatever the pointers are
    assert forward(d, B=0, tgt=0, out=0, ws=0, ws_bytes=0) == 0 and forward(d, Lq=0, tgt=0, out=0, ws=0, ws_bytes=0) == 0
    assert dec_calls() == before          # no refused call reached a launch


def test_short_misaligned_and_null_workspaces_are_refused():
    L = _lib.lib()
    for d in (desc(), desc(sa=0), desc(text=0, ref_dim=2)):
        need = L.vllm_deform_dec_layer_workspace_bytes(ctypes.byref(d), 2, 130, 9, 161)
        assert need > 0
        before = dec_calls()
        base = PTR + (1 << 32)
        for w, n in ((base, need - 1), (base + 8, need), (base + 8, need + 4096), (0, need)):
            assert forward(d, ws=w, ws_bytes=n) == EINVAL
            assert "workspace" in last_error(), last_error()
        assert dec_calls() == before


def test_the_attention_kernel_refuses_what_it_cannot_run():
    """every refusal of vllm_mha_fwd_bf16 is decided on the host: fake pointers, no device"""
    L = _lib.lib()

    def mha(q=PTR, k=PTR, v=PTR, out=PTR, bs=130 * 512, ld=512, B=2, Lq=130, Lk=130, H=8, Dh=32, **kw):
        a = dict(q_bs=bs, ldq=ld, k_bs=bs, ldk=ld, v_bs=bs, ldv=ld, o_bs=bs, ldo=ld)
        a.update(kw)
        return L.vllm_mha_fwd_bf16(vp(q), a["q_bs"], a["ldq"], vp(k), a["k_bs"], a["ldk"], vp(v), a["v_bs"], a["ldv"], vp(out), a["o_bs"],
                                   a["ldo"], None, None, B, Lq, Lk, H, Dh, 0.17, None)
    for Dh in (16, 48, 128, 0):
        assert mha(Dh=Dh) == EINVAL and "head dim" in last_error(), Dh
    for kw in (dict(q=0), dict(k=0), dict(v=0), dict(out=0)):
        assert mha(**kw) == EINVAL and "null pointer" in last_error(), kw
    for kw in (dict(q=PTR + 8), dict(k=PTR + 8), dict(v=PTR + 8), dict(out=PTR + 8), dict(ldq=516), dict(ldk=260), dict(ldv=248), dict(ldo=255),
               dict(q_bs=130 * 512 + 4), dict(o_bs=130 * 512 + 1)):
        assert mha(**kw) == EINVAL and "misaligned operand" in last_error(), (kw, last_error())
    assert mha(Lk=0) == EINVAL and "at least one key" in last_error()
    assert mha(H=0) == EINVAL and mha(B=-1) == EINVAL and mha(Lq=-1) == EINVAL
    assert mha(B=0, q=0, out=0) == 0 and mha(Lq=0, q=0, k=0, v=0, out=0) == 0          # B Lq == 0: nothing to do


def test_constructors_take_the_reference_arguments_and_names():
    m = I.make_layer("unipose", "small")
    assert [n for n, _ in m.named_parameters()] == UNIPOSE_NAMES
    assert isinstance(m.cross_attn, D.MSDeformAttn) and isinstance(m.self_attn, nn.MultiheadAttention) and not m.self_attn.batch_first
    assert isinstance(m.ca_text, nn.MultiheadAttention) and m.activation is F.relu and m.norm_ext is None and m.key_aware_proj is None
    plain = D.DeformableTransformerDecoderLayer(d_model=64, d_ffn=128, n_levels=2, n_heads=2, dropout=0.0)
    assert [n for n, _ in plain.named_parameters()] == [n for n in UNIPOSE_NAMES if not n.startswith("ca")]
    assert isinstance(plain.dropout1, nn.Identity) and not hasattr(plain, "ca_text")
    m.rm_self_attn_modules()
    assert m.self_attn is None and m.dropout2 is None and m.norm2 is None
    assert [n for n, _ in m.named_parameters()] == [n for n in UNIPOSE_NAMES if not n.startswith(("self_attn", "norm2"))]
    g = I.make_layer("gdino", "wide")
    assert [n for n, _ in g.named_parameters()] == GDINO_NAMES
    assert isinstance(g.encoder_attn, D.GroundingDinoMultiscaleDeformableAttention) and g.self_attn.batch_first and g.activation_fn is F.gelu
    assert D.DeformableTransformerDecoderLayer.native_layer is False and D.GroundingDinoDecoderLayer.native_layer is False
    assert not any("native" in k for k in list(I.make_layer("unipose", "small").state_dict()) + list(g.state_dict()))
    with pytest.raises(NotImplementedError, match="ffn_extra_layernorm"):
        D.DeformableTransformerDecoderLayer(ffn_extra_layernorm=True)
    with pytest.raises(AssertionError):
        D.DeformableTransformerDecoderLayer(use_text_feat_guide=True)
    import visionllm_amd
    assert visionllm_amd.DeformableTransformerDecoderLayer is D.DeformableTransformerDecoderLayer
    assert visionllm_amd.GroundingDinoDecoderLayer is D.GroundingDinoDecoderLayer


@pytest.mark.parametrize("flavour", I.FLAVOURS)
def test_every_reason_to_keep_the_composed_path(flavour):
    """CPU tensors: the device reasons are always there; every other condition adds its own reason when, and only when, it is broken."""
    m = I.as_bf16(I.make_layer(flavour, "small"), "cpu")
    for p in m.parameters():
        p.requires_grad_(False)
    t = I.to(I.make_inputs("small"), "cpu")
    Lq, B = t["tgt"].shape[1], t["tgt"].shape[0]
    base = I.applies(flavour, m, t)
    device_only = ["tgt / memory: bf16 CUDA tensors [., ., C]", "query_pos: a bf16 CUDA tensor of tgt's shape", "parameters: bf16 on the GPU",
                   "cross-attention: msda_layer_fused_ok", "memory_text: a bf16 CUDA tensor [B, Lt, C]"]
    assert base == device_only

    def extra(mod=m, tt=t, **kw):
        return [r for r in I.applies(flavour, mod, tt, **kw) if r not in device_only]

    assert extra() == []
    for p in m.parameters():
        p.requires_grad_(True)
    with torch.enable_grad():
        assert extra() == ["requires_grad under grad mode: there is no native backward"]
    with torch.no_grad():
        assert extra() == []
    for p in m.parameters():
        p.requires_grad_(False)
    with torch.enable_grad():
        assert extra(tt=dict(t, tgt=t["tgt"].clone().requires_grad_(True))) == ["requires_grad under grad mode: there is no native backward"]
    m.train()
    assert extra() == ["active dropout"]
    m.eval()
    nodrop = I.as_bf16(I.make_layer(flavour, "small", dropout=0.0), "cpu").train()
    assert "active dropout" not in I.applies(flavour, nodrop, t)
    mha_only = copy_with(flavour, dropout=0.0)
    mha_only.self_attn.dropout = 0.1          # the attention module's own dropout, in training mode
    assert "active dropout" in I.applies(flavour, mha_only.train(), t) and "active dropout" not in I.applies(flavour, mha_only.eval(), t)
    other_act = I.as_bf16(I.make_layer(flavour, "small", activation="prelu" if flavour == "unipose" else "silu"), "cpu")
    assert "activation: relu or gelu" in extra(other_act)
    assert extra(tt=dict(t, reference_points=t["reference_points"][..., :1])) == ["reference_points: last dim 2 or 4"]
    assert extra(tt=dict(t, reference_points=None)) == ["reference_points: last dim 2 or 4"]
    fmask = torch.zeros(Lq, Lq).masked_fill(t["self_attn_mask"], float("-inf"))
    for bad in (fmask, t["self_attn_mask"][None].expand(B * 2, Lq, Lq), t["self_attn_mask"][:, :-1], t["self_attn_mask"].to(torch.uint8)):
        got = extra(tt=dict(t, self_attn_mask=bad))
        assert len(got) == 1 and got[0].startswith("self_attn_mask"), got
    assert extra(tt=dict(t, self_attn_mask=None)) == []
    for bad in (t["text_mask"].float(), t["text_mask"][:, :-1], t["text_mask"][0]):
        assert extra(tt=dict(t, text_mask=bad)) == ["text mask: None or bool [B, Lt]"]
    assert extra(tt=dict(t, text_mask=None)) == []
    d16 = copy_with(flavour, heads=4)
    assert extra(d16) == ["self_attn: head dim 16 (32 or 64)", "text attention: head dim 16 (32 or 64)"]
    broken = copy_with(flavour)
    broken.self_attn.add_zero_attn = True
    assert extra(broken) == ["self_attn: bias_k / add_zero_attn"]
    broken = copy_with(flavour)
    broken.self_attn.in_proj_bias = None
    assert extra(broken) == ["self_attn: no bias"]
    broken = copy_with(flavour)
    broken.self_attn._qkv_same_embed_dim = False
    assert extra(broken) == ["self_attn: separate q / k / v projection weights"]
    broken = copy_with(flavour)
    (broken.linear1 if flavour == "unipose" else broken.fc1).bias = None
    assert extra(broken) == ["parameters: a Linear / LayerNorm without bias"]
    f32 = I.make_layer(flavour, "small")
    for p in f32.parameters():
        p.requires_grad_(False)
    assert "parameters: bf16 on the GPU" in I.applies(flavour, f32, I.to(t, "cpu", torch.float32))
    if flavour == "gdino":
        assert extra(output_attentions=True) == ["output_attentions: the attention weights stay inside the native call"]
    else:
        assert extra(cross_attn_mask=torch.zeros(1)) == ["cross_attn_mask"]
    # meta tensors: decided without touching data
    meta = I.to(t, "meta")
    assert I.applies(flavour, m, meta)[0] == device_only[0]
    # and the switch changes nothing where the native call does not apply
    assert not (m.native_layer_applies(t["tgt"]) if flavour == "gdino" else m.native_layer_applies(t["tgt"].transpose(0, 1)))


def copy_with(flavour, **kw):
    m = I.as_bf16(I.make_layer(flavour, "small", **kw), "cpu")
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def test_d_model_and_d_ffn_conditions():
    t = I.to(I.make_inputs("small"), "cpu")
    m = D.DeformableTransformerDecoderLayer(d_model=64, d_ffn=100, n_levels=2, n_heads=2, use_text_cross_attention=True)
    assert "d_model a multiple of 64 up to 512, d_ffn a multiple of 64" in I.applies("unipose", m, t)
    assert "d_model a multiple of 64 up to 512, d_ffn a multiple of 64" not in I.applies("unipose", I.make_layer("unipose", "small"), t)


def mha_restated(mha, q, k, v, attn_mask=None, key_padding_mask=None):
    """nn.MultiheadAttention's arithmetic, batch-first tensors -> [B, Lq, C]"""
    C, H = mha.embed_dim, mha.num_heads
    Wq, Wk, Wv = mha.in_proj_weight.split(C)
    bq, bk, bv = mha.in_proj_bias.split(C)
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    heads = lambda x, L: x.reshape(B, L, H, C // H).transpose(1, 2)
    qh, kh, vh = heads(q @ Wq.T + bq, Lq), heads(k @ Wk.T + bk, Lk), heads(v @ Wv.T + bv, Lk)
    s = qh @ kh.transpose(-2, -1) / (C // H) ** 0.5
    if attn_mask is not None:
        s = s.masked_fill(attn_mask[None, None], float("-inf"))
    if key_padding_mask is not None:
        s = s.masked_fill(key_padding_mask[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, C)
    return o @ mha.out_proj.weight.T + mha.out_proj.bias


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("case", [("small", 2, True, True), ("small", 4, False, False), ("wide", 4, True, True)])
def test_composed_forward_is_the_restated_layer(flavour, case, monkeypatch):
    """fp32 on the CPU, the switch off and on (CPU tensors keep the composed path): the four statements of the issue, written out here"""
    m = I.make_layer(flavour, case[0])
    t = I.to(I.make_inputs(*case), "cpu", torch.float32)
    pos = t["pos"] if t["pos"] is not None else 0
    if flavour == "unipose":
        sa, sa_n, ta, ta_n, ca, ca_n, fc1, fc2, ffn_n, act = (m.self_attn, m.norm2, m.ca_text, m.catext_norm, m.cross_attn, m.norm1, m.linear1,
                                                              m.linear2, m.norm3, m.activation)
    else:
        sa, sa_n, ta, ta_n, ca, ca_n, fc1, fc2, ffn_n, act = (m.self_attn, m.self_attn_layer_norm, m.encoder_attn_text,
                                                              m.encoder_attn_text_layer_norm, m.encoder_attn, m.encoder_attn_layer_norm, m.fc1,
                                                              m.fc2, m.final_layer_norm, m.activation_fn)
    before = dec_calls()
    with torch.no_grad(), I.cpu_operator():
        x = t["tgt"]
        x = sa_n(x + mha_restated(sa, x + pos, x + pos, x, attn_mask=t["self_attn_mask"]))
        x = ta_n(x + mha_restated(ta, x + pos, t["memory_text"], t["memory_text"], key_padding_mask=t["text_mask"]))
        if flavour == "unipose":
            attn = ca(x + pos, t["reference_points"], t["memory"], t["spatial_shapes"], t["level_start_index"], t["padding_mask"])
        else:
            attn = ca(x, None if t["padding_mask"] is None else ~t["padding_mask"], t["memory"], None, t["pos"], t["reference_points"],
                      t["spatial_shapes"], t["level_start_index"])[0]
        x = ca_n(x + attn)
        want = ffn_n(x + fc2(act(fc1(x))))
        off = I.call(flavour, m, t)
        monkeypatch.setattr(type(m), "native_layer", True)
        on = I.call(flavour, m, t)
    assert dec_calls() == before
    assert torch.equal(on, off)
    err = (off - want).abs().max().item()
    print(f"{flavour} {case}: max |module - restated| {err:.3e} at max |out| {want.abs().max().item():.2f}")
    assert err <= 1e-4 * want.abs().max().item()          # fp32 both: the order of the sums is all that differs
    ref = I.reference(flavour, *case)
    assert (off.double() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()          # and the fp64 yardstick is the same layer


def _masked_cases():
    out = []
    for Lq, Lk in I.MHA_L:
        for B in I.MHA_B:
            for pattern in [None] + I.mha_patterns(Lq, Lk):
                for kpm in (False, True):
                    if (pattern is not None or kpm) and Lk > 1:          # (a single key is never padded: (1, 1) has no masked case)
                        out.append((Lq, Lk, B, pattern, kpm))
    return out


@pytest.mark.parametrize("Lq,Lk,B,pattern,kpm", _masked_cases())
def test_every_masked_attention_case_masks_its_share(Lq, Lk, B, pattern, kpm):
    share = I.mha_conditions(32, Lq, Lk, 1, B, pattern, kpm)
    print(f"{Lq}x{Lk} B{B} {pattern} kpm{int(kpm)}: masked pairs {share:.3f}")
    if pattern is None and B == 1:
        assert 0.15 <= share < 0.20 or Lk < 10          # the pattern's own definition: the tail 15 % of image 0 (rounded up on short rows)
        assert share <= 0.80
    else:
        assert 0.20 <= share <= 0.80
    am, kp, dead_row = I.mha_masks(pattern, kpm, Lq, Lk, B)
    if pattern == "first_tile":
        assert am[:(Lq + 1) // 2, :64].all() and not am[:, 64:].any()
    if pattern == "full_row":
        assert am[dead_row].all() and (~am).any(1).sum() == Lq - 1


def test_layer_inputs_carry_the_masks_they_say():
    for shape in I.SHAPES:
        t = I.make_inputs(shape)
        m = t["self_attn_mask"]
        assert 0.20 <= m.float().mean().item() <= 0.80 and (~m).any(1).all()          # denoising mask: no row without a key
        assert t["text_mask"].any() and (~t["text_mask"]).any(1).all()
        assert 0.10 <= t["padding_mask"].float().mean().item() <= 0.30
        n = I.make_inputs(shape, 4, False, False)
        assert n["pos"] is None and n["self_attn_mask"] is None and n["reference_points"].shape[-1] == 4
