"""CPU: the boundary of the native Grounding-DINO decoder (include/vllm_hip.h, section f2d) -- symbols, descriptor layout, the size
query, every refusal of the decoder entry and of its two row kernels (refused calls only, fake device pointers: nothing is dereferenced,
no device is touched), and the module mirror where no GPU is needed: parameter names, a state-dict round trip, every reason
``native_decoder_reasons`` has to say no, and the composed forward in fp32 against a restatement written here."""
import ctypes
import math
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import deformable_decoder as D

import deform_decoder_inputs as I
import deform_decoder_layer_inputs as LI

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
GIB = 1 << 30
NEW = ("vllm_deform_decoder_desc_sizeof", "vllm_deform_decoder_workspace_bytes", "vllm_deform_decoder_calls", "vllm_deform_decoder_forward",
       "vllm_refpoint_embed_bf16", "vllm_box_refine_f32")
OWN_POINTERS = ("ref_head_w0", "ref_head_b0", "ref_head_w1", "ref_head_b1", "layer_norm_w", "layer_norm_b", "dim_t")
BOX_POINTERS = ("w0", "b0", "w1", "b1", "w2", "b2")

# the reference's parameter names (GroundingDinoDecoder of modeling_ov_grounding_dino_mask_dn.py, three layers, bbox_embed None), in
# registration order
LAYER_NAMES = [
    "self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
    "self_attn_layer_norm.weight", "self_attn_layer_norm.bias",
    "encoder_attn_text.in_proj_weight", "encoder_attn_text.in_proj_bias", "encoder_attn_text.out_proj.weight", "encoder_attn_text.out_proj.bias",
    "encoder_attn_text_layer_norm.weight", "encoder_attn_text_layer_norm.bias",
    "encoder_attn.sampling_offsets.weight", "encoder_attn.sampling_offsets.bias", "encoder_attn.attention_weights.weight",
    "encoder_attn.attention_weights.bias", "encoder_attn.value_proj.weight", "encoder_attn.value_proj.bias",
    "encoder_attn.output_proj.weight", "encoder_attn.output_proj.bias",
    "encoder_attn_layer_norm.weight", "encoder_attn_layer_norm.bias",
    "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "final_layer_norm.weight", "final_layer_norm.bias",
]
PARAMETER_NAMES = (["layer_norm.weight", "layer_norm.bias"] + [f"layers.{i}.{n}" for i in range(3) for n in LAYER_NAMES] +
                   [f"reference_points_head.layers.{i}.{n}" for i in range(2) for n in ("weight", "bias")])

LAYER_ATTN_POINTERS = ("value_proj_w", "value_proj_b", "sampling_offsets_w", "sampling_offsets_b", "attention_weights_w", "attention_weights_b",
                       "output_proj_w", "output_proj_b")
LAYER_POINTERS = ("sa_in_proj_w", "sa_in_proj_b", "sa_out_proj_w", "sa_out_proj_b", "sa_norm_w", "sa_norm_b", "text_in_proj_w", "text_in_proj_b",
                  "text_out_proj_w", "text_out_proj_b", "text_norm_w", "text_norm_b", "ca_norm_w", "ca_norm_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
                  "ffn_norm_w", "ffn_norm_b")


def layer_desc(C=256, M=8, Lv=4, P=4, F=2048, ref_dim=4, heads=8, **ptrs):
    """a layer descriptor the layer entry accepts (fake pointers), as test_deform_decoder_layer_cpu builds it"""
    d = _lib.VllmDeformDecLayerDesc()
    a = d.cross_attn
    a.d_model, a.n_heads, a.n_levels, a.n_points, a.ref_dim = C, M, Lv, P, ref_dim
    d.d_ffn, d.act, d.n_heads_sa, d.has_self_attn, d.has_text_attn = F, 0, heads, 1, 1
    d.sa_norm_eps = d.text_norm_eps = d.ca_norm_eps = d.ffn_norm_eps = 1e-5
    for n in LAYER_ATTN_POINTERS:
        setattr(a, n, ptrs.get(n, PTR))
    for n in LAYER_POINTERS:
        setattr(d, n, ptrs.get(n, PTR))
    return d


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def last_error():
    return _lib.lib().vllm_last_error().decode()


def calls():
    return _lib.lib().vllm_deform_decoder_calls()


def layer_calls():
    return _lib.lib().vllm_deform_dec_layer_calls()


def desc(n=6, P=128, box="shared", layer_kw=(), box_ptrs=(), **own):
    """-> (descriptor, what it points to).  ``layer_kw``: {layer index: keyword arguments of the layer tests' ``desc``}; ``own``:
    n_layers / pointers of the decoder's own; ``box_ptrs``: {(layer index, name): address}"""
    layer_kw, box_ptrs = dict(layer_kw), dict(box_ptrs)
    layers = (_lib.VllmDeformDecLayerDesc * max(n, 1))()
    for i in range(n):
        layers[i] = layer_desc(**layer_kw.get(i, {}))
    d = _lib.VllmDeformDecoderDesc()
    d.n_layers, d.n_pos_feats, d.layer_norm_eps, d.inverse_sigmoid_eps = own.pop("n_layers", n), P, own.pop("layer_norm_eps", 1e-5), 1e-5
    d.layers = layers
    for name in OWN_POINTERS:
        setattr(d, name, own.pop(name, PTR))
    boxes = None
    if box is not None:
        boxes = (_lib.VllmBoxHead * max(n, 1))()
        for i in range(n):
            for name in BOX_POINTERS:
                setattr(boxes[i], name, box_ptrs.get((i, name), PTR + (4096 * (i + 1) if box == "per_layer" else 0)))
        d.box_heads = boxes
    assert not own, own
    return d, (layers, boxes)


def forward(d, B=2, Lq=130, Lt=9, S=161, tgt=PTR, ref=PTR + GIB, vr=PTR + 2 * GIB, text=PTR + 3 * GIB, memory=PTR + 4 * GIB, shapes=PTR, lsi=PTR,
            inter=PTR + 5 * GIB, irp=PTR + 6 * GIB, ws=PTR + 7 * GIB, ws_bytes=1 << 40):
    return _lib.lib().vllm_deform_decoder_forward(ctypes.byref(d), vp(tgt), vp(ref), vp(vr), None, vp(text), None, vp(memory), None, vp(shapes),
                                                  vp(lsi), B, Lq, Lt, S, vp(inter), vp(irp), vp(ws), ws_bytes, None)


def query(d, B=2, Lq=130, Lt=9, S=161):
    return _lib.lib().vllm_deform_decoder_workspace_bytes(ctypes.byref(d), B, Lq, Lt, S)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T vllm_" in line}
    for n in NEW:
        assert n in protos, n
        assert n in exported, n
    assert _lib.header_abi_version() == 2 and _lib.lib().vllm_abi_version() == 2          # additions only
    hdr = open(_lib.HEADER).read()
    assert "f2d. The whole Grounding-DINO DECODER" in hdr
    for n in ("vllm_deform_decoder_forward", "vllm_refpoint_embed_bf16"):
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + n + r"\s*\(", hdr, flags=re.S), f"no 'Alignment' line directly above {n}"


def test_descriptor_mirrors_have_the_library_size_and_the_header_order():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.VllmDeformDecoderDesc) == L.vllm_deform_decoder_desc_sizeof()
    _lib.check_struct_layouts()
    hdr = open(_lib.HEADER).read()
    for cls, name in ((_lib.VllmDeformDecoderDesc, "VllmDeformDecoderDesc"), (_lib.VllmBoxHead, "VllmBoxHead")):
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        order = [re.search(r"\b" + n + r"\b", body).start() for n, _ in cls._fields_]
        assert order == sorted(order), f"{name}: field order differs from include/vllm_hip.h"
    assert ctypes.sizeof(_lib.VllmBoxHead) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert calls() >= 0


def test_workspace_query_is_the_sum_of_its_pieces_and_monotone():
    L = _lib.lib()
    d, keep = desc()
    a256 = lambda x: (x + 255) & ~255
    base = query(d)
    layer = L.vllm_deform_dec_layer_workspace_bytes(ctypes.byref(keep[0][0]), 2, 130, 9, 161)
    R, C, P, Lv = 260, 256, 128, 4
    # one layer's workspace, the hidden state twice, sine, two MLP intermediates, query_pos, reference_points_input
    assert layer > 0 and base == a256(layer) + 5 * a256(R * C * 2) + a256(R * 4 * P * 2) + a256(R * Lv * 16)
    no_box, _k = desc(box=None)
    assert query(no_box) == base - a256(R * C * 2)
    # the LARGEST layer's workspace serves every layer
    wide, keep_w = desc(layer_kw={3: dict(F=4096)})
    assert query(wide) - base == a256(L.vllm_deform_dec_layer_workspace_bytes(ctypes.byref(keep_w[0][3]), 2, 130, 9, 161)) - a256(layer)
    one, _k1 = desc(n=1)
    assert query(one) == base          # a layer more costs nothing
    assert query(d, B=3) > base and query(d, Lq=131) > base and query(d, Lt=10) > base and query(d, S=162) > base and query(d) == base
    assert query(d, B=0) == 0 and query(d, Lq=0) == 0
    assert query(d, B=-1) < 0 and query(d, Lt=-1) < 0 and query(d, B=1 << 16, Lq=1 << 15) < 0 and "2^31" in last_error()
    assert L.vllm_deform_decoder_workspace_bytes(None, 2, 130, 9, 161) < 0 and "null descriptor" in last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(n_layers=0), "n_layers"),
    (dict(n_layers=65), "n_layers"),
    (dict(P=0), "n_pos_feats"),
    (dict(P=8), "n_pos_feats"),
    (dict(P=127), "n_pos_feats"),
    (dict(layer_kw={0: dict(ref_dim=2)}), "4-d reference points"),
    (dict(layer_kw={2: dict(ref_dim=2)}), "layer 2 has ref_dim=2"),
    (dict(layer_kw={1: dict(ref_dim=3)}), "reference_points must be 2 or 4"),          # the attention layer's own gate
    (dict(layer_kw={4: dict(C=128, M=4, heads=4)}), "layer 4 has d_model=128"),
    (dict(layer_kw={5: dict(Lv=2, P=8)}), "n_levels=2"),
    (dict(layer_kw={3: dict(F=2000)}), "d_ffn"),                                       # a layer descriptor its own entry refuses
    (dict(layer_kw={1: dict(heads=16)}), "head dim 32 or 64"),
    (dict(layer_norm_eps=-1.0), "negative eps"),
] + [({name: 0}, "missing weights") for name in OWN_POINTERS] + [(dict(box_ptrs={(4, name): 0}), "box head 4") for name in BOX_POINTERS],
    ids=lambda v: None if isinstance(v, dict) else v.replace(" ", "_"))
def test_refused_descriptors_have_their_own_messages(kw, word):
    d, keep = desc(**kw)
    before, before_layer = calls(), layer_calls()
    assert query(d) < 0
    assert word in last_error(), last_error()
    assert forward(d) == EINVAL
    assert word in last_error() and "workspace" not in last_error(), last_error()
    assert (calls(), layer_calls()) == (before, before_layer)


def test_a_null_layer_array_is_refused():
    d, keep = desc()
    d.layers = ctypes.POINTER(_lib.VllmDeformDecLayerDesc)()
    assert query(d) < 0 and "n_layers" in last_error()
    assert forward(d) == EINVAL and "n_layers" in last_error()


def test_null_misaligned_and_overlapping_operands_have_their_own_messages():
    d, keep = desc()
    before, before_layer = calls(), layer_calls()
    for kw in (dict(tgt=0), dict(ref=0), dict(vr=0), dict(inter=0), dict(irp=0), dict(text=0), dict(memory=0), dict(shapes=0), dict(lsi=0)):
        assert forward(d, **kw) == EINVAL, kw
        assert "null pointer" in last_error() and "workspace" not in last_error(), (kw, last_error())
    for kw in (dict(tgt=PTR + 8), dict(ref=PTR + GIB + 8), dict(vr=PTR + 2 * GIB + 4), dict(inter=PTR + 5 * GIB + 8), dict(irp=PTR + 6 * GIB + 8)):
        assert forward(d, **kw) == EINVAL, kw
        assert "deform_decoder: misaligned tgt" in last_error(), (kw, last_error())
    assert forward(d, vr=PTR + 2 * GIB + 8, ws_bytes=0) == EINVAL and "workspace" in last_error()          # valid_ratios: 8 bytes do
    for kw in (dict(text=PTR + 3 * GIB + 8), dict(memory=PTR + 4 * GIB + 8)):          # the layer's own gate, on the operands it will get
        assert forward(d, **kw) == EINVAL and "deform_dec_layer: misaligned tgt" in last_error(), (kw, last_error())
    dd, _k = desc(dim_t=PTR + 8)
    assert forward(dd) == EINVAL and "deform_decoder: misaligned tgt" in last_error()
    for name in OWN_POINTERS[:-1]:
        dd, _k = desc(**{name: PTR + 8})
        assert forward(dd) == EINVAL and "deform_decoder: misaligned weight or bias" in last_error(), (name, last_error())
    for name in BOX_POINTERS:
        dd, _k = desc(box_ptrs={(2, name): PTR + 4})
        assert forward(dd) == EINVAL and "box head 2" in last_error(), (name, last_error())
    dd, _k = desc(box_ptrs={(2, "b2"): PTR + 8})
    assert forward(dd, ws_bytes=0) == EINVAL and "workspace" in last_error()                                 # the four-element bias: 8 bytes do
    dd, _k = desc(layer_kw={3: dict(fc1_w=PTR + 8)})
    assert forward(dd) == EINVAL and "deform_dec_layer: misaligned weight or bias" in last_error()
    R, C, n = 260, 256, 6
    ibytes, rbytes = n * R * C * 2, n * R * 16
    for kw in (dict(inter=PTR), dict(inter=PTR - ibytes + 16), dict(inter=PTR + GIB), dict(inter=PTR + 2 * GIB), dict(inter=PTR + 3 * GIB),
               dict(inter=PTR + 4 * GIB + 4096), dict(irp=PTR + R * C * 2 - 16), dict(irp=PTR + GIB - rbytes + 16), dict(irp=PTR + 2 * GIB + 16),
               dict(irp=PTR + 3 * GIB), dict(irp=PTR + 4 * GIB)):
        assert forward(d, **kw) == EINVAL, kw
        assert "an output overlaps an input" in last_error() and "workspace" not in last_error(), (kw, last_error())
    for kw in (dict(irp=PTR + 5 * GIB), dict(irp=PTR + 5 * GIB + ibytes - 16), dict(inter=PTR + 6 * GIB + rbytes - 16)):
        assert forward(d, **kw) == EINVAL and "the two outputs overlap" in last_error(), (kw, last_error())
    assert forward(d, irp=PTR + 5 * GIB + ibytes, ws_bytes=0) == EINVAL and "workspace" in last_error()     # back to back is no overlap
    assert forward(d, B=1 << 16, Lq=1 << 15) == EINVAL and "2^31" in last_error()
    assert forward(d, B=-1) == EINVAL and "2^31" in last_error()
    wide, _k = desc(P=2048, layer_kw={i: dict(F=64) for i in range(6)})          # 16 KiB of sine per row: 2^17 rows reach 2^31 bytes
    assert forward(wide, B=1 << 7, Lq=1 << 10) == EINVAL and "sine embedding reach 2^31" in last_error()
    assert query(wide, B=1 << 7, Lq=1 << 10) < 0
    assert forward(d, S=0) == EINVAL and "empty" in last_error()
    assert forward(d, Lt=0) == EINVAL and "empty" in last_error()
    # B Lq == 0: nothing to do, whatever the pointers are
    assert forward(d, B=0, tgt=0, inter=0, irp=0, ws=0, ws_bytes=0) == 0 and forward(d, Lq=0, tgt=0, ref=0, ws=0, ws_bytes=0) == 0
    assert (calls(), layer_calls()) == (before, before_layer)          # no refused call reached a launch


def test_short_misaligned_and_null_workspaces_are_refused():
    for d, keep in (desc(), desc(box=None), desc(n=1, box="per_layer")):
        need = query(d)
        assert need > 0
        before = calls()
        base = PTR + 7 * GIB
        for w, n in ((base, need - 1), (base + 8, need), (base + 8, need + 4096), (0, need)):
            assert forward(d, ws=w, ws_bytes=n) == EINVAL
            assert "deform_decoder: workspace" in last_error(), last_error()
        assert calls() == before


def test_the_row_kernels_refuse_what_they_cannot_run():
    """every refusal of vllm_refpoint_embed_bf16 and vllm_box_refine_f32 is decided on the host: fake pointers, no device"""
    L = _lib.lib()

    def embed(ref=PTR, vr=PTR, dim_t=PTR, B=2, Lq=37, Lv=4, ref_dim=4, P=32, rpi=PTR, sine=PTR, ld=128):
        return L.vllm_refpoint_embed_bf16(vp(ref), vp(vr), vp(dim_t), B, Lq, Lv, ref_dim, P, vp(rpi), vp(sine), ld, None)
    for rd in (2, 3, 0):
        assert embed(ref_dim=rd) == EINVAL and "4-d reference points only" in last_error(), rd
    for P in (31, 4, 12, 0, -8):
        assert embed(P=P, ld=1024) == EINVAL and "multiple of 8" in last_error(), P
    for kw in (dict(ref=0), dict(vr=0), dict(dim_t=0), dict(rpi=0), dict(sine=0)):
        assert embed(**kw) == EINVAL and "null pointer" in last_error(), kw
    for kw in (dict(ref=PTR + 8), dict(vr=PTR + 4), dict(dim_t=PTR + 4), dict(rpi=PTR + 8), dict(sine=PTR + 8), dict(ld=120), dict(ld=132)):
        assert embed(**kw) == EINVAL and "misaligned operand" in last_error(), (kw, last_error())
    assert embed(Lv=0) == EINVAL and embed(B=-1) == EINVAL
    assert embed(B=0, ref=0, sine=0) == 0 and embed(Lq=0, ref=0, rpi=0) == 0

    def refine(h=PTR, ldh=256, W=PTR, b=PTR, ref=PTR + GIB, new=PTR + 2 * GIB, R=37, C=256, eps=1e-5):
        return L.vllm_box_refine_f32(vp(h), ldh, vp(W), vp(b), vp(ref), vp(new), R, C, eps, None)
    for C in (0, 32, 96, 576, 1024):
        assert refine(C=C, ldh=1024) == EINVAL and "multiple of 64 in 64 .. 512" in last_error(), C
    for kw in (dict(h=0), dict(W=0), dict(b=0), dict(ref=0), dict(new=0)):
        assert refine(**kw) == EINVAL and "null pointer" in last_error(), kw
    for kw in (dict(h=PTR + 8), dict(W=PTR + 8), dict(b=PTR + 4), dict(ref=PTR + GIB + 8), dict(new=PTR + 2 * GIB + 8), dict(ldh=248), dict(ldh=260)):
        assert refine(**kw) == EINVAL and "misaligned operand" in last_error(), (kw, last_error())
    assert refine(new=PTR + GIB + 16) == EINVAL and "overlaps ref without being ref" in last_error()
    assert refine(R=-1) == EINVAL
    assert refine(R=0, h=0, new=0) == 0


# ---- the module mirror ----------------------------------------------------------------------------------------------------------------------------
def test_constructor_takes_the_reference_arguments_and_names():
    m = I.make_decoder()
    assert [n for n, _ in m.named_parameters()] == PARAMETER_NAMES
    assert isinstance(m.layer_norm, nn.LayerNorm) and len(m.layers) == 3 and all(isinstance(l, D.GroundingDinoDecoderLayer) for l in m.layers)
    assert isinstance(m.reference_points_head, D.GroundingDinoMLPPredictionHead) and m.reference_points_head.num_layers == 2
    assert [tuple(l.weight.shape) for l in m.reference_points_head.layers] == [(64, 128), (64, 64)]
    assert m.bbox_embed is None and m.class_embed is None and m.query_scale is None and m.native_decoder is False
    assert m.dropout == 0.1 and m.gradient_checkpointing is False
    from visionllm_amd import GroundingDinoDecoder, GroundingDinoMLPPredictionHead
    assert GroundingDinoDecoder is D.GroundingDinoDecoder and GroundingDinoMLPPredictionHead is D.GroundingDinoMLPPredictionHead


def test_state_dict_round_trip():
    a, b = I.make_decoder("per_layer"), D.GroundingDinoDecoder(I.config())
    b.bbox_embed = nn.ModuleList(D.GroundingDinoMLPPredictionHead(64, 64, 4, 3) for _ in range(3))
    sd = a.state_dict()
    assert [k for k in sd if not k.startswith("bbox_embed.")] == PARAMETER_NAMES
    assert [k for k in sd if k.startswith("bbox_embed.")] == [f"bbox_embed.{i}.layers.{j}.{n}" for i in range(3) for j in range(3)
                                                               for n in ("weight", "bias")]
    missing, unexpected = b.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    t = I.make_inputs(37)
    tf = I.to(t, "cpu", torch.float32)
    with torch.no_grad(), LI.cpu_operator():
        for x, y in zip(I.call(a, tf), I.call(b.eval(), tf)):
            assert torch.equal(x, y)


def test_get_proposal_pos_embed_is_the_reference_formula():
    m = I.make_decoder()
    g = torch.Generator().manual_seed(5)
    prop = torch.rand(2, 7, 4, generator=g)
    pos = m.get_proposal_pos_embed(prop)
    assert pos.shape == (2, 7, 128) and pos.dtype == torch.float32
    dim_t = torch.tensor([10000.0 ** (2 * (i // 2) / 32) for i in range(32)], dtype=torch.float64)
    for grp, k in enumerate((1, 0, 2, 3)):          # y, x, w, h
        arg = prop[:, :, k, None].double() * (2 * math.pi) / dim_t
        want = torch.where(torch.arange(32) % 2 == 0, arg.sin(), arg.cos())
        assert torch.allclose(pos[:, :, 32 * grp:32 * grp + 32].double(), want, atol=2e-6, rtol=0)
    assert m.get_proposal_pos_embed(prop[:, :, :2]).shape == (2, 7, 64)
    assert torch.equal(m.get_proposal_pos_embed(prop[:, :, :2]), pos[:, :, :64])
    with pytest.raises(ValueError):
        m.get_proposal_pos_embed(prop[:, :, :3])


def restated(m, t):
    """GroundingDinoDecoder.forward said again with torch.nn.functional only (4-d reference points; the layers through their own forward,
    which test_deform_decoder_layer_cpu restates) -> (last, intermediate [B, n, Lq, C], reference points [B, n, Lq, 4])"""
    x, ref, vr = t["tgt"], t["reference_points"], t["valid_ratios"]
    P = x.shape[-1] // 2
    dim_t = torch.tensor([10000.0 ** (2 * (i // 2) / P) for i in range(P)], dtype=torch.float64).to(x.dtype)
    even = torch.arange(P) % 2 == 0
    inter, refs = [], []
    for i, layer in enumerate(m.layers):
        ref_in = torch.stack([ref * torch.stack([vr[:, l, 0], vr[:, l, 1], vr[:, l, 0], vr[:, l, 1]], -1)[:, None] for l in range(vr.shape[1])], 2)
        lvl0 = ref_in[:, :, 0]
        groups = []
        for k in (1, 0, 2, 3):
            arg = lvl0[:, :, k, None] * (2 * math.pi) / dim_t
            groups.append(torch.where(even, arg.sin(), arg.cos()))
        sine = torch.cat(groups, -1).to(x.dtype)
        h0, h1 = m.reference_points_head.layers
        pos = F.linear(F.relu(F.linear(sine, h0.weight, h0.bias)), h1.weight, h1.bias)
        x = layer(x, pos, ref_in, t["spatial_shapes"], t["level_start_index"], t["memory"], t["attention_mask"], t["memory_text"], t["text_mask"],
                  t["self_attn_mask"])[0]
        if m.bbox_embed is not None:
            b0, b1, b2 = m.bbox_embed[i].layers
            delta = F.linear(F.relu(F.linear(F.relu(F.linear(x, b0.weight, b0.bias)), b1.weight, b1.bias)), b2.weight, b2.bias)
            c = ref.clamp(0, 1)
            ref = torch.sigmoid(delta + torch.log(c.clamp(min=1e-5) / (1 - c).clamp(min=1e-5)))
        inter.append(F.layer_norm(x, (x.shape[-1],), m.layer_norm.weight, m.layer_norm.bias, m.layer_norm.eps))
        refs.append(ref)
    return inter[-1], torch.stack(inter, 1), torch.stack(refs, 1)


@pytest.mark.parametrize("box", I.BOXES, ids=[f"box_{b}" for b in I.BOXES])
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
def test_composed_forward_equals_a_restatement(with_masks, box):
    m = I.make_decoder(box)
    t = I.to(I.make_inputs(37, with_masks), "cpu", torch.float32)
    with torch.no_grad(), LI.cpu_operator():
        got = I.call(m, t)
        want = restated(m, t)
        as_dict = I.call(m, t, return_dict=True)
    assert isinstance(got, tuple) and len(got) == 3
    assert got[1].shape == (I.B, I.LAYERS, 37, I.C) and got[2].shape == (I.B, I.LAYERS, 37, 4)
    for g, w, name in zip(got, want, ("last_hidden_state", "intermediate", "reference points")):
        assert g.dtype == torch.float32 and g.shape == w.shape
        err = (g - w).abs().max().item()
        print(f"{name}: max |composed - restated| {err:.3e}")
        # fp32 and the same operations: only the order of two products (ref * ratio * 2 pi) and the fp64-built table may differ
        assert err <= 2e-5 * max(1.0, w.abs().max().item()), name
    assert torch.equal(got[0], got[1][:, -1])
    if box is None:
        assert torch.equal(got[2], t["reference_points"][:, None].expand(-1, I.LAYERS, -1, -1))
    assert isinstance(as_dict, D.GroundingDinoDecoderOutput) and as_dict.hidden_states is None and as_dict.attentions is None
    assert torch.equal(as_dict.last_hidden_state, got[0]) and torch.equal(as_dict.intermediate_hidden_states, got[1]) and \
        torch.equal(as_dict.intermediate_reference_points, got[2])
    assert [f.name for f in __import__("dataclasses").fields(as_dict)] == ["last_hidden_state", "intermediate_hidden_states",
                                                                           "intermediate_reference_points", "hidden_states", "attentions"]


def test_composed_forward_returns_the_optional_outputs():
    m = I.make_decoder("shared")
    t = I.to(I.make_inputs(37), "cpu", torch.float32)
    with torch.no_grad(), LI.cpu_operator():
        out = I.call(m, t, output_hidden_states=True, output_attentions=True)
        assert len(out) == 5 and len(out[3]) == I.LAYERS + 1 and len(out[4]) == 3 and all(len(a) == I.LAYERS for a in out[4])
        assert out[4][0][0].shape == (I.B, I.HEADS, 37, 37) and out[4][1][0].shape == (I.B, I.HEADS, 37, I.LT)
        assert torch.equal(out[3][-1], out[0])
        with pytest.raises(ValueError, match="must be of size 2"):
            I.call(m, dict(t, reference_points=t["reference_points"][..., :3].contiguous()))


class FakeCuda(torch.Tensor):
    """a CPU tensor that says it is on the GPU: the reasons are decided from dtypes, shapes and flags alone"""
    @property
    def is_cuda(self):
        return True


def fake(t):
    return None if t is None else t.as_subclass(FakeCuda)


def fake_params(m):
    for mod in m.modules():
        for k, p in list(mod._parameters.items()):
            if p is not None:
                mod._parameters[k] = nn.Parameter(p.data, requires_grad=p.requires_grad).as_subclass(FakeCuda)
    return m


def fake_module(m):
    return fake_params(I.as_bf16(m, "cpu"))


def test_every_reason_to_keep_the_composed_path():
    t32 = I.make_inputs(37)
    t = {k: fake(v) for k, v in I.to(t32, "cpu").items()}
    with torch.no_grad():
        m = fake_module(I.make_decoder("shared"))
        assert I.reasons(m, t) == []                                           # the baseline: nothing to object to
        assert I.reasons(fake_module(I.make_decoder()), t) == [] and I.reasons(fake_module(I.make_decoder("per_layer")), t) == []
        assert I.reasons(m, dict(t, reference_points=fake(t32["reference_points"].to(torch.bfloat16)))) == []
        no_masks = {k: fake(v) for k, v in I.to(I.make_inputs(37, False), "cpu").items()}
        assert I.reasons(m, no_masks) == []

        def one(why, mod=m, tt=t, **kw):
            got = I.reasons(mod, tt, **kw)
            assert any(why in r for r in got), (why, got)
            return got
        m.train()
        got = one("training mode")
        assert any(r.startswith("layers.0: active dropout") for r in got)
        m.eval()
        one("output_attentions", output_attentions=True)
        one("output_hidden_states", output_hidden_states=True)
        one("reference_points: [B, Lq, 4]", tt=dict(t, reference_points=fake(t32["reference_points"][..., :2].contiguous())))
        one("reference_points: an fp32 or bf16 CUDA tensor", tt=dict(t, reference_points=t32["reference_points"]))             # on the CPU
        one("reference_points: an fp32 or bf16 CUDA tensor", tt=dict(t, reference_points=fake(t32["reference_points"].double())))
        one("reference_points: an fp32 or bf16 CUDA tensor", tt=dict(t, reference_points=fake(t32["reference_points"][:, :5].contiguous())))
        one("valid_ratios", tt=dict(t, valid_ratios=t32["valid_ratios"]))
        one("valid_ratios", tt=dict(t, valid_ratios=fake(t32["valid_ratios"][:, :1].contiguous())))
        one("valid_ratios", tt=dict(t, valid_ratios=None))
        one("inputs_embeds / vision_encoder_hidden_states", tt=dict(t, tgt=fake(t32["tgt"].float())))
        one("inputs_embeds / vision_encoder_hidden_states", tt=dict(t, memory=I.to(t32, "cpu")["memory"]))                       # on the CPU
        one("vision_encoder_attention_mask", tt=dict(t, attention_mask=fake(t32["attention_mask"].float())))
        got = one("layers.1: self_attn_mask", tt=dict(t, self_attn_mask=fake(t32["self_attn_mask"].float())))
        assert sum("self_attn_mask" in r for r in got) == I.LAYERS                                                               # every layer says so
        f32 = fake_params(I.make_decoder("shared"))
        got = one("parameters: bf16 on the GPU", mod=f32)
        assert any(r.startswith("layers.2: parameters: bf16 on the GPU") for r in got)
        one("parameters: bf16 on the GPU", mod=I.as_bf16(I.make_decoder("shared"), "cpu"))                                      # bf16, on the CPU
        m.query_scale = nn.Identity()
        one("query_scale")
        m.query_scale = None
        good = m.bbox_embed
        for bad in (nn.ModuleList(list(good)[:2]), [nn.Linear(64, 4)] * 3, [D.GroundingDinoMLPPredictionHead(64, 64, 4, 2)] * 3,
                    [D.GroundingDinoMLPPredictionHead(64, 32, 4, 3)] * 3, [D.GroundingDinoMLPPredictionHead(64, 64, 2, 3)] * 3, good[0]):
            del m.bbox_embed          # (a registered child module cannot be overwritten by a plain list)
            m.bbox_embed = bad
            one("bbox_embed: None or 3 three-layer heads of width d_model")
        del m.bbox_embed
        m.bbox_embed = good
        assert I.reasons(m, t) == []
        one("query_dim 4", mod=fake_module(I.make_decoder(query_dim=2)))
    one("requires_grad under grad mode")                                       # grad mode, trainable parameters
    frozen = fake_module(I.make_decoder("shared").requires_grad_(False))
    assert I.reasons(frozen, t) == []                                          # frozen: grad mode alone is no reason
    x = fake(I.to(t32, "cpu")["tgt"].float().requires_grad_(True).to(torch.bfloat16))
    assert x.requires_grad
    one("requires_grad under grad mode", mod=frozen, tt=dict(t, tgt=x))


def test_the_switch_is_off_by_default_and_the_cpu_never_takes_the_native_call(monkeypatch):
    assert D.GroundingDinoDecoder.native_decoder is False
    m = I.make_decoder("shared")
    t = I.to(I.make_inputs(37), "cpu", torch.float32)
    monkeypatch.setattr(D.GroundingDinoDecoder, "native_decoder", True)
    before = calls()
    with torch.no_grad(), LI.cpu_operator():
        on = I.call(m, t)
        monkeypatch.setattr(D.GroundingDinoDecoder, "native_decoder", False)
        off = I.call(m, t)
    assert calls() == before and I.reasons(m, t) != []
    for a, b in zip(on, off):
        assert torch.equal(a, b)
