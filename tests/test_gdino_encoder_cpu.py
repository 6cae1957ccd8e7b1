"""CPU: the Grounding-DINO text enhancer and encoder (include/vllm_hip.h, section f2g; visionllm_amd/gdino_encoder.py) where no GPU is
needed -- symbols, the two tagged descriptors against the library's sizeof and the C compiler's layout, the size queries, every refusal
of the five new entries (fake pointers: a refused call dereferences nothing and touches no device), the mirrors' constructor arguments
and parameter names against the golden's state-dict keys, the mirrors in fp64 against tests/golden/gdino_encoder.npz (made by RUNNING
the reference, tools/gen_golden_gdino_encoder.py), every reason that keeps the composed path, the mask quirk of the reference's
``repeat``, and the conditions the GPU tests' inputs must show on the fp64 run."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import gdino_encoder as G

import gdino_encoder_inputs as I
from deform_encoder_layer_inputs import cpu_operator

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gdino_encoder.npz")
NEW = ("vllm_text_enhancer_desc_sizeof", "vllm_gdino_encoder_desc_sizeof", "vllm_text_enhancer_workspace_bytes",
       "vllm_gdino_encoder_workspace_bytes", "vllm_text_enhancer_calls", "vllm_gdino_encoder_calls", "vllm_text_enhancer_forward",
       "vllm_gdino_encoder_forward", "vllm_mha_fwd_masks_bf16", "vllm_text_pos_embed_bf16", "vllm_encoder_refpoints_f32")
ENTRIES = ("vllm_text_enhancer_forward", "vllm_gdino_encoder_forward", "vllm_mha_fwd_masks_bf16", "vllm_text_pos_embed_bf16",
           "vllm_encoder_refpoints_f32")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def err():
    return _lib.lib().vllm_last_error().decode()


def counters():
    L = _lib.lib()
    return (L.vllm_text_enhancer_calls(), L.vllm_gdino_encoder_calls(), L.vllm_fusion_layer_calls(), L.vllm_deform_enc_layer_calls())


# ---- descriptors with fake pointers ---------------------------------------------------------------------------------------------------------------
def enh_desc(C=64, H=2, F=256, act=0, **kw):
    d = _lib.VllmTextEnhancerDesc()
    d.d_model, d.n_heads, d.d_ffn, d.act, d.norm_before_eps, d.norm_after_eps = C, H, F, act, 1e-5, 1e-5
    for n in _lib.pointer_fields(_lib.VllmTextEnhancerDesc):
        setattr(d, n, kw.get(n, PTR))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def fusion_desc(C=64, E=256, H=2):
    d = _lib.VllmFusionLayerDesc()
    d.d_model, d.embed_dim, d.n_heads, d.vision_norm_eps, d.text_norm_eps = C, E, H, 1e-5, 1e-5
    for n in _lib.pointer_fields(_lib.VllmFusionLayerDesc):
        setattr(d, n, PTR)
    return d


def deform_desc(C=64, M=4, Lv=2, P=4, F=512):
    d = _lib.VllmDeformEncLayerDesc()
    a = d.attn
    a.d_model, a.n_heads, a.n_levels, a.n_points, a.ref_dim = C, M, Lv, P, 2
    d.d_ffn, d.act, d.norm1_eps, d.norm2_eps = F, 0, 1e-5, 1e-5
    for n in _lib.pointer_fields(_lib.VllmMsdaLayerDesc):
        setattr(a, n, PTR)
    for n in _lib.pointer_fields(_lib.VllmDeformEncLayerDesc):
        setattr(d, n, PTR)
    return d


def encoder_desc(n=2, dim_t=PTR, fusion=None, enhancer=None, deformable=None):
    """-> (descriptor, the arrays it points to: keep them alive)"""
    fus, enh, dfm = (_lib.VllmFusionLayerDesc * n)(), (_lib.VllmTextEnhancerDesc * n)(), (_lib.VllmDeformEncLayerDesc * n)()
    for i in range(n):
        fus[i], enh[i], dfm[i] = (fusion or fusion_desc)(), (enhancer or enh_desc)(), (deformable or deform_desc)()
    d = _lib.VllmGdinoEncoderDesc()
    d.n_layers, d.fusion, d.enhancer, d.deformable, d.dim_t = n, fus, enh, dfm, dim_t
    return d, (fus, enh, dfm)


def enh_forward(d, text=PTR, pos=PTR, mask=PTR, n_masks=1, B=2, Lt=5, out=PTR + (1 << 16), ws=PTR + (1 << 18), ws_bytes=1 << 40):
    return _lib.lib().vllm_text_enhancer_forward(ctypes.byref(d) if d is not None else None, vp(text), vp(pos), vp(mask), n_masks, B, Lt, vp(out),
                                                 vp(ws), ws_bytes, None)


A = dict(vision=PTR, vision_pos=PTR + (1 << 16), vmask=PTR, vr=PTR + (2 << 16), shapes=PTR, lsi=PTR, text=PTR + (3 << 16), tmask=PTR, sam=PTR,
         n_masks=2, positions=PTR + (4 << 16), emb=0, B=2, S=36, Lt=5, out_vision=PTR + (5 << 16), out_text=PTR + (6 << 16), ws=1 << 30,
         ws_bytes=1 << 40)


def enc_forward(d, **kw):
    a = dict(A, **kw)
    return _lib.lib().vllm_gdino_encoder_forward(
        ctypes.byref(d) if d is not None else None, vp(a["vision"]), vp(a["vision_pos"]), vp(a["vmask"]), vp(a["vr"]), vp(a["shapes"]),
        vp(a["lsi"]), vp(a["text"]), vp(a["tmask"]), vp(a["sam"]), a["n_masks"], vp(a["positions"]), vp(a["emb"]), a["B"], a["S"], a["Lt"],
        vp(a["out_vision"]), vp(a["out_text"]), vp(a["ws"]), a["ws_bytes"], None)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T vllm_" in line}
    for n in NEW:
        assert n in protos and n in exported, n
    assert _lib.header_abi_version() == 2 and _lib.lib().vllm_abi_version() == 2          # additions only
    hdr = open(_lib.HEADER).read()
    assert "f2g. The TEXT ENHANCER" in hdr and "THE MASK OF THE ENHANCER" in hdr
    for lines in ("mask_dn.py:787-857", ":1185-1290", ":1560-1722"):
        assert lines in hdr
    for n in ENTRIES:
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + n + r"\s*\(", hdr, flags=re.S), f"no 'Alignment' line directly above {n}"


def test_descriptors_have_the_library_size_and_the_c_compilers_layout(tmp_path):
    L = _lib.lib()
    structs = _lib.GDINO_ENCODER_STRUCTS
    assert list(structs) == ["VllmTextEnhancerDesc", "VllmGdinoEncoderDesc"]
    assert list(_lib.parse_tagged_structs(_lib.GDINO_ENCODER_HEADER, {**_lib.STRUCTS, **_lib.TAGGED_STRUCTS})) == list(structs)
    assert ctypes.sizeof(_lib.VllmTextEnhancerDesc) == L.vllm_text_enhancer_desc_sizeof()
    assert ctypes.sizeof(_lib.VllmGdinoEncoderDesc) == L.vllm_gdino_encoder_desc_sizeof()
    f = dict(_lib.VllmGdinoEncoderDesc._fields_)
    assert f["fusion"] is ctypes.POINTER(_lib.VllmFusionLayerDesc) and f["enhancer"] is ctypes.POINTER(_lib.VllmTextEnhancerDesc)
    assert f["deformable"] is ctypes.POINTER(_lib.VllmDeformEncLayerDesc) and f["dim_t"] is ctypes.c_void_p
    assert _lib.pointer_fields(_lib.VllmTextEnhancerDesc) == (
        "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "norm_before_w", "norm_before_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
        "norm_after_w", "norm_after_b")
    protos = _lib.parse_header()
    with pytest.raises(RuntimeError, match="vllm_text_enhancer_desc_sizeof"):          # the load insists on the export
        _lib._check_struct_layouts(L, {k: v for k, v in protos.items() if k != "vllm_text_enhancer_desc_sizeof"})
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if not cc:
        pytest.skip("no host C compiler")
    lines, want = [], {}
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof(struct {name}));')
        want[name] = ctypes.sizeof(cls)
        for member, _ in cls._fields_:
            lines.append(f'printf("{name}.{member} %zu\\n", offsetof(struct {name}, {member}));')
            want[f"{name}.{member}"] = getattr(cls, member).offset
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vllm_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(tmp_path / "layout")], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout
    assert {k: int(v) for k, v in (ln.split() for ln in out.splitlines())} == want and len(want) == 26


def test_size_queries_are_monotone_multiples_of_16_and_zero_for_nothing():
    L = _lib.lib()
    e = enh_desc()
    q = lambda b, lt: L.vllm_text_enhancer_workspace_bytes(ctypes.byref(e), b, lt)
    assert q(0, 5) == 0 and q(3, 0) == 0
    sizes = [q(b, lt) for b, lt in ((1, 1), (1, 5), (2, 5), (2, 70), (8, 256))]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) >= 4
    assert q(-1, 5) < 0 and "B=-1" in err()
    assert L.vllm_text_enhancer_workspace_bytes(None, 1, 1) < 0 and "null descriptor" in err()
    assert L.vllm_text_enhancer_workspace_bytes(ctypes.byref(enh_desc(H=4)), 1, 1) < 0 and "head dim 32 or 64" in err()
    d, keep = encoder_desc()
    Q = lambda b, s, lt: L.vllm_gdino_encoder_workspace_bytes(ctypes.byref(d), b, s, lt)
    assert Q(0, 36, 5) == 0 and Q(2, 0, 5) == 0 and Q(2, 36, 0) == 0
    sizes = [Q(b, s, lt) for b, s, lt in ((1, 36, 1), (1, 36, 5), (2, 36, 5), (2, 76, 5), (2, 76, 70), (8, 1000, 256))]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    # one block's workspace serves all three blocks: the encoder asks for less than the sum of its parts and more than the largest
    parts = [L.vllm_fusion_layer_workspace_bytes(ctypes.byref(keep[0][0]), 2, 36, 5), q(2, 5),
             L.vllm_deform_enc_layer_workspace_bytes(ctypes.byref(keep[2][0]), 2, 36)]
    assert max(parts) < Q(2, 36, 5) < sum(parts) + (1 << 16)
    assert Q(-1, 36, 5) < 0 and L.vllm_gdino_encoder_workspace_bytes(None, 1, 1, 1) < 0 and "null descriptor" in err()


# ---- refusals: nothing is enqueued, no counter moves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(C=96), "d_model=96"), (dict(C=576, H=9), "d_model=576"), (dict(H=4), "head dim 32 or 64"), (dict(H=0), "head dim 32 or 64"),
    (dict(F=100), "d_ffn=100"), (dict(act=5), "unknown act 5"), (dict(norm_before_eps=-1.0), "negative eps"),
    (dict(norm_after_eps=-1.0), "negative eps"), (dict(in_proj_w=0), "missing weights"), (dict(fc2_b=0), "missing weights"),
    (dict(norm_after_w=0), "missing weights"),
])
def test_enhancer_refuses_a_bad_descriptor(kw, word):
    before = counters()
    assert enh_forward(enh_desc(**kw)) == EINVAL and word in err(), err()
    assert counters() == before


def test_enhancer_refuses_bad_operands_and_workspaces():
    L = _lib.lib()
    d = enh_desc()
    before = counters()
    need = L.vllm_text_enhancer_workspace_bytes(ctypes.byref(d), 2, 5)
    assert enh_forward(None) == EINVAL and "null descriptor" in err()
    assert enh_forward(d, B=0) == 0 and enh_forward(d, Lt=0) == 0          # nothing to do
    assert enh_forward(d, B=-1) == EINVAL and "B=-1" in err()
    assert enh_forward(d, B=1 << 15, Lt=1 << 15) == EINVAL and "2^31" in err()
    for kw, word in ((dict(text=0), "null pointer"), (dict(out=0), "null pointer"), (dict(n_masks=0), "n_masks=0"),
                     (dict(text=PTR + 8), "misaligned text"), (dict(pos=PTR + 2), "misaligned text"), (dict(out=PTR + (1 << 16) + 4), "misaligned text"),
                     (dict(out=PTR), "out overlaps an input"), (dict(out=PTR + 16), "out overlaps an input"),
                     (dict(ws=0), "null workspace"), (dict(ws=PTR + (1 << 18) + 8), "misaligned workspace"),
                     (dict(ws_bytes=need - 1), "workspace too small"), (dict(ws=PTR + 256), "workspace overlaps an operand")):
        assert enh_forward(d, **kw) == EINVAL and word in err(), (kw, err())
    assert enh_forward(enh_desc(fc1_w=PTR + 2)) == EINVAL and "misaligned weight or bias" in err()
    assert enh_forward(d, pos=0, mask=0, ws_bytes=need - 1) == EINVAL          # optional operands may be NULL: the next refusal is the workspace's
    assert "workspace too small" in err()
    assert counters() == before


def test_encoder_refuses_bad_descriptors_operands_and_workspaces():
    L = _lib.lib()
    d, keep = encoder_desc()
    before = counters()
    need = L.vllm_gdino_encoder_workspace_bytes(ctypes.byref(d), A["B"], A["S"], A["Lt"])
    assert need > 0
    assert enc_forward(None) == EINVAL and "null descriptor" in err()
    for n in (0, 65):
        bad, _k = encoder_desc()
        bad.n_layers = n
        assert enc_forward(bad) == EINVAL and f"n_layers={n}" in err()
    bad, _k = encoder_desc()
    bad.enhancer = None
    assert enc_forward(bad) == EINVAL and "three arrays" in err()
    bad, _k = encoder_desc(dim_t=0)
    assert enc_forward(bad) == EINVAL and "missing dim_t" in err()
    bad, _k = encoder_desc(dim_t=PTR + 4)
    assert enc_forward(bad) == EINVAL and "misaligned" in err()
    # a layer descriptor its own entry refuses, in that entry's words
    for kw, word in ((dict(fusion=lambda: fusion_desc(E=128)), "fusion_layer: embed_dim=128"), (dict(enhancer=lambda: enh_desc(H=4)), "text_enhancer: n_heads=4"),
                     (dict(deformable=lambda: deform_desc(F=100)), "deform_enc_layer: d_ffn=100")):
        bad, _k = encoder_desc(**kw)
        assert enc_forward(bad) == EINVAL and word in err(), err()
    # layers of differing d_model (layer 1 of the enhancer at 128) or n_levels
    bad, k = encoder_desc()
    k[1][1] = enh_desc(C=128, H=2)
    assert enc_forward(bad) == EINVAL and "layer 1 has d_model=64 / 128 / 64" in err(), err()
    bad, k = encoder_desc()
    k[2][1] = deform_desc(Lv=3)
    assert enc_forward(bad) == EINVAL and "n_levels=3" in err(), err()
    assert enc_forward(d, B=0) == 0 and enc_forward(d, S=0) == 0 and enc_forward(d, Lt=0) == 0          # nothing to do
    assert enc_forward(d, B=-1) == EINVAL
    for key in ("vision", "vision_pos", "vr", "shapes", "lsi", "text", "out_vision", "out_text"):
        assert enc_forward(d, **{key: 0}) == EINVAL and "null pointer" in err(), key
    assert enc_forward(d, n_masks=0) == EINVAL and "n_masks=0" in err()
    for key, off in (("vision", 8), ("vision_pos", 2), ("text", 4), ("emb", PTR + 8), ("out_vision", 8), ("out_text", 2), ("vr", 4), ("shapes", 4),
                     ("lsi", 4), ("positions", 2)):
        assert enc_forward(d, **{key: A[key] + off}) == EINVAL and "misaligned" in err(), key
    for kw in (dict(out_vision=A["vision"]), dict(out_vision=A["vision_pos"] + 16), dict(out_text=A["text"]), dict(out_text=A["vision"] + 32),
               dict(out_vision=A["vr"]), dict(out_text=A["positions"]), dict(emb=A["out_text"])):
        assert enc_forward(d, **kw) == EINVAL and "an output overlaps an input" in err(), (kw, err())
    assert enc_forward(d, out_text=A["out_vision"] + 64) == EINVAL and "the two outputs overlap" in err()
    assert enc_forward(d, ws=0) == EINVAL and "null workspace" in err()
    assert enc_forward(d, ws=A["ws"] + 8) == EINVAL and "misaligned workspace" in err()
    assert enc_forward(d, ws_bytes=need - 1) == EINVAL and "workspace too small" in err()
    assert enc_forward(d, ws=A["text"] - 256) == EINVAL and "workspace overlaps an operand" in err()
    assert enc_forward(d, vmask=0, tmask=0, sam=0, positions=0, ws_bytes=need - 1) == EINVAL and "workspace too small" in err()   # optional operands
    assert counters() == before


def test_kernel_entries_refuse_what_they_cannot_run():
    L = _lib.lib()
    p = vp(PTR)
    before = counters()
    mha = lambda D=32, n_masks=1, q=PTR, ldq=64, Lk=5, B=2: L.vllm_mha_fwd_masks_bf16(vp(q), 5 * 64, ldq, p, 5 * 64, 64, p, 5 * 64, 64, p, 5 * 64, 64, p,
                                                                                        n_masks, None, B, 5, Lk, 2, D, 0.17, None)
    assert mha(D=48) == EINVAL and "head dim 48" in err()
    assert mha(n_masks=0) == EINVAL and "n_masks=0" in err()
    assert mha(n_masks=-3) == EINVAL and "n_masks=-3" in err()
    assert mha(q=0) == EINVAL and "null pointer" in err()
    assert mha(q=PTR + 8) == EINVAL and "misaligned operand" in err()
    assert mha(ldq=60) == EINVAL and "misaligned operand" in err()
    assert mha(Lk=0) == EINVAL and "at least one key" in err()
    assert mha(B=0) == 0
    tpe = lambda C=64, B=2, Lt=5, pos=PTR, dim_t=PTR, out=PTR, ld=64: L.vllm_text_pos_embed_bf16(vp(pos), vp(dim_t), B, Lt, C, vp(out), ld, None)
    for kw, word in ((dict(C=96), "C=96"), (dict(C=576), "C=576"), (dict(C=0), "C=0"), (dict(B=-1), "B=-1"), (dict(dim_t=0), "null pointer"),
                     (dict(out=0), "null pointer"), (dict(out=PTR + 8), "misaligned"), (dict(dim_t=PTR + 4), "misaligned"), (dict(pos=PTR + 2), "misaligned"),
                     (dict(ld=56), "ld_out=56"), (dict(ld=68), "ld_out=68")):
        assert tpe(**kw) == EINVAL and word in err(), (kw, err())
    assert tpe(B=0) == 0 and tpe(Lt=0) == 0
    ref = lambda L_=2, B=2, S=36, shapes=PTR, lsi=PTR, vr=PTR, out=PTR: L.vllm_encoder_refpoints_f32(vp(shapes), vp(lsi), vp(vr), B, S, L_, vp(out), None)
    for kw, word in ((dict(L_=0), "L=0"), (dict(L_=17), "L=17"), (dict(B=-1), "B=-1"), (dict(B=1 << 16, S=1 << 16), "2^31"), (dict(shapes=0), "null pointer"),
                     (dict(lsi=0), "null pointer"), (dict(vr=0), "null pointer"), (dict(out=0), "null pointer"), (dict(out=PTR + 8), "misaligned"),
                     (dict(vr=PTR + 4), "misaligned"), (dict(shapes=PTR + 4), "misaligned")):
        assert ref(**kw) == EINVAL and word in err(), (kw, err())
    assert ref(B=0) == 0 and ref(S=0) == 0
    assert counters() == before


# ---- the mirrors against the reference's run ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


def golden_layers(golden):
    C, FFN, HEADS, POINTS = (int(v) for v in golden["config"])
    cfg = types.SimpleNamespace(d_model=C, encoder_ffn_dim=FFN, encoder_attention_heads=HEADS, fusion_dropout=0.0, fusion_droppath=0.1,
                                text_enhancer_dropout=0.0, activation_function="relu", num_feature_levels=len(golden["spatial_shapes"]),
                                encoder_n_points=POINTS, dropout=0.1, activation_dropout=0.0, disable_custom_kernels=True, encoder_layers=2)
    m = G.GroundingDinoEncoder(cfg)
    sd = {k[len("sd."):]: torch.from_numpy(v) for k, v in golden.items() if k.startswith("sd.")}
    return m, sd


def rel(x, ref):
    return ((x - ref).abs().max() / ref.abs().max()).item()


def test_constructor_arguments_and_parameter_names_are_the_references(golden):
    m, sd = golden_layers(golden)
    assert set(m.state_dict()) == set(sd) and all(m.state_dict()[k].shape == v.shape for k, v in sd.items())
    assert m.load_state_dict(sd, strict=True)
    layer = m.layers[0]
    assert [n for n, _ in layer.named_children()] == ["text_enhancer_layer", "fusion_layer", "deformable_layer"]
    e = layer.text_enhancer_layer
    assert [n for n, _ in e.named_children()] == ["self_attn", "fc1", "fc2", "layer_norm_before", "layer_norm_after"]
    assert isinstance(e.self_attn, nn.MultiheadAttention) and e.self_attn.num_heads == 2 == e.num_heads and e.self_attn.batch_first
    assert e.fc1.out_features == 256 and e.activation is torch.nn.functional.relu and e.dropout == 0.0
    assert G.GroundingDinoTextEnhancerLayer.native_layer is False and G.GroundingDinoEncoder.native_encoder is False
    assert [f.name for f in G.dataclasses.fields(G.GroundingDinoEncoderOutput)] == [
        "last_hidden_state_vision", "last_hidden_state_text", "hidden_states_vision", "hidden_states_text", "attentions"]
    import visionllm_amd
    for n in ("GroundingDinoTextEnhancerLayer", "GroundingDinoEncoderLayer", "GroundingDinoEncoder", "GroundingDinoEncoderOutput", "get_sine_pos_embed"):
        assert getattr(visionllm_amd, n) is getattr(G, n) and n in visionllm_amd.__all__


def test_mirrors_in_fp64_reproduce_the_references_run(golden):
    m, sd = golden_layers(golden)
    m.load_state_dict(sd)
    m = m.double().eval()
    t = {k: torch.from_numpy(v) for k, v in golden.items() if not k.startswith("sd.") and k != "config"}
    f64 = lambda k: t[k].double()
    ref = G.GroundingDinoEncoder.get_reference_points(t["spatial_shapes"], f64("valid_ratios"), "cpu")
    assert ref.shape == t["reference_points"].shape and rel(ref, t["reference_points"]) <= 1e-10
    kw = dict(vision_position_embedding=f64("vision_pos"), spatial_shapes=t["spatial_shapes"], level_start_index=t["level_start_index"],
              key_padding_mask=t["vision_attention_mask"], reference_points=ref, text_attention_mask=t["text_attention_mask"],
              text_position_embedding=None, text_self_attention_masks=t["text_self_attention_masks"], text_position_ids=t["text_position_ids"])
    with torch.no_grad(), cpu_operator():
        (v1, t1), attn = m.layers[0](vision_features=f64("vision"), text_features=f64("text"), **kw)
        (v2, t2), _ = m.layers[1](vision_features=v1, text_features=t1, **kw)
        out = m(f64("vision"), t["vision_attention_mask"], f64("vision_pos"), t["spatial_shapes"], t["level_start_index"], f64("valid_ratios"),
                f64("text"), t["text_attention_mask"], None, t["text_self_attention_masks"], t["text_position_ids"], return_dict=True)
        tup = m(f64("vision"), t["vision_attention_mask"], f64("vision_pos"), t["spatial_shapes"], t["level_start_index"], f64("valid_ratios"),
                f64("text"), t["text_attention_mask"], None, t["text_self_attention_masks"], t["text_position_ids"], output_hidden_states=True,
                output_attentions=True, return_dict=False)
    figures = dict(v1=rel(v1, t["out_vision_1"]), t1=rel(t1, t["out_text_1"]), v2=rel(v2, t["out_vision_2"]), t2=rel(t2, t["out_text_2"]),
                   enc_v=rel(out.last_hidden_state_vision, t["out_vision_2"]), enc_t=rel(out.last_hidden_state_text, t["out_text_2"]))
    print(figures)
    assert max(figures.values()) <= 1e-10
    assert len(attn) == 4 and attn[2].shape == (2, 2, 5, 5) and all(a is not None for a in attn)
    assert isinstance(out, G.GroundingDinoEncoderOutput) and out.hidden_states_vision is None and out.attentions is None
    assert len(tup) == 5 and len(tup[2]) == 3 and len(tup[3]) == 3 and len(tup[4]) == 4 and len(tup[4][2]) == 2
    assert torch.equal(tup[0], out.last_hidden_state_vision) and torch.equal(tup[2][1], v1) and torch.equal(tup[3][1], t1)
    # the enhancer alone: layer 1's input text is layer 0's fused text, which only the layer sees -- so the enhancer is pinned through the
    # layer outputs above, and its position embedding here: ids that restart per phrase give the same rows as get_sine_pos_embed says
    pe = m.layers[0].get_text_position_embeddings(f64("text"), None, t["text_position_ids"])
    assert pe.dtype == torch.float32 and pe.shape == (2, 5, 64)
    assert torch.equal(pe[0, 0], pe[0, 2]) and torch.equal(pe[1, 0], pe[1, 3]) and not torch.equal(pe[0, 1], pe[0, 2])
    d = G.sine_dim_t(64, "cpu")
    want = torch.where(torch.arange(64) % 2 == 0, torch.sin(t["text_position_ids"][..., None] * (2 * torch.pi) / d),
                       torch.cos(t["text_position_ids"][..., None] * (2 * torch.pi) / d))
    assert torch.allclose(pe, want.float(), atol=1e-6)


# ---- reasons ------------------------------------------------------------------------------------------------------------------------------------
class FakeCuda(torch.Tensor):
    """a CPU tensor that says it is on the GPU: the reasons are decided from dtypes, shapes and flags alone"""
    @property
    def is_cuda(self):
        return True


def fake_inputs(t):
    return {k: v.as_subclass(FakeCuda) if torch.is_tensor(v) else v for k, v in t.items()}


def fake_module(m, dtype=torch.bfloat16):
    """a frozen copy of ``m`` in ``dtype`` whose parameters say they are on the GPU"""
    m = I.copy.deepcopy(m).to(dtype).eval()
    for mod in m.modules():
        for k, p in list(mod._parameters.items()):
            if p is not None:
                mod._parameters[k] = nn.Parameter(p.data, requires_grad=False).as_subclass(FakeCuda)
    return m


def enc_reasons(m, t, **kw):
    a = dict(vision_features=t["vision"], vision_attention_mask=t["vision_mask"], vision_position_embedding=t["vision_pos"],
             spatial_shapes=t["spatial_shapes"], level_start_index=t["level_start_index"], valid_ratios=t["valid_ratios"], text_features=t["text"],
             text_attention_mask=t["text_mask"], text_position_embedding=None, text_self_attention_masks=t["text_self_attention_masks"],
             text_position_ids=t["text_position_ids"])
    a.update(kw)
    return m.native_encoder_reasons(**a)


@pytest.mark.parametrize("name", list(I.CONFIGS))
def test_both_configurations_are_served_apart_from_the_device(name):
    """bf16 module and inputs that say they are on the GPU: no member and no level has anything to object to; on the CPU as it is, every
    reason is about the device."""
    m = fake_module(I.make_encoder(name, 2))
    t = fake_inputs(I.to(I.make_inputs(name, 5), "cpu"))
    layer = m.layers[1]
    e = layer.text_enhancer_layer
    assert e.self_attn.head_dim == (32 if name == "a" else 64) and layer.fusion_layer.attn.head_dim == (128 if name == "a" else 256)
    with torch.no_grad():
        assert layer.fusion_layer.native_layer_reasons(t["vision"], t["text"], t["vision_mask"], t["text_mask"]) == []
        for mask in (~t["text_self_attention_masks"], (~t["text_self_attention_masks"])[0], I.enhancer_mask(t, "BH", 2), None):
            for pos in (t["text_pos"], None):
                assert e.native_layer_reasons(t["text"], mask, pos) == [] and e.native_layer_applies(t["text"], mask, pos)
        assert layer.deformable_layer.native_layer_reasons(t["vision"], t["vision_pos"], t["valid_ratios"]) == []
        assert enc_reasons(m, t) == [] and enc_reasons(m, t, text_position_ids=None) == []
        assert enc_reasons(m, t, text_position_ids=None, text_position_embedding=t["text_pos"]) == []
        assert enc_reasons(m, t, vision_attention_mask=None, text_attention_mask=None, valid_ratios=t["valid_ratios"].to(torch.bfloat16)) == []
        real = I.as_bf16(I.make_encoder(name, 1), "cpu")
        cpu = I.to(I.make_inputs(name, 5), "cpu")
        why = real.layers[0].text_enhancer_layer.native_layer_reasons(cpu["text"], ~cpu["text_self_attention_masks"], cpu["text_pos"])
        assert why and all("GPU" in r or "CUDA" in r for r in why), why
        assert enc_reasons(real, cpu) == ["vision_features / text_features: bf16 CUDA tensors [B, ., d_model] of one batch"]


def test_every_reason_of_the_enhancer_to_keep_the_composed_path():
    t = fake_inputs(I.to(I.make_inputs("a", 5), "cpu"))
    x, pos, mask = t["text"], t["text_pos"], ~t["text_self_attention_masks"]

    def why(m=None, x=x, mask=mask, pos=pos, **kw):
        m = m or fake_module(I.make_enhancer("a", **kw))
        r = m.native_layer_reasons(x, mask, pos)
        assert m.native_layer_applies(x, mask, pos) == (not r)
        return r
    with torch.no_grad():
        assert why() == []
        m = fake_module(I.make_enhancer("a"))
        m.train()
        assert why(m) == ["training mode"]
        assert why(fake_module(I.make_enhancer("a"), torch.float32)) == ["parameters: bf16 on the GPU"]
        assert why(I.as_bf16(I.make_enhancer("a"), "cpu")) == ["parameters: bf16 on the GPU"]          # real CPU parameters
        assert why(x=x.float()) == ["hidden_states: a bf16 CUDA tensor [B, Lt, d_model]"]
        assert why(x=I.to(I.make_inputs("a", 5), "cpu")["text"])[0] == "hidden_states: a bf16 CUDA tensor [B, Lt, d_model]"
        assert why(pos=pos.float()) == ["position_embeddings: None or a bf16 CUDA tensor of hidden_states' shape"]
        assert why(pos=pos[:, :4]) == ["position_embeddings: None or a bf16 CUDA tensor of hidden_states' shape"]
        wide = torch.zeros(3, 5, 128, dtype=torch.bfloat16).as_subclass(FakeCuda)
        assert why(x=wide[:, :, ::2]) == ["hidden_states / position_embeddings: a contiguous last dim"]
        assert why(x=wide) == ["position_embeddings: None or a bf16 CUDA tensor of hidden_states' shape",
                               "shapes: [B, Lt, d_model], B Lt rows of the widest intermediate under 2^31 bytes"]
        assert why(mask=mask.float()) == ["attention_masks: None or bool [Lt, Lt], [B, Lt, Lt] or [B H, Lt, Lt] (a float mask keeps the composed path)"]
        assert why(mask=mask[:2])[0].startswith("attention_masks:") and why(mask=mask[:, :4])[0].startswith("attention_masks:")
        assert why(encoder_attention_heads=8) == ["self_attn: head dim 16 (32 or 64)"]          # 4 heads of 16
        assert why(activation_function="silu") == ["activation: relu or gelu"]
        assert why(activation_function="gelu") == []
        assert why(encoder_ffn_dim=200) == ["d_model a multiple of 64 in 64 .. 512, d_ffn a multiple of 64"]
        m = fake_module(I.make_enhancer("a"))
        m.self_attn.add_zero_attn = True
        assert why(m) == ["self_attn: bias_k / add_zero_attn"]
        m = fake_module(I.make_enhancer("a"))
        m.self_attn.bias_k = nn.Parameter(torch.zeros(1, 1, 64, dtype=torch.bfloat16), requires_grad=False).as_subclass(FakeCuda)
        assert why(m) == ["self_attn: bias_k / add_zero_attn"]
        m = fake_module(I.make_enhancer("a"))
        m.self_attn.in_proj_weight = None
        assert why(m) == ["self_attn: separate q / k / v projection weights"]
    m = fake_module(I.make_enhancer("a"))
    for p in m.parameters():
        p.requires_grad_(True)
    assert why(m) == ["requires_grad under grad mode: there is no native backward"]
    with torch.no_grad():
        assert why(m) == []


def test_every_reason_of_the_encoder_to_keep_the_composed_path():
    m = fake_module(I.make_encoder("a", 2))
    t = fake_inputs(I.to(I.make_inputs("a", 5), "cpu"))
    with torch.no_grad():
        assert enc_reasons(m, t, output_attentions=True) == ["output_attentions: the attention weights stay inside the native call"]
        assert enc_reasons(m, t, output_hidden_states=True) == ["output_hidden_states: the hidden states between two layers stay inside the native call"]
        why = enc_reasons(m, t, text_self_attention_masks=None)
        assert why == ["text_self_attention_masks: missing"]
        for vr in (None, t["valid_ratios"][:, :1], t["valid_ratios"].double(), t["valid_ratios"][:2]):
            assert enc_reasons(m, t, valid_ratios=vr) == ["valid_ratios: an fp32 or bf16 CUDA tensor [B, n_levels, 2]"]
        assert enc_reasons(m, t, text_position_ids=t["text_position_ids"][:, :3]) == ["text_position_ids: None or a CUDA tensor [B, Lt]"]
        assert enc_reasons(m, t, text_position_ids=None, text_position_embedding=t["text_pos"].float()) == [
            "text_position_embedding: None or a bf16 CUDA tensor of text_features' shape"]
        assert enc_reasons(m, t, vision_position_embedding=None) == ["vision_position_embedding: a bf16 CUDA tensor of vision_features' shape"]
        # a member's reasons carry the member's name
        assert enc_reasons(m, t, text_self_attention_masks=t["text_self_attention_masks"].float()) == [
            f"layers.{i}.text_enhancer_layer: attention_masks: None or bool [Lt, Lt], [B, Lt, Lt] or [B H, Lt, Lt] (a float mask keeps the composed path)"
            for i in range(2)]
        assert enc_reasons(m, t, vision_attention_mask=t["vision_mask"].float()) == [
            f"layers.{i}.fusion_layer: attention_mask_vision: bool [B, S] or None" for i in range(2)]
        m.layers[1].deformable_layer.fc1 = nn.Linear(64, 100, dtype=torch.bfloat16)
        why = enc_reasons(m, t)
        assert why and all(r.startswith("layers.1.deformable_layer: ") for r in why), why
        d16 = fake_module(I.make_encoder("a", 1, encoder_attention_heads=8))
        why = enc_reasons(d16, t)
        assert "layers.0.text_enhancer_layer: self_attn: head dim 16 (32 or 64)" in why
        m = fake_module(I.make_encoder("a", 1))
        m.train()
        assert "training mode" in enc_reasons(m, t) and "layers.0.text_enhancer_layer: training mode" in enc_reasons(m, t)


def test_the_switches_change_nothing_on_the_cpu(monkeypatch):
    """On, CPU tensors keep the composed path (the deformable operator through its CPU twin): the bits of the run with the switches off,
    the composed types, no call into the library."""
    m = I.make_encoder("a", 2)
    t = I.to(I.make_inputs("a", 5), "cpu", torch.float32)
    before = counters()
    with torch.no_grad(), cpu_operator():
        off = I.encoder_call(m, t, return_dict=False)
        monkeypatch.setattr(G.GroundingDinoEncoder, "native_encoder", True)
        monkeypatch.setattr(G.GroundingDinoTextEnhancerLayer, "native_layer", True)
        on = I.encoder_call(m, t, return_dict=False)
        e = m.layers[0].text_enhancer_layer
        h, w = e(t["text"], ~t["text_self_attention_masks"], t["text_pos"])
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and counters() == before
    assert w is not None and w.shape == (3, 2, 5, 5) and h.shape == t["text"].shape


# ---- the quirk ----------------------------------------------------------------------------------------------------------------------------------
def test_a_batched_mask_reaches_head_h_of_image_b_as_the_mask_of_image_b_H_plus_h_mod_B():
    """Config a: B 3, H 2, three different masks.  The composed enhancer equals a hand-written per-(image, head) attention under mask
    (b H + h) % B -- and differs from the one under mask b, which is what a reader of the reference would expect."""
    m = I.make_enhancer("a").double()
    t = I.to(I.make_inputs("a", 5), "cpu", torch.float64)
    masks = ~t["text_self_attention_masks"]
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[0], masks[2])
    x, pos = t["text"], t["text_pos"]
    B, Lt, C = x.shape
    H = m.num_heads
    assert (B, H) == (3, 2)
    with torch.no_grad():
        got, weights = m(x, masks, pos)
        W, bias = m.self_attn.in_proj_weight, m.self_attn.in_proj_bias
        q = (x + pos) @ W[:C].T + bias[:C]
        k = (x + pos) @ W[C:2 * C].T + bias[C:2 * C]
        v = x @ W[2 * C:].T + bias[2 * C:]

        def tail(ctx):
            y = m.layer_norm_before(x + m.self_attn.out_proj(ctx))
            return m.layer_norm_after(y + m.fc2(m.activation(m.fc1(y))))
        quirk, by_image = tail(I.quirk_attention(q, k, v, masks, H, False)), tail(I.quirk_attention(q, k, v, masks, H, True))
    assert rel(got, quirk) <= 1e-12
    assert rel(got, by_image) > 1e-3
    # the weights say it directly: head h of image b is zero exactly where mask (b H + h) % B forbids
    for b in range(B):
        for h in range(H):
            assert torch.equal(weights[b, h] == 0, masks[(b * H + h) % B])
    # and the three mask shapes the native route takes mean what the module makes of them
    with torch.no_grad():
        same, _ = m(x, masks.repeat(H, 1, 1), pos)          # [B H, Lt, Lt]: used as it is
    assert torch.equal(same, got)
    assert G._n_masks(masks, B, H, Lt) == B and G._n_masks(masks[0], B, H, Lt) == 1 and G._n_masks(masks.repeat(H, 1, 1), B, H, Lt) == B * H
    assert G._n_masks(masks[:2], B, H, Lt) is None


# ---- the conditions of the GPU tests' inputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_layers,Lt", [("a", 1, 5), ("a", 3, 5), ("b", 2, 5), ("a", 1, 70), ("b", 1, 70), ("a", 1, 1), ("b", 1, 1)])
def test_inputs_keep_a_key_in_every_row_pad_some_vision_rows_and_take_both_relu_branches(name, n_layers, Lt):
    t = I.make_inputs(name, Lt)
    allowed = t["text_self_attention_masks"]
    B = allowed.shape[0]
    assert allowed.any(-1).all(), "an enhancer row without a key"
    assert (~t["text_mask"]).any(-1).all() and (~t["vision_mask"]).any(-1).all(), "an image without a text token or a pixel"
    if Lt >= 5:
        assert len({tuple(I.phrases(b, Lt)) for b in range(B)}) == B          # the phrases differ per image
        assert not torch.equal(allowed[0], allowed[1])
    padded = t["vision_mask"].float().mean().item()
    vr = t["valid_ratios"]
    assert 0.10 <= padded <= 0.30 and (vr > 0.5).all() and (vr <= 1).all() and (vr == 1).any()
    v, x, rec = I.reference_encoder(name, n_layers, Lt)
    assert torch.isfinite(v).all() and torch.isfinite(x).all() and len(rec) == 2 * n_layers
    for key, pre in rec.items():
        neg = (pre < 0).float().mean().item()
        print(f"{name} x{n_layers} Lt {Lt} {key}: negative pre-activation {neg:.3f}; padded vision rows {padded:.3f}")
        assert 0.30 <= neg <= 0.70, (key, neg)


@pytest.mark.parametrize("name", list(I.CONFIGS))
def test_enhancer_inputs_take_both_relu_branches(name):
    for Lt in I.LTS:
        for kind in ("B", "2d", "BH"):
            t = I.make_inputs(name, Lt)
            mask = I.enhancer_mask(t, kind, 2)
            assert (~mask).any(-1).all(), "a row without a key"
            out, w, pre = I.reference_enhancer(name, Lt, kind, True)
            neg = (pre < 0).float().mean().item()
            assert torch.isfinite(out).all() and 0.30 <= neg <= 0.70, (name, Lt, kind, neg)
    # the scores of the enhancer-alone inputs: a softmax that is neither flat nor one-hot
    m = I.make_enhancer(name).double()
    t = I.to(I.make_inputs(name, 70), "cpu", torch.float64)
    C, H = m.self_attn.embed_dim, m.num_heads
    x = t["enh_text"] + t["enh_pos"]
    W, b = m.self_attn.in_proj_weight.detach(), m.self_attn.in_proj_bias.detach()
    q, k = (x @ W[:C].T + b[:C]).reshape(-1, 70, H, C // H), (x @ W[C:2 * C].T + b[C:2 * C]).reshape(-1, 70, H, C // H)
    std = (torch.einsum("bqhd,bkhd->bhqk", q, k) / (C // H) ** 0.5).std().item()
    print(f"{name}: enhancer_scale {I.enhancer_scale(name):.3f}, score std {std:.2f}")
    assert 1.5 <= std <= 2.5
