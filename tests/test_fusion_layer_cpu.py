"""CPU: the boundary of the native fusion layer (include/vllm_hip.h, section f2f) -- symbols, descriptor layout, the size query, the
refusals of the layer entry and of vllm_xattn_fwd_bf16 (refused calls only, fake device pointers: nothing is dereferenced, no device is
touched), the plan of the key split, and the module mirror where no GPU is needed: constructor arguments and parameter names, the state
dict and both outputs of the reference's own fp64 run (tests/golden/fusion_layer.npz, tools/gen_golden_fusion.py), every reason
``native_layer_reasons`` has to say no, and the conditions the GPU tests' inputs are meant to meet."""
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
from visionllm_amd import fusion_layer as FL

import fusion_layer_inputs as I

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
GIB = 1 << 30
NEW = ("vllm_fusion_layer_desc_sizeof", "vllm_fusion_layer_workspace_bytes", "vllm_fusion_layer_calls", "vllm_fusion_layer_forward",
       "vllm_xattn_fwd_bf16", "vllm_xattn_workspace_bytes", "vllm_xattn_plan")
POINTERS = ("vision_norm_w", "vision_norm_b", "text_norm_w", "text_norm_b", "vision_proj_w", "vision_proj_b", "text_proj_w", "text_proj_b",
            "values_vision_proj_w", "values_vision_proj_b", "values_text_proj_w", "values_text_proj_b", "out_vision_proj_w",
            "out_vision_proj_b", "out_text_proj_w", "out_text_proj_b", "vision_param", "text_param")
# the reference's parameter names (GroundingDinoFusionLayer of modeling_ov_grounding_dino_mask_dn.py:1044-1057, :882-888), in registration order
PARAMETER_NAMES = ["vision_param", "text_param", "layer_norm_vision.weight", "layer_norm_vision.bias", "layer_norm_text.weight",
                   "layer_norm_text.bias"] + [f"attn.{n}.{p}" for n in ("vision_proj", "text_proj", "values_vision_proj", "values_text_proj",
                                                                       "out_vision_proj", "out_text_proj") for p in ("weight", "bias")]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_layer.npz")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def last_error():
    return _lib.lib().vllm_last_error().decode()


def calls():
    return _lib.lib().vllm_fusion_layer_calls()


def desc(C=256, E=1024, H=4, eps=1e-5, **own):
    d = _lib.VllmFusionLayerDesc()
    d.d_model, d.embed_dim, d.n_heads, d.vision_norm_eps, d.text_norm_eps = C, E, H, eps, eps
    for n in POINTERS:
        setattr(d, n, own.pop(n, PTR))
    assert not own, own
    return d


def query(d, B=2, S=300, Lt=9):
    return _lib.lib().vllm_fusion_layer_workspace_bytes(ctypes.byref(d), B, S, Lt)


def forward(d, B=2, S=300, Lt=9, vision=PTR + GIB, text=PTR + 2 * GIB, vmask=PTR + 3 * GIB, tmask=PTR + 4 * GIB, out_v=PTR + 5 * GIB,
            out_t=PTR + 6 * GIB, ws=PTR + 8 * GIB, ws_bytes=1 << 40):
    return _lib.lib().vllm_fusion_layer_forward(ctypes.byref(d), vp(vision), vp(text), vp(vmask), vp(tmask), B, S, Lt, vp(out_v), vp(out_t),
                                                vp(ws), ws_bytes, None)


def xattn(B=2, Lq=70, Lk=600, H=2, D=128, q=PTR, k=PTR + GIB, v=PTR + 2 * GIB, out=PTR + 3 * GIB, ld=None, bs=None, kpm=0, ws=PTR + 4 * GIB,
          ws_bytes=1 << 40, **kw):
    ld = H * D if ld is None else ld
    g = lambda n, dflt: kw.get(n, dflt)
    qbs, kbs = (Lq * ld if bs is None else bs), (Lk * ld if bs is None else bs)
    return _lib.lib().vllm_xattn_fwd_bf16(vp(q), g("q_bs", qbs), g("ldq", ld), vp(k), g("k_bs", kbs), g("ldk", ld), vp(v), g("v_bs", kbs), g("ldv", ld),
                                          vp(out), g("o_bs", qbs), g("ldo", ld), vp(kpm), B, Lq, Lk, H, D, D ** -0.5, vp(ws), ws_bytes, None)


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
    assert "f2f. The FUSION LAYER" in hdr and "mask_dn.py:860-1101" in hdr and "STATED DEPARTURES" in hdr
    for n in ("vllm_fusion_layer_forward", "vllm_xattn_fwd_bf16"):
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + n + r"\s*\(", hdr, flags=re.S), f"no 'Alignment' line directly above {n}"


def test_descriptor_mirror_has_the_library_size_and_the_header_order():
    """The descriptor is a tagged struct (``struct VllmFusionLayerDesc``, no typedef name): the binding reads it from the header under
    parse_structs' member rules, and the library's own sizeof is compared when it is loaded."""
    L = _lib.lib()
    assert list(_lib.TAGGED_STRUCTS) == ["VllmFusionLayerDesc"] and _lib.TAGGED_STRUCTS["VllmFusionLayerDesc"] is _lib.VllmFusionLayerDesc
    assert "VllmFusionLayerDesc" not in _lib.STRUCTS and list(_lib.parse_tagged_structs()) == ["VllmFusionLayerDesc"]
    assert ctypes.sizeof(_lib.VllmFusionLayerDesc) == L.vllm_fusion_layer_desc_sizeof()
    _lib.check_struct_layouts()
    protos = _lib.parse_header()
    with pytest.raises(RuntimeError, match="vllm_fusion_layer_desc_sizeof"):          # the load insists on the export
        _lib._check_struct_layouts(L, {k: v for k, v in protos.items() if k != "vllm_fusion_layer_desc_sizeof"})
    assert _lib.pointer_fields(_lib.VllmFusionLayerDesc) == POINTERS
    assert [n for n, _ in _lib.VllmFusionLayerDesc._fields_] == ["d_model", "embed_dim", "n_heads", "vision_norm_eps", "text_norm_eps", *POINTERS]
    hdr = open(_lib.HEADER).read()
    at = hdr.index("\nstruct VllmFusionLayerDesc {")
    body = hdr[at:hdr.index("};", at)]
    order = [re.search(r"\b" + n + r"\b", body).start() for n, _ in _lib.VllmFusionLayerDesc._fields_]
    assert order == sorted(order), "VllmFusionLayerDesc: field order differs from include/vllm_hip.h"
    assert calls() >= 0


def test_descriptor_has_the_c_compilers_layout(tmp_path):
    """sizeof and every offsetof as the host C compiler lays out include/vllm_hip.h (read as C: ``struct VllmFusionLayerDesc``)"""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if not cc:
        pytest.skip("no host C compiler")
    cls = _lib.VllmFusionLayerDesc
    lines = ['printf("size %zu\\n", sizeof(struct VllmFusionLayerDesc));']
    want = {"size": ctypes.sizeof(cls)}
    for member, _ in cls._fields_:
        lines.append(f'printf("{member} %zu\\n", offsetof(struct VllmFusionLayerDesc, {member}));')
        want[member] = getattr(cls, member).offset
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vllm_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(tmp_path / "layout")], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout
    assert {k: int(v) for k, v in (ln.split() for ln in out.splitlines())} == want and len(want) == 24


@pytest.mark.parametrize("member", ["unsigned long n", "struct Other *p", "int a : 3", "int n[]"])
def test_a_tagged_member_the_parser_cannot_read_is_an_error_not_a_gap(tmp_path, member):
    hdr = tmp_path / "h.h"
    hdr.write_text("typedef struct Good { int a, *b, c[2]; } Good;\nstruct Fine { Good g; const Good *p; float x; };\nstruct Bad {\n    int before;\n    "
                   + member + ";\n};\n")
    with pytest.raises(ValueError) as e:
        _lib.parse_tagged_structs(str(hdr))
    assert "struct Bad" in str(e.value) and member in str(e.value)
    hdr.write_text("typedef struct Good { int a, *b, c[2]; } Good;\nstruct Fine { Good g; const Good *p; float x; };\n")
    fine = _lib.parse_tagged_structs(str(hdr))["Fine"]
    assert [n for n, _ in fine._fields_] == ["g", "p", "x"] and list(_lib.parse_structs(str(hdr))) == ["Good"]


def test_workspace_query_is_positive_and_monotone_and_refuses():
    L = _lib.lib()
    d = desc()
    base = query(d)
    assert base > 0
    assert query(d, B=3) > base and query(d, S=301) > base and query(d, Lt=10) > base
    a256 = lambda x: (x + 255) & ~255
    B, S, Lt, C, E = 2, 300, 9, 256, 1024
    # the normalised inputs, vision_proj / values_vision_proj, text_proj / values_text_proj / the text side's attention output; one split
    assert I.plan(B, Lt, S, 4, 256)[0] == 1 and I.plan(B, S, Lt, 4, 256)[0] == 1
    assert base == a256(B * S * C * 2) + a256(B * Lt * C * 2) + 2 * a256(B * S * E * 2) + 3 * a256(B * Lt * E * 2)
    S3 = I.lk3(B, Lt, 4, 256)
    assert query(d, S=S3) == a256(B * S3 * C * 2) + a256(B * Lt * C * 2) + 2 * a256(B * S3 * E * 2) + 3 * a256(B * Lt * E * 2) + \
        a256(L.vllm_xattn_workspace_bytes(B, Lt, S3, 4, 256))
    assert query(d, B=0) == 0 and query(d, S=0) == 0
    for kw, word in ((dict(B=-1), "B=-1"), (dict(S=-1), "S=-1"), (dict(Lt=0), "Lt=0"), (dict(B=1 << 10, S=1 << 12), "2^31")):
        assert query(d, **kw) < 0 and word in last_error(), (kw, last_error())
    assert L.vllm_fusion_layer_workspace_bytes(None, 2, 300, 9) < 0 and "null descriptor" in last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(C=0), "d_model"), (dict(C=32), "d_model"), (dict(C=96), "d_model"), (dict(C=576), "d_model"),
    (dict(E=1024, H=16), "head dim"), (dict(E=1024, H=2), "head dim"), (dict(E=1000, H=3), "head dim"), (dict(H=0), "head dim"),
    (dict(eps=-1.0), "negative eps"),
] + [({name: 0}, "missing weights") for name in POINTERS], ids=lambda v: None if isinstance(v, dict) else v.replace(" ", "_"))
def test_refused_descriptors_have_their_own_messages(kw, word):
    d = desc(**kw)
    before = calls()
    assert query(d) < 0
    assert word in last_error(), last_error()
    assert forward(d) == EINVAL
    assert word in last_error() and "workspace" not in last_error(), last_error()
    assert calls() == before


def test_null_misaligned_and_overlapping_operands_have_their_own_messages():
    d = desc()
    before = calls()
    B, S, Lt, C = 2, 300, 9, 256
    for n in ("vision", "text", "out_v", "out_t"):
        assert forward(d, **{n: 0}) == EINVAL and "null pointer" in last_error() and "workspace" not in last_error(), (n, last_error())
    base = dict(vision=PTR + GIB, text=PTR + 2 * GIB, out_v=PTR + 5 * GIB, out_t=PTR + 6 * GIB)
    for n in base:
        assert forward(d, **{n: base[n] + 8}) == EINVAL and "fusion_layer: misaligned vision" in last_error(), (n, last_error())
    assert forward(d, vmask=0, tmask=0, ws_bytes=0) == EINVAL and "workspace" in last_error()          # both masks are optional
    assert forward(d, vmask=PTR + 3 * GIB + 1, ws_bytes=0) == EINVAL and "workspace" in last_error()   # element alignment
    for name in POINTERS:
        assert forward(desc(**{name: PTR + 8})) == EINVAL and "misaligned weight, bias or parameter" in last_error(), name
    for kw in (dict(out_v=base["vision"]), dict(out_v=base["vision"] + B * S * C * 2 - 16), dict(out_v=base["text"]), dict(out_t=base["text"] + 16),
               dict(out_t=base["vision"] + 32), dict(out_t=base["out_v"] + 64)):
        assert forward(d, **kw) == EINVAL and "overlap an input or each other" in last_error(), (kw, last_error())
    assert forward(d, out_t=base["out_v"] + B * S * C * 2, ws_bytes=0) == EINVAL and "workspace" in last_error()   # back to back is no overlap
    assert forward(d, out_v=PTR + 8 * GIB + 4096) == EINVAL and "workspace overlaps an operand" in last_error()
    for kw, word in ((dict(Lt=0), "Lt=0"), (dict(B=-1), "B=-1"), (dict(B=1 << 10, S=1 << 12), "2^31")):
        assert forward(d, **kw) == EINVAL and word in last_error(), (kw, last_error())
    need = query(d)
    assert forward(d, ws=0, ws_bytes=need) == EINVAL and "null workspace" in last_error()
    assert forward(d, ws=PTR + 8 * GIB + 8, ws_bytes=need) == EINVAL and "misaligned workspace" in last_error()
    assert forward(d, ws_bytes=need - 1) == EINVAL and "workspace too small" in last_error()
    # B S == 0: nothing to do, whatever the pointers are
    assert forward(d, B=0, vision=0, out_v=0, ws=0, ws_bytes=0) == 0 and forward(d, S=0, vision=0, text=0, ws=0, ws_bytes=0) == 0
    assert calls() == before          # no refused call reached a launch


def test_the_attention_kernels_refusals_have_their_own_messages():
    L = _lib.lib()
    for D in (32, 64, 96, 512):
        assert xattn(D=D, H=1) == EINVAL and f"head dim {D}" in last_error()
    for kw in (dict(B=-1), dict(Lq=-1), dict(H=0)):
        assert xattn(**kw) == EINVAL and "xattn_fwd: B=" in last_error(), kw
    assert xattn(Lk=0) == EINVAL and "at least one key" in last_error()
    for n in ("q", "k", "v", "out"):
        assert xattn(**{n: 0}) == EINVAL and "null pointer" in last_error() and "workspace" not in last_error(), n
        assert xattn(**{n: PTR + 8}) == EINVAL and "misaligned operand" in last_error(), n
    for n in ("ldq", "ldk", "ldv", "ldo"):
        assert xattn(**{n: 256 + 4}) == EINVAL and "misaligned operand" in last_error(), n
        assert xattn(**{n: 256 - 8}) == EINVAL and "row stride below H D = 256" in last_error(), n
    for n in ("q_bs", "k_bs", "v_bs", "o_bs"):
        assert xattn(**{n: 70 * 256 + 4}) == EINVAL and "misaligned operand" in last_error(), n
    need = L.vllm_xattn_workspace_bytes(2, 70, 600, 2, 128)
    assert need == 2 * 2 * 70 * I.plan(2, 70, 600, 2, 128)[0] * (128 + 2) * 4 > 0
    assert xattn(ws=0, ws_bytes=need) == EINVAL and "null workspace" in last_error()
    assert xattn(ws=PTR + 4 * GIB + 8, ws_bytes=need) == EINVAL and "misaligned workspace" in last_error()
    assert xattn(ws_bytes=need - 1) == EINVAL and "workspace too small" in last_error()
    # one split: no workspace is asked for; no rows: nothing to do
    assert L.vllm_xattn_workspace_bytes(2, 300, 7, 2, 128) == 0
    assert xattn(B=0, q=0, out=0, ws=0, ws_bytes=0) == 0 and xattn(Lq=0, q=0, ws=0, ws_bytes=0) == 0
    assert L.vllm_xattn_workspace_bytes(2, 70, 300, 2, 64) < 0 and "D 128 or 256" in last_error()
    s, k = ctypes.c_int(), ctypes.c_int()
    assert L.vllm_xattn_plan(2, 70, 300, 2, 64, ctypes.byref(s), ctypes.byref(k)) == EINVAL and "head dim 64" in last_error()
    assert L.vllm_xattn_plan(2, 70, 300, 2, 128, None, ctypes.byref(k)) == EINVAL and "null pointer" in last_error()


def test_the_plan():
    for D, Lq, Lk, H, B, long_keys in I.xattn_cases():
        s, kps = I.plan(B, Lq, Lk, H, D)
        assert (s, kps) == I.plan(B, Lq, Lk, H, D), "the plan is a function of its arguments"
        assert kps % I.KEY_TILE == 0 and kps > 0 and (s - 1) * kps < Lk <= s * kps
        if long_keys:
            assert s == 3 and Lk - 2 * kps == 1, (D, Lq, Lk, H, B, s, kps)          # >= 3 splits, a ragged last split of one key
            assert I.plan(B, Lq, Lk - 1, H, D)[0] < 3 or (Lk - 1) - 2 * I.plan(B, Lq, Lk - 1, H, D)[1] != 1
        else:
            assert s == 1, (D, Lq, Lk, H, B, s)
        need = _lib.lib().vllm_xattn_workspace_bytes(B, Lq, Lk, H, D)
        assert need == (B * H * Lq * s * (D + 2) * 4 if s > 1 else 0)
    # the workload: image -> text is one split, text -> image fills two workgroups per CU of 256 CUs exactly
    assert I.plan(8, 37485, 256, 4, 256) == (1, 256)
    s, kps = I.plan(8, 256, 37485, 4, 256)
    assert s == 4 and kps % I.KEY_TILE == 0 and 3 * kps < 37485 <= 4 * kps
    for name in I.LAYER_SHAPES:
        sh = I.shape_of(name)
        assert I.plan(sh.B, sh.S, sh.Lt, sh.H, sh.D)[0] == 1
        assert I.plan(sh.B, sh.Lt, sh.S, sh.H, sh.D)[0] == (3 if name == "split" else 1)


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------------------------
def test_constructors_take_the_references_arguments_and_register_its_names():
    cfg = I.config("one_split", fusion_droppath=0.1)
    m = FL.GroundingDinoFusionLayer(cfg, init_values=1e-4)
    assert [n for n, _ in m.named_parameters()] == PARAMETER_NAMES
    assert isinstance(m.drop_path, FL.GroundingDinoDropPath) and m.drop_path.drop_prob == 0.1 and "p=0.1" in repr(m.drop_path)
    assert isinstance(FL.GroundingDinoFusionLayer(I.config("one_split")).drop_path, nn.Identity)
    assert torch.equal(m.vision_param.detach(), 1e-4 * torch.ones(64)) and torch.equal(m.text_param.detach(), 1e-4 * torch.ones(64))
    a = FL.GroundingDinoBiMultiHeadAttention(cfg)
    assert (a.embed_dim, a.num_heads, a.head_dim, a.vision_dim, a.text_dim, a.scale, a.dropout) == (256, 2, 128, 64, 64, 128 ** -0.5, 0.0)
    with pytest.raises(ValueError, match=r"`embed_dim` must be divisible by `num_heads` \(got `embed_dim`: 256 and `num_heads`: 3\)\."):
        FL.GroundingDinoBiMultiHeadAttention(types.SimpleNamespace(d_model=64, encoder_ffn_dim=512, encoder_attention_heads=6, fusion_dropout=0.0))
    d = FL.GroundingDinoDropPath(0.5)
    x = torch.ones(4, 3)
    assert d.eval()(x) is x
    import visionllm_amd
    for n in ("GroundingDinoFusionLayer", "GroundingDinoBiMultiHeadAttention", "GroundingDinoDropPath"):
        assert getattr(visionllm_amd, n) is getattr(FL, n) and n in visionllm_amd.__all__


def test_composed_path_reproduces_the_references_own_fp64_run():
    z = np.load(GOLDEN)
    C, FFN, HEADS = (int(x) for x in z["config"])
    cfg = types.SimpleNamespace(d_model=C, encoder_ffn_dim=FFN, encoder_attention_heads=HEADS, fusion_dropout=0.0, fusion_droppath=0.1)
    m = FL.GroundingDinoFusionLayer(cfg).double().eval()
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    assert sorted(sd) == sorted(PARAMETER_NAMES)
    m.load_state_dict(sd, strict=True)
    assert 0.5 <= float(m.vision_param.detach().min()) and float(m.vision_param.detach().max()) <= 1.5          # O(1), not the constructor's 1e-4
    vision, text = torch.from_numpy(z["vision"]), torch.from_numpy(z["text"])
    assert tuple(vision.shape) == (2, 37, 64) and tuple(text.shape) == (2, 5, 64) and vision.dtype == torch.float64
    vm, tm = torch.from_numpy(z["attention_mask_vision"]), torch.from_numpy(z["attention_mask_text"])
    assert vm.any() and tm.any()
    with torch.no_grad():
        (ov, wv), (ot, wt) = m(vision, text, vm, tm)
    assert tuple(wv.shape) == (4, 37, 5) and tuple(wt.shape) == (4, 5, 37)
    for got, name in ((ov, "out_vision"), (ot, "out_text")):
        want = torch.from_numpy(z[name])
        assert torch.isfinite(want).all()
        print(name, "max abs difference", (got - want).abs().max().item())
        assert torch.allclose(got, want, rtol=2e-6, atol=2e-6), name


def test_routing_every_reason_yields_exactly_that_reason():
    name = "one_split"
    t32 = I.make_inputs(name, "both")
    t = {k: I.fake(v) for k, v in t32.items()}
    with torch.no_grad():
        m = I.fake_module(I.make_layer(name))
        assert I.reasons(m, t) == [] and m.native_layer_applies(t["vision"], t["text"]) is True          # the baseline: nothing to object to

        def one(why, mod=m, tt=t):
            got = I.reasons(mod, tt)
            assert len(got) == 1 and why in got[0], (why, got)
        m.train()
        one("training mode")
        m.eval()
        one("bf16 CUDA tensors", tt=dict(t, vision=I.fake(t32["vision"].float())))          # fp32
        one("bf16 CUDA tensors", tt=dict(t, text=t32["text"]))                                # not on the GPU
        one("bf16 CUDA tensors", tt=dict(t, vision=I.fake(t32["vision"][0])))                 # not [B, S, C]
        wide = I.fake(torch.zeros(2, 300, 128, dtype=torch.bfloat16)[:, :, ::2])
        assert wide.stride(-1) == 2
        one("contiguous last dim", tt=dict(t, vision=wide))
        one("shapes", tt=dict(t, text=I.fake(t32["text"][:1])))                               # another batch
        one("shapes", tt=dict(t, vision=I.fake(torch.zeros(2, 300, 128, dtype=torch.bfloat16))))
        one("shapes", tt=dict(t, text=I.fake(t32["text"][:, :0]), attention_mask_text=None))  # no text token
        # a head dim outside the contract: embed 256 over 4 heads = 64
        other = I.fake_module(FL.GroundingDinoFusionLayer(I.config(name, encoder_attention_heads=8)))
        one("head dim 128 or 256", mod=other)
        one("attention_mask_vision: bool", tt=dict(t, attention_mask_vision=t32["attention_mask_vision"].to(torch.uint8)))
        one("attention_mask_text: bool", tt=dict(t, attention_mask_text=t32["attention_mask_text"].float()))
        one("attention_mask_text: bool", tt=dict(t, attention_mask_text=t32["attention_mask_text"][:, :3]))
        half = I.fake_module(I.make_layer(name))
        half.attn.out_text_proj.float()
        one("parameters: bf16 on the GPU", mod=half)
    one("requires_grad under grad mode")                                       # grad mode, trainable parameters
    frozen = I.fake_module(I.copy.deepcopy(I.make_layer(name)).requires_grad_(False))
    assert I.reasons(frozen, t) == []                                          # frozen: grad mode alone is no reason
    x = I.fake(t32["vision"].float().requires_grad_(True).to(torch.bfloat16))
    assert x.requires_grad
    one("requires_grad under grad mode", mod=frozen, tt=dict(t, vision=x))


def test_the_switch_is_off_by_default_and_the_cpu_never_takes_the_native_call(monkeypatch):
    assert FL.GroundingDinoFusionLayer.native_layer is False
    m = I.make_layer("one_split")
    t = I.to(I.make_inputs("one_split", "both"), "cpu", torch.float32)
    monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", True)
    before = calls()
    with torch.no_grad():
        on = I.call(m, t)
        monkeypatch.setattr(FL.GroundingDinoFusionLayer, "native_layer", False)
        off = I.call(m, t)
    assert calls() == before and I.reasons(m, t) != []
    assert on[2][0] is not None and torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


# ---- the conditions the inputs are meant to meet -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", I.xattn_cases(), ids=lambda c: "D{}-{}x{}-H{}-B{}".format(*c[:5]))
def test_kernel_inputs_meet_their_conditions(case):
    D, Lq, Lk, H, B, long_keys = case
    kps = I.plan(B, Lq, Lk, H, D)[1]
    for pattern in I.patterns(Lk, long_keys):
        ref, mag, share, std = I.xattn_reference(D, Lq, Lk, H, B, pattern)
        assert 1.0 <= std <= 4.0, (case, std)
        mask, said, dead_images = I.key_mask(pattern, B, Lk, kps)
        assert abs(share - said) < 1e-12 and (pattern is None) == (share == 0.0), (case, pattern, share, said)
        dead = torch.isnan(ref).all(-1).all(-1)
        want_dead = torch.zeros(B, Lq, dtype=torch.bool)
        want_dead[dead_images] = True
        assert torch.equal(dead, want_dead) and torch.equal(torch.isnan(ref), dead[:, :, None, None].expand_as(ref)), (case, pattern)
        if pattern in ("first_split", "middle_split"):
            lo = 0 if pattern == "first_split" else kps
            assert mask[:, lo:lo + kps].all() and int(mask.sum()) == B * kps          # a whole split, nothing else
        # the reference's clamped statements give the exact masked softmax on these inputs: the header's departures are not exercised
        live = ~torch.isnan(ref)
        clamped = I.xattn_clamped(D, Lq, Lk, H, B, pattern)
        assert torch.equal(torch.isnan(clamped), ~live)
        if live.any():
            assert (clamped[live] - ref[live]).abs().max().item() <= 1e-12, (case, pattern)


@pytest.mark.parametrize("name,masks", I.LAYER_CASES, ids=[f"{s}-{m}" for s, m in I.LAYER_CASES])
def test_layer_inputs_meet_their_conditions(name, masks):
    sh = I.shape_of(name)
    s = I.layer_scores(name)
    std = s.std(unbiased=False).item()
    print(name, "score std", std)
    assert 1.0 <= std <= 4.0
    m = I.make_layer(name)
    for p in (m.vision_param.detach(), m.text_param.detach()):
        assert 0.5 <= float(p.min()) and float(p.max()) <= 1.5 and float(p.max() - p.min()) > 0.5
    vm, tm = I.layer_masks(name, masks)
    sv, st = I.said_shares(name, masks)
    assert abs((0.0 if vm is None else vm.double().mean().item()) - sv) < 1e-12 and abs((0.0 if tm is None else tm.double().mean().item()) - st) < 1e-12
    # both directions by the reference's clamped statements against the exact masked softmax, in fp64, from the layer's own q / k
    d = I.copy.deepcopy(m).double()
    a = d.attn
    vision, text = (x.double() for x in I.raw_inputs(name))
    with torch.no_grad():
        v, t = d.layer_norm_vision(vision), d.layer_norm_text(text)
        q, k = I._heads(a.vision_proj(v), sh.B, sh.H, sh.D), I._heads(a.text_proj(t), sh.B, sh.H, sh.D)
        vv, vt = I._heads(a.values_vision_proj(v), sh.B, sh.H, sh.D), I._heads(a.values_text_proj(t), sh.B, sh.H, sh.D)
        for qq, kk, val, mask in ((q, k, vt, tm), (k, q, vv, vm)):
            exact = I.exact_attention(qq, kk, val, mask, a.scale)[0]
            clamped = I.clamped_attention(qq, kk, val, mask, a.scale)
            live = ~torch.isnan(exact)
            assert torch.equal(torch.isnan(clamped), ~live)
            assert (clamped[live] - exact[live]).abs().max().item() <= 1e-12
    ov, ot = I.reference(name, masks)
    assert tuple(ov.shape) == (sh.B, sh.S, sh.C) and tuple(ot.shape) == (sh.B, sh.Lt, sh.C) and torch.isfinite(ot).all()
    dead = torch.isnan(ov)
    if masks == I.DEAD:          # exactly image 1 of the vision output
        assert dead[1].all() and not dead[0].any()
    else:
        assert not dead.any()
