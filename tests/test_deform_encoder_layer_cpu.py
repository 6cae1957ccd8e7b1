"""CPU: the boundary of the native deformable encoder layer (include/vllm_hip.h, section f2b) -- symbols, descriptor layout, the size
query, the argument gates (refused calls only, fake pointers: nothing is dereferenced, no device is touched), and the module mirrors
where no GPU is needed: the cases' own conditions, the switch on CPU tensors, the layer chain with the switch off, and every reason
``native_layer_reasons`` has to say no (in the decoder layers' words where the condition is shared)."""
import ctypes
import re
import subprocess

import pytest
import torch
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import deformable_encoder as E

import deform_encoder_layer_inputs as I

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
NEW = ("vllm_deform_enc_layer_desc_sizeof", "vllm_deform_enc_layer_workspace_bytes", "vllm_deform_enc_layer_calls",
       "vllm_deform_enc_layer_forward", "vllm_add_layernorm_bf16", "vllm_add_bf16", "vllm_gemm_bf16_relu")
ATTN_POINTERS = ("value_proj_w", "value_proj_b", "sampling_offsets_w", "sampling_offsets_b", "attention_weights_w", "attention_weights_b",
                 "output_proj_w", "output_proj_b")
POINTERS = ("norm1_w", "norm1_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "norm2_w", "norm2_b")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def desc(C=256, M=8, Lv=4, P=4, F=2048, act=0, ref_dim=2, **ptrs):
    d = _lib.VllmDeformEncLayerDesc()
    a = d.attn
    a.d_model, a.n_heads, a.n_levels, a.n_points, a.ref_dim = C, M, Lv, P, ref_dim
    d.d_ffn, d.act, d.norm1_eps, d.norm2_eps = F, act, 1e-5, 1e-5
    for n in ATTN_POINTERS:
        setattr(a, n, ptrs.get(n, PTR))
    for n in POINTERS:
        setattr(d, n, ptrs.get(n, PTR))
    return d


def last_error():
    return _lib.lib().vllm_last_error().decode()


def forward(d, B=2, S=161, src=PTR, pos=PTR, query_in=0, ref=PTR, shapes=PTR, lsi=PTR, out=PTR, query_out=0, ws=PTR, ws_bytes=1 << 40):
    return _lib.lib().vllm_deform_enc_layer_forward(ctypes.byref(d), vp(src), vp(pos), vp(query_in), vp(ref), None, vp(shapes), vp(lsi), B, S,
                                                    vp(out), vp(query_out), vp(ws), ws_bytes, None)


@pytest.fixture
def slab_option():
    """restores the process-wide option "deform_enc_ffn_slab_rows" behind a test that sets it"""
    L = _lib.lib()
    old = L.vllm_set_option(b"deform_enc_ffn_slab_rows", 0)
    L.vllm_set_option(b"deform_enc_ffn_slab_rows", old)
    yield lambda v: L.vllm_set_option(b"deform_enc_ffn_slab_rows", v)
    L.vllm_set_option(b"deform_enc_ffn_slab_rows", old)


def test_symbols_are_declared_and_exported_and_the_abi_version_stays_2():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T vllm_" in line}
    for n in NEW:
        assert n in protos, n
        assert n in exported, n
    assert _lib.header_abi_version() == 2 and _lib.lib().vllm_abi_version() == 2
    assert "f2b. The whole deformable ENCODER layer" in open(_lib.HEADER).read()


def test_descriptor_mirror_has_the_library_size_and_the_header_order():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.VllmDeformEncLayerDesc) == L.vllm_deform_enc_layer_desc_sizeof()
    _lib.check_struct_layouts()
    hdr = open(_lib.HEADER).read()
    body = hdr[hdr.index("typedef struct VllmDeformEncLayerDesc {"):hdr.index("} VllmDeformEncLayerDesc;")]
    order = [re.search(r"\b" + n + r"\b", body).start() for n, _ in _lib.VllmDeformEncLayerDesc._fields_]
    assert order == sorted(order), "field order differs from include/vllm_hip.h"
    assert _lib.VllmDeformEncLayerDesc._fields_[0] == ("attn", _lib.VllmMsdaLayerDesc)
    assert L.vllm_deform_enc_layer_calls() >= 0


def test_workspace_query_is_positive_monotone_and_shrinks_with_a_slab(slab_option):
    L = _lib.lib()
    d = desc()
    q = lambda b, s: L.vllm_deform_enc_layer_workspace_bytes(ctypes.byref(d), b, s)
    a256 = lambda x: (x + 255) & ~255
    slab_option(0)
    base = q(2, 161)
    assert base > 0
    # the query / linear2's output, src + attn, the whole intermediate, and the attention layer's own workspace
    attn = L.vllm_msda_layer_workspace_bytes(ctypes.byref(d.attn), 2, 161, 161)
    assert attn > 0 and base == 2 * a256(322 * 256 * 2) + a256(322 * 2048 * 2) + attn
    assert q(3, 161) > base and q(2, 162) > base and q(2, 161) == base
    assert q(0, 161) == 0 and q(2, 0) == 0 and q(-1, 161) < 0 and q(1 << 16, 1 << 15) < 0
    slab_option(64)
    assert q(2, 161) == base - a256(322 * 2048 * 2) + a256(64 * 2048 * 2)
    assert q(3, 161) > q(2, 161)
    slab_option(1000)          # more rows than there are: the whole tensor
    assert q(2, 161) == base
    assert L.vllm_set_option(b"deform_enc_ffn_slab_rows", -1) == EINVAL and "deform_enc_ffn_slab_rows" in last_error()
    assert L.vllm_deform_enc_layer_workspace_bytes(None, 2, 161) < 0


@pytest.mark.parametrize("kw,word", [
    (dict(act=7), "unknown act"),
    (dict(act=2), "unknown act"),                 # quick-GELU is a GEMM epilogue, not an activation of these layers
    (dict(F=2000), "d_ffn"),
    (dict(F=0), "d_ffn"),
    (dict(ref_dim=4), "ref_dim"),
    (dict(C=576, M=9), "above 512"),
    (dict(C=80, M=8), "multiple of 64"),
], ids=["act7", "act_quick_gelu", "d_ffn2000", "d_ffn0", "ref_dim4", "d_model576", "d_model80"])
def test_refused_descriptors_have_their_own_messages(kw, word):
    L = _lib.lib()
    d = desc(**kw)
    calls = L.vllm_deform_enc_layer_calls()
    assert L.vllm_deform_enc_layer_workspace_bytes(ctypes.byref(d), 2, 161) < 0
    assert word in last_error(), last_error()
    assert forward(d) == EINVAL
    assert word in last_error() and "workspace" not in last_error(), last_error()
    assert L.vllm_deform_enc_layer_calls() == calls


def test_null_and_misaligned_operands_have_their_own_messages():
    L = _lib.lib()
    d = desc()
    calls = L.vllm_deform_enc_layer_calls()
    for kw in (dict(src=0), dict(ref=0), dict(shapes=0), dict(lsi=0), dict(out=0)):
        assert forward(d, **kw) == EINVAL, kw
        assert "null pointer" in last_error() and "workspace" not in last_error(), (kw, last_error())
    assert forward(d, pos=0, query_out=PTR) == EINVAL and "query_out needs pos" in last_error()
    for kw in (dict(src=PTR + 8), dict(pos=PTR + 8), dict(query_in=PTR + 8), dict(out=PTR + 8), dict(query_out=PTR + 8), dict(ref=PTR + 4)):
        assert forward(d, **kw) == EINVAL, kw
        assert "misaligned src" in last_error() and "workspace" not in last_error(), (kw, last_error())
    for name in ATTN_POINTERS + POINTERS:
        assert forward(desc(**{name: PTR + 8})) == EINVAL, name
        assert "misaligned weight or bias" in last_error(), (name, last_error())
        assert forward(desc(**{name: 0})) == EINVAL, name
        assert "missing weights" in last_error(), (name, last_error())
    assert forward(d, B=1 << 16, S=1 << 15) == EINVAL and "2^31" in last_error()
    assert forward(d, B=-1) == EINVAL and "2^31" in last_error()
    # B S == 0: nothing to do, whatever the pointers are
    assert forward(d, B=0, src=0, out=0, ws=0, ws_bytes=0) == 0 and forward(d, S=0, src=0, out=0, ws=0, ws_bytes=0) == 0
    assert L.vllm_deform_enc_layer_calls() == calls          # no refused call reached a launch


def test_short_misaligned_and_null_workspaces_are_refused(slab_option):
    L = _lib.lib()
    d = desc()
    for slab in (0, 64):
        slab_option(slab)
        need = L.vllm_deform_enc_layer_workspace_bytes(ctypes.byref(d), 2, 161)
        assert need > 0
        calls = L.vllm_deform_enc_layer_calls()
        for w, n in ((PTR, need - 1), (PTR + 8, need), (PTR + 8, need + 4096), (0, need)):
            assert forward(d, ws=w, ws_bytes=n) == EINVAL
            assert "workspace" in last_error(), last_error()
        assert L.vllm_deform_enc_layer_calls() == calls


def test_kernel_entries_refuse_what_they_cannot_run():
    L = _lib.lib()
    p = vp(PTR)
    ln = lambda C=256, rows=5, x=p, ldx=256, res=None, ldr=0, pos=None, ypos=None, ldq=0: L.vllm_add_layernorm_bf16(
        x, ldx, res, ldr, p, p, p, 256 if C <= 256 else C, pos, 256, ypos, ldq, rows, C, 1e-5, None)
    assert ln(C=96) == EINVAL and "multiple of 64" in last_error()
    assert ln(C=576) == EINVAL and "multiple of 64" in last_error()
    assert ln(x=None) == EINVAL and "null pointer" in last_error()
    assert ln(ypos=p) == EINVAL and "null pointer" in last_error()              # y_pos without pos
    assert ln(x=vp(PTR + 8)) == EINVAL and "misaligned" in last_error()
    assert ln(ldx=252) == EINVAL and "misaligned" in last_error()                # a row stride below C
    assert ln(res=p, ldr=260) == EINVAL and "misaligned" in last_error()         # no multiple of 8
    assert ln(pos=p, ypos=p, ldq=8) == EINVAL and "misaligned" in last_error()
    assert ln(rows=0, x=None) == 0
    assert L.vllm_add_bf16(None, p, p, 5, None) == EINVAL and "null pointer" in last_error()
    assert L.vllm_add_bf16(p, p, p, -1, None) == EINVAL
    assert L.vllm_add_bf16(None, None, None, 0, None) == 0
    assert L.vllm_gemm_bf16_relu(None, p, p, p, 77, 128, 64, 64, 64, 128, 0, None) == EINVAL and "null pointer" in last_error()
    assert L.vllm_gemm_bf16_relu(p, p, p, p, 77, 128, 64, 64, 64, 128, 1, None) == EINVAL and "force_bits" in last_error()
    assert L.vllm_gemm_bf16_relu(p, p, p, p, 77, 128, 60, 64, 64, 128, 0, None) == EINVAL and "K=60" in last_error()


def test_the_public_gemm_entry_still_refuses_epilogue_7():
    """the ReLU epilogue is an internal number: the public word 7 stays unknown, with or without force bits"""
    L = _lib.lib()
    p = vp(PTR)
    for epi in (7, 105, 7 | 0x100):
        assert L.vllm_gemm_bf16(p, p, p, p, 77, 128, 64, 64, 64, 128, epi, None, None, 0, 0, None) == EINVAL
        assert f"unknown epilogue {epi & 0xff}" in last_error(), last_error()


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("case", I.CASES, ids=I.IDS)
def test_every_case_pads_some_rows_and_takes_both_relu_branches(flavour, case):
    padded, negative = I.conditions(flavour, *case)
    print(f"{flavour} {case}: padded {padded}, negative pre-activation {negative:.3f}")
    assert (padded is None) == (not case[2])
    assert padded is None or 0.10 <= padded <= 0.30
    assert 0.30 <= negative <= 0.70


def test_constructors_take_the_reference_arguments_and_names():
    m = I.make_layer("unipose", "small")
    assert [n for n, _ in m.named_children()] == ["self_attn", "dropout1", "norm1", "linear1", "dropout2", "linear2", "dropout3", "norm2"]
    assert isinstance(m.self_attn, E.MSDeformAttn) and m.activation is torch.nn.functional.relu
    g = I.make_layer("gdino", "gelu")
    assert [n for n, _ in g.named_children()] == ["self_attn", "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm"]
    assert isinstance(g.self_attn, E.GroundingDinoMultiscaleDeformableAttention) and g.activation_fn is torch.nn.functional.gelu
    assert E.DeformableTransformerEncoderLayer.native_layer is False and E.GroundingDinoDeformableLayer.native_layer is False
    assert not any("native" in k for k in list(m.state_dict()) + list(g.state_dict()))
    with pytest.raises(NotImplementedError, match="add_channel_attention"):
        E.DeformableTransformerEncoderLayer(add_channel_attention=True)
    with pytest.raises(NotImplementedError, match="use_deformable_box_attn"):
        E.DeformableTransformerEncoderLayer(use_deformable_box_attn=True)
    assert isinstance(E.DeformableTransformerEncoderLayer(activation="prelu").activation, nn.PReLU)
    import visionllm_amd
    assert visionllm_amd.DeformableTransformerEncoderLayer is E.DeformableTransformerEncoderLayer
    assert visionllm_amd.GroundingDinoDeformableLayer is E.GroundingDinoDeformableLayer
    assert visionllm_amd.encoder_layers_forward is E.encoder_layers_forward


@pytest.mark.parametrize("flavour", I.FLAVOURS)
def test_the_switch_changes_nothing_on_the_cpu(flavour, monkeypatch):
    """On, CPU tensors still take the composed path: the operator raises as before, and with the operator's CPU twin in its place the
    result has the bits of the run with the switch off.  No call reaches the library."""
    m = I.make_layer(flavour, "small")
    t = I.to(I.make_inputs("small"), "cpu", torch.float32)
    calls = _lib.lib().vllm_deform_enc_layer_calls()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            I.call(flavour, m, t)
        with I.cpu_operator():
            off = I.call(flavour, m, t)
        monkeypatch.setattr(type(m), "native_layer", True)
        assert m.native_layer is True
        assert not m.native_layer_applies(t["src"], t["pos"], t["reference_points"])
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            I.call(flavour, m, t)
        with I.cpu_operator():
            on = I.call(flavour, m, t)
            bf = I.call(flavour, I.as_bf16(m, "cpu"), I.to(I.make_inputs("small"), "cpu"))       # bf16, but not on the GPU
    assert torch.equal(on, off) and bf.dtype == torch.bfloat16
    assert _lib.lib().vllm_deform_enc_layer_calls() == calls


@pytest.mark.parametrize("flavour", I.FLAVOURS)
@pytest.mark.parametrize("with_pos,with_mask", [(True, True), (False, False)])
def test_encoder_layers_forward_with_the_switch_off_is_the_plain_loop(flavour, with_pos, with_mask):
    layers = [I.make_layer(flavour, "small"), I.make_layer(flavour, "small", activation="gelu")]
    with torch.no_grad():
        layers[1].self_attn.value_proj.weight.mul_(0.5)          # two different layers
    t = I.to(I.make_inputs("small", with_pos, with_mask), "cpu", torch.float32)
    with torch.no_grad(), I.cpu_operator():
        x = t["src"]
        for layer in layers:
            x = I.call(flavour, layer, dict(t, src=x))
        got = E.encoder_layers_forward(layers, t["src"], t["pos"], t["reference_points"], t["spatial_shapes"], t["level_start_index"],
                                       t["padding_mask"])
    assert torch.equal(got, x)
    ref = I.reference(flavour, "small", with_pos, with_mask)[0]
    with torch.no_grad(), I.cpu_operator():
        one = E.encoder_layers_forward(layers[:1], t["src"], t["pos"], t["reference_points"], t["spatial_shapes"], t["level_start_index"],
                                       t["padding_mask"])
    assert (one.double() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()          # fp32 against the fp64 yardstick


def reasons(flavour, m, t, **kw):
    return m.native_layer_reasons(t["src"], t["pos"], t["reference_points"], **kw)


DEVICE_ONLY = ["src: a bf16 CUDA tensor [B, S, C]", "pos / query_in: bf16 CUDA tensors of src's shape", "parameters: bf16 on the GPU",
               "self-attention: msda_layer_fused_ok"]


@pytest.mark.parametrize("flavour", I.FLAVOURS)
def test_every_reason_to_keep_the_composed_path(flavour):
    """CPU tensors: a frozen bf16 module on bf16 inputs has the device reasons and no other; every other condition adds its own reason
    when, and only when, it is broken; ``native_layer_applies`` is ``not native_layer_reasons`` throughout."""
    def frozen(**kw):
        mod = I.as_bf16(I.make_layer(flavour, "small", **kw), "cpu")
        for p in mod.parameters():
            p.requires_grad_(False)
        return mod

    m = frozen()
    t = I.to(I.make_inputs("small"), "cpu")
    assert reasons(flavour, m, t) == DEVICE_ONLY
    assert reasons(flavour, m, dict(t, pos=None)) == [r for r in DEVICE_ONLY if not r.startswith("pos")]

    def extra(mod=m, tt=t, **kw):
        got = reasons(flavour, mod, tt, **kw)
        assert got and not mod.native_layer_applies(tt["src"], tt["pos"], tt["reference_points"], **kw)
        return [r for r in got if r not in DEVICE_ONLY]

    assert extra() == []
    # the switch test's case (fp32 tensors on the CPU, an fp32 module): the input's own reason comes first
    f32, t32 = I.make_layer(flavour, "small"), I.to(I.make_inputs("small"), "cpu", torch.float32)
    assert not f32.native_layer_applies(t32["src"], t32["pos"], t32["reference_points"])
    assert reasons(flavour, f32, t32)[0] == DEVICE_ONLY[0] and "parameters: bf16 on the GPU" in reasons(flavour, f32, t32)
    grad = "requires_grad under grad mode: there is no native backward"
    for p in m.parameters():
        p.requires_grad_(True)
    with torch.enable_grad():
        assert extra() == [grad]
    with torch.no_grad():
        assert extra() == []
    for p in m.parameters():
        p.requires_grad_(False)
    with torch.enable_grad():
        assert extra(tt=dict(t, src=t["src"].clone().requires_grad_(True))) == [grad]
        assert extra(tt=dict(t, pos=t["pos"].clone().requires_grad_(True))) == [grad]
    m.train()
    assert extra() == ["active dropout"]
    m.eval()
    assert extra(frozen(dropout=0.0).train()) == []
    assert extra(frozen(activation="prelu" if flavour == "unipose" else "silu")) == ["activation: relu or gelu"]
    ref4 = torch.cat([t["reference_points"], torch.full_like(t["reference_points"], 0.2)], -1)
    assert extra(tt=dict(t, reference_points=ref4)) == ["reference_points: last dim 2"]
    assert extra(tt=dict(t, reference_points=None)) == ["reference_points: last dim 2"]
    assert extra(tt=dict(t, pos=t["pos"][:, :-1])) == []          # (the pos reason is among the device ones already)
    assert extra(tt=dict(t, src=t["src"][0])) == [] and reasons(flavour, m, dict(t, src=t["src"][0])) == DEVICE_ONLY[:1]
    broken = frozen()
    (broken.linear1 if flavour == "unipose" else broken.fc1).bias = None
    assert extra(broken) == ["parameters: a Linear / LayerNorm without bias"]
    if flavour == "gdino":
        assert extra(output_attentions=True) == ["output_attentions: the attention weights stay inside the native call"]
    meta = I.to(t, "meta")                                         # decided without touching data
    assert reasons(flavour, m, meta)[0] == DEVICE_ONLY[0]


def test_d_model_and_d_ffn_conditions():
    t = I.to(I.make_inputs("small"), "cpu")
    m = E.DeformableTransformerEncoderLayer(d_model=t["src"].shape[-1], d_ffn=100, n_levels=t["reference_points"].shape[2])
    assert "d_model a multiple of 64 up to 512, d_ffn a multiple of 64" in reasons("unipose", m, t)


class FakeCuda(torch.Tensor):
    """a CPU tensor that says it is on the GPU: the reasons are decided from dtypes, shapes and flags alone"""
    @property
    def is_cuda(self):
        return True


def fake_inputs(t):
    return {k: v.as_subclass(FakeCuda) if torch.is_tensor(v) else v for k, v in t.items()}


def fake_module(m):
    """a frozen bf16 copy of ``m`` whose parameters say they are on the GPU"""
    m = I.as_bf16(m, "cpu")
    for mod in m.modules():
        for k, p in list(mod._parameters.items()):
            if p is not None:
                mod._parameters[k] = nn.Parameter(p.data, requires_grad=False).as_subclass(FakeCuda)
    return m


@pytest.mark.parametrize("flavour", I.FLAVOURS)
def test_encoder_and_decoder_layers_name_a_shared_condition_alike(flavour):
    """Tensors and parameters that say they are on the GPU: both layers have nothing to object to, and a parameter left in fp32, a
    dropout that training mode applies and an activation outside relu / gelu draw the same one string from both."""
    import deform_decoder_layer_inputs as DI
    te, td = fake_inputs(I.to(I.make_inputs("small"), "cpu")), fake_inputs(DI.to(DI.make_inputs("small"), "cpu"))

    def both(change=lambda m: m, **kw):
        with torch.no_grad():
            enc, dec = (change(fake_module(X.make_layer(flavour, "small", **kw))) for X in (I, DI))
            assert enc.native_layer_applies(te["src"], te["pos"], te["reference_points"]) == (not reasons(flavour, enc, te))
            return reasons(flavour, enc, te), DI.applies(flavour, dec, td)

    def fp32_weight(m):
        fc2 = m.linear2 if flavour == "unipose" else m.fc2
        fc2.weight.data = fc2.weight.data.float()
        return m

    assert both() == ([], [])
    assert both(fp32_weight) == (["parameters: bf16 on the GPU"],) * 2
    assert both(lambda m: m.train()) == (["active dropout"],) * 2
    assert both(activation="prelu" if flavour == "unipose" else "silu") == (["activation: relu or gelu"],) * 2
