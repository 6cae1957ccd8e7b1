"""CPU: the host side of the embeddings' training path (no GPU): the new symbols and the struct are declared and exported, the ctypes
mirror has the library's size, the workspace query answers without a device and refuses bad descriptors, an fp32 emulation of the new
kernels' arithmetic stays inside the GPU tests' per-element bounds at every case (so a faithful implementation can meet them), CPU
tensors raise, and ``native_training`` is off by default."""
import ctypes

import pytest
import torch

import embed_train_inputs as E
from visionllm_amd import _lib
from visionllm_amd._lib import VllmVitEmbed
from visionllm_amd.clip_vit import _CLIPVisionEmbeddings
from visionllm_amd.intern_vit import InternVisionConfig, InternVisionEmbeddings, InternVisionModel

SYMBOLS = ("vllm_vit_embed_workspace_bytes", "vllm_vit_embed_forward", "vllm_vit_embed_backward")


def test_symbols_and_struct_are_declared_and_exported():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in SYMBOLS + ("vllm_vit_embed_sizeof",):
        assert name in protos, name
        assert getattr(L, name) is not None
    assert "typedef struct VllmVitEmbed" in open(_lib.HEADER).read()
    assert protos["vllm_vit_embed_workspace_bytes"][0] is ctypes.c_long
    assert len(protos["vllm_vit_embed_forward"][1]) == 7 and len(protos["vllm_vit_embed_backward"][1]) == 11
    assert L.vllm_abi_version() == 2                       # additions only


def test_sizeof_matches_the_mirror():
    L = _lib.lib()
    _lib.check_struct_layouts()
    assert L.vllm_vit_embed_sizeof() == ctypes.sizeof(VllmVitEmbed) == 4 * 4 + 4 * 8


def _desc(hidden=128, patch=14, image=70):
    one = ctypes.c_void_p(1 << 20)
    return VllmVitEmbed(hidden=hidden, patch=patch, image=image, pixel_is_f32=0, patch_w=one, patch_b=one, cls=one, pos=one)


def test_workspace_query_is_host_only_and_refuses_bad_descriptors():
    L = _lib.lib()
    q = lambda d, n: L.vllm_vit_embed_workspace_bytes(ctypes.byref(d), n)
    small, big = q(_desc(), 3), q(_desc(), 40)
    assert 0 < small < big
    assert q(_desc(), 0) > 0
    # it holds at least the padded weight / dW, the im2col matrix with a CLS row per tile and the bias partials
    S, kpad = 26, E.kpad_for(14)
    assert small >= 128 * kpad * 2 + 3 * S * kpad * 2 + ((S + E.TS_ROWS - 1) // E.TS_ROWS) * 128 * 4
    assert q(_desc(hidden=100), 3) < 0 and b"hidden" in L.vllm_last_error()      # hidden % 64
    assert q(_desc(image=72), 3) < 0 and b"patch" in L.vllm_last_error()         # image % patch
    assert q(_desc(hidden=8256), 3) < 0                                          # > 8192
    assert q(_desc(), -1) < 0
    d = _desc()
    d.patch_w = None
    assert q(d, 3) < 0


@pytest.mark.parametrize("case", range(len(E.CASES)))
def test_emulation_meets_the_bounds(case):
    n, image, patch, C, bias, pdt = E.CASES[case]
    c = E.make_case(*E.CASES[case], seed=case)
    ref, mag = E.reference(c, patch)
    gpos, gcls, gb = E.emulate_tile_sums(c["gout"])
    gw = E.emulate_wgrad(c["gout"], c["pix"], patch)
    assert torch.equal(gcls, gpos[0])
    rows = [("pos", gpos, ref["pos"][0], mag["pos"][0]), ("cls", gcls, ref["cls"].view(-1), mag["cls"].view(-1)),
            ("w", gw, ref["w"].view(C, -1), mag["w"].view(C, -1))]
    if bias:
        rows.append(("b", gb, ref["b"], mag["b"]))
    for name, a, r, m in rows:
        e = E.excess_ulp(a, r, m)
        print(f"case {case} {name}: {e:.3f} of the bound")
        assert e <= 1.0, name
    # the restated statements' own fp64 autograd is the same function
    _, g64 = E.autograd_embeddings(c, patch, torch.float64)
    for k in ("w", "b", "cls", "pos"):
        if ref[k] is None:
            assert g64[k] is None
        else:
            assert g64[k].shape == ref[k].shape and torch.allclose(g64[k], ref[k], rtol=1e-9, atol=1e-12), k


def test_restated_im2col_is_the_convolution():
    c = E.make_case(*E.CASES[0])
    pix, w = c["pix"].double(), c["w"].double()
    y = torch.nn.functional.conv2d(pix, w, None, stride=14).flatten(2).transpose(1, 2)
    assert torch.allclose(E.im2col(pix, 14) @ w.view(128, -1).T, y, rtol=1e-12, atol=1e-12)


def test_cpu_tensors_raise():
    cfg = InternVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=1, image_size=70, patch_size=14)
    emb = InternVisionEmbeddings(cfg).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="CUDA"):
        emb(torch.zeros(1, 3, 70, 70, dtype=torch.bfloat16))
    with torch.no_grad(), pytest.raises(RuntimeError, match="CUDA"):
        emb(torch.zeros(1, 3, 70, 70, dtype=torch.bfloat16))
    clip = _CLIPVisionEmbeddings(cfg).to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="CUDA"):
        clip(torch.zeros(1, 3, 70, 70, dtype=torch.bfloat16))


def test_native_training_is_off_by_default():
    cfg = InternVisionConfig(hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=1, image_size=70, patch_size=14)
    model = InternVisionModel(cfg)
    assert model.native_training is False
    with pytest.raises(ValueError, match="pixel_values or pixel_embeds"):
        model()
