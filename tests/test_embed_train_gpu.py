"""GPU: training the embeddings of the vision tower (embed_train.hip) and the tower from pixels.

Yardstick: torch fp64 autograd / closed forms of the reference's statements restated in embed_train_inputs.py, on the CPU, on the same
bf16 parameters, pixels and grad_out.  The C entry is judged per element (1 bf16 ulp + 2^-17 of the sum of the absolute terms); the
assembled tower by DESIGN section 5's rule: relative rms against fp64 <= 1.25 x that of torch's own bf16 autograd of the same statements
(both numbers are printed)."""
import ctypes
import functools

import pytest
import torch

import embed_train_inputs as E
import vit_layer_train_inputs as VI
from bounds import P, stream
from visionllm_amd import _lib
from visionllm_amd.clip_vit import CLIPVisionModel, _CLIPVisionEmbeddings
from visionllm_amd.intern_vit import InternVisionConfig, InternVisionEmbeddings, InternVisionModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
NAMES = ("w", "b", "cls", "pos")
PAD = 24   # NaN elements in front of and behind every gradient view (48 bytes: the views stay 16-byte aligned)


def desc_of(c, image, patch):
    C = c["w"].shape[0]
    return _lib.VllmVitEmbed(hidden=C, patch=patch, image=image, pixel_is_f32=1 if c["pix"].dtype == torch.float32 else 0,
                             patch_w=c["w"].data_ptr(), patch_b=c["b"].data_ptr() if c["b"] is not None else None,
                             cls=c["cls"].data_ptr(), pos=c["pos"].data_ptr())


def workspace(d, n):
    wsb = _lib.lib().vllm_vit_embed_workspace_bytes(ctypes.byref(d), n)
    assert wsb > 0, _lib.lib().vllm_last_error()
    return torch.empty(wsb, dtype=torch.uint8, device=DEV), wsb


def nan_buffers(c):
    """-> {name: (whole NaN buffer, the gradient view inside it)} in the parameters' shapes"""
    out = {}
    for k in NAMES:
        if c[k] is None:
            out[k] = (None, None)
            continue
        full = torch.full((c[k].numel() + 2 * PAD,), NAN, device=DEV).to(torch.bfloat16)
        out[k] = (full, full[PAD:PAD + c[k].numel()].view(c[k].shape))
    return out


def c_backward(c, image, patch, want=NAMES, n=None, d=None, ws=None):
    """vllm_vit_embed_backward straight through the C ABI on NaN-filled buffers -> (rc, buffers)"""
    L = _lib.lib()
    d = d if d is not None else desc_of(c, image, patch)
    n = c["pix"].shape[0] if n is None else n
    ws, wsb = ws if ws is not None else workspace(d, max(n, 1))
    bufs = nan_buffers(c)
    ptrs = [P(bufs[k][1]) if (k in want and bufs[k][1] is not None) else None for k in NAMES]
    rc = L.vllm_vit_embed_backward(ctypes.byref(d), P(c["pix"]), n, P(c["gout"]), *ptrs, P(ws), wsb, stream())
    torch.cuda.synchronize()
    return rc, bufs


def untouched(bufs, k):
    full, view = bufs[k]
    return bool(torch.isnan(full[:PAD].float()).all() and torch.isnan(full[PAD + view.numel():].float()).all())


@functools.lru_cache(maxsize=None)
def case(idx):
    """-> everything the tests of case `idx` share (computed once, never modified)"""
    n, image, patch, C, bias, pdt = E.CASES[idx]
    c = E.make_case(*E.CASES[idx], seed=idx, device=DEV)
    ref, mag = E.reference(c, patch)
    rc, bufs = c_backward(c, image, patch)
    assert rc == 0, _lib.lib().vllm_last_error()
    return dict(c=c, image=image, patch=patch, ref=ref, mag=mag, bufs=bufs, grads={k: bufs[k][1] for k in NAMES})


# ---- 1, 2: the C entry against fp64, nothing written outside the gradients ---------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(E.CASES)))
def test_backward_against_fp64(idx):
    L = _lib.lib()
    k = case(idx)
    n, image, patch, C, bias, pdt = E.CASES[idx]
    for name in NAMES:
        g = k["grads"][name]
        if k["c"][name] is None:
            assert g is None
            continue
        e = E.excess_ulp(g.cpu(), k["ref"][name], k["mag"][name])
        print(f"embed bwd case {idx} grad_{name}: {e:.3f} of the bound")
        assert e <= 1.0, name
        assert not torch.isnan(g.float()).any(), name
    assert torch.equal(k["grads"]["cls"].view(-1), k["grads"]["pos"][0, 0])
    if idx == E.SPLIT_CASE:
        S = (image // patch) ** 2 + 1
        assert L.vllm_gemm_wgrad_workspace_bytes(n * S, C, E.kpad_for(patch)) > 0


@pytest.mark.parametrize("idx", range(len(E.CASES)))
def test_no_overrun(idx):
    k = case(idx)
    for name in NAMES:
        if k["c"][name] is not None:
            assert untouched(k["bufs"], name), f"grad_{name}: wrote outside the tensor"


# ---- 3: NULL subsets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_null_subsets(idx):
    k = case(idx)
    for name in NAMES:
        if k["c"][name] is None:
            continue
        rc, bufs = c_backward(k["c"], k["image"], k["patch"], want=(name,))
        assert rc == 0
        assert torch.equal(bufs[name][1], k["grads"][name]), name
        assert untouched(bufs, name)
        for other in NAMES:
            if other != name and bufs[other][0] is not None:
                assert torch.isnan(bufs[other][0].float()).all(), f"asked for {name}, {other} was written"
    rc, bufs = c_backward(k["c"], k["image"], k["patch"], want=())
    assert rc == 0
    for name in NAMES:
        if bufs[name][0] is not None:
            assert torch.isnan(bufs[name][0].float()).all(), name


# ---- 4: determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", [0, 2, 5])
def test_deterministic(idx):
    k = case(idx)
    rc, bufs = c_backward(k["c"], k["image"], k["patch"])
    assert rc == 0
    for name in NAMES:
        if k["c"][name] is not None:
            assert torch.equal(bufs[name][1], k["grads"][name]), name


# ---- 5: refusals, and the empty batch ----------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_no_tiles_gives_zeros():
    L = _lib.lib()
    k = case(0)
    c, image, patch = k["c"], k["image"], k["patch"]
    good = desc_of(c, image, patch)
    ws = workspace(good, 3)
    ws[0].zero_()

    def refused(**kw):
        rc, bufs = c_backward(c, image, patch, **kw)
        assert rc == -1 and L.vllm_last_error()
        for name in NAMES:
            assert torch.isnan(bufs[name][0].float()).all(), name

    for field, value in (("hidden", 100), ("image", 72), ("patch", 0), ("patch_w", None), ("pixel_is_f32", 2)):
        bad = desc_of(c, image, patch)
        setattr(bad, field, value)
        refused(d=bad, ws=ws)
        out = torch.full((3, 26, 128), 7.0, device=DEV).to(torch.bfloat16)
        assert L.vllm_vit_embed_forward(ctypes.byref(bad), P(c["pix"]), 3, P(out), P(ws[0]), ws[1], stream()) == -1
        torch.cuda.synchronize()
        assert (out == 7.0).all()
    refused(ws=(ws[0], ws[1] - 256))                        # short workspace
    assert b"workspace" in L.vllm_last_error()
    refused(ws=(ws[0][8:], ws[1]))                          # misaligned workspace
    refused(n=-1, ws=ws)
    nobias = dict(c, b=None)
    bufs = nan_buffers(c)
    rc = L.vllm_vit_embed_backward(ctypes.byref(desc_of(nobias, image, patch)), P(c["pix"]), 3, P(c["gout"]), P(bufs["w"][1]), P(bufs["b"][1]),
                                   P(bufs["cls"][1]), P(bufs["pos"][1]), P(ws[0]), ws[1], stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"bias" in L.vllm_last_error()       # a bias gradient for a convolution without a bias
    assert all(torch.isnan(bufs[name][0].float()).all() for name in NAMES)
    assert (ws[0] == 0).all()
    rc, bufs = c_backward(c, image, patch, n=0, ws=ws)
    assert rc == 0
    for name in NAMES:
        assert (bufs[name][1] == 0).all() and untouched(bufs, name), name


# ---- 6: the forward ----------------------------------------------------------------------------------------------------------------------
def c_forward(c, image, patch):
    d = desc_of(c, image, patch)
    n, S, C = c["gout"].shape
    ws, wsb = workspace(d, n)
    out = torch.full((n, S, C), NAN, device=DEV).to(torch.bfloat16)
    _lib.check(_lib.lib().vllm_vit_embed_forward(ctypes.byref(d), P(c["pix"]), n, P(out), P(ws), wsb, stream()), "vllm_vit_embed_forward")
    torch.cuda.synchronize()
    return out


def intern_model(c, image, patch, layers=2, heads=2, inter=256, seed=0):
    C = c["w"].shape[0]
    cfg = InternVisionConfig(hidden_size=C, num_attention_heads=heads, intermediate_size=inter, num_hidden_layers=layers, image_size=image,
                             patch_size=patch, layer_norm_eps=VI.EPS)
    model = InternVisionModel(cfg)
    for i, lyr in enumerate(model.encoder.layers):
        lyr.load_state_dict({k: v.float() for k, v in VI.make_params(C, inter, seed=seed + i).items()})
    model = model.to(DEV).to(torch.bfloat16)
    load_embeddings(model.embeddings, c)
    return model


def load_embeddings(emb, c):
    with torch.no_grad():
        emb.patch_embedding.weight.copy_(c["w"])
        if c["b"] is not None:
            emb.patch_embedding.bias.copy_(c["b"])
        emb.class_embedding.copy_(c["cls"].view(emb.class_embedding.shape))
        pos = emb.position_embedding if isinstance(emb.position_embedding, torch.nn.Parameter) else emb.position_embedding.weight
        pos.copy_(c["pos"].view(pos.shape))


@pytest.mark.parametrize("idx", [0, 2])
def test_forward_equals_the_inference_encoder(idx):
    k = case(idx)
    c = k["c"]
    model = intern_model(c, k["image"], k["patch"], layers=1)
    hs0 = model(c["pix"], output_hidden_states=True).hidden_states[0]
    assert torch.equal(c_forward(c, k["image"], k["patch"]), hs0)
    ref = E.embeddings(c["pix"].cpu().double(), c["w"].cpu().double(), c["b"].cpu().double(), c["cls"].cpu().double(), c["pos"].cpu().double(), k["patch"])
    assert VI.rel_rms(hs0.cpu(), ref) < 2.0 ** -8


def clip_config(C, image, patch):
    from types import SimpleNamespace
    return SimpleNamespace(hidden_size=C, num_attention_heads=C // 64, intermediate_size=2 * C, num_hidden_layers=1, image_size=image,
                           patch_size=patch, layer_norm_eps=1e-5, hidden_act="quick_gelu", output_hidden_states=False, use_return_dict=True)


def test_clip_forward():
    k = case(1)
    c = k["c"]
    assert c["b"] is None
    emb = _CLIPVisionEmbeddings(clip_config(192, k["image"], k["patch"])).to(DEV).to(torch.bfloat16)
    load_embeddings(emb, c)
    direct = c_forward(c, k["image"], k["patch"])
    with torch.no_grad():
        y0 = emb(c["pix"])
    y1 = emb(c["pix"])
    assert y0.grad_fn is None and y1.grad_fn is not None
    assert torch.equal(y0, direct) and torch.equal(y1, direct)
    ref = E.embeddings(c["pix"].cpu().double(), c["w"].cpu().double(), None, c["cls"].cpu().double(), c["pos"].cpu().double(), k["patch"])
    assert VI.rel_rms(direct.cpu(), ref) < 2.0 ** -8
    # the embeddings inside the CLIP model: the encoder's hidden_states[0] is pre_layrnorm of these rows
    model = CLIPVisionModel(clip_config(192, k["image"], k["patch"])).to(DEV).to(torch.bfloat16)
    load_embeddings(model.vision_model.embeddings, c)
    ln = model.vision_model.pre_layrnorm
    hs0 = model(c["pix"], output_hidden_states=True).hidden_states[0]
    want = torch.nn.functional.layer_norm(direct.float(), (192,), ln.weight.float(), ln.bias.float(), ln.eps)
    assert VI.rel_rms(hs0, want) < 2.0 ** -8


# ---- 7: the modules under autograd -------------------------------------------------------------------------------------------------------
def intern_embeddings(k):
    c = k["c"]
    cfg = InternVisionConfig(hidden_size=c["w"].shape[0], num_attention_heads=2, intermediate_size=256, num_hidden_layers=1, image_size=k["image"],
                             patch_size=k["patch"])
    emb = InternVisionEmbeddings(cfg).to(DEV).to(torch.bfloat16)
    load_embeddings(emb, c)
    return emb


def module_params(emb):
    pos = emb.position_embedding if isinstance(emb.position_embedding, torch.nn.Parameter) else emb.position_embedding.weight
    return dict(w=emb.patch_embedding.weight, b=emb.patch_embedding.bias, cls=emb.class_embedding, pos=pos)


def run_module(emb, pix, gout):
    for p in emb.parameters():
        p.grad = None
    y = emb(pix)
    y.backward(gout)
    return y.detach(), {n: (p.grad.clone() if p is not None and p.grad is not None else None) for n, p in module_params(emb).items()}


@pytest.mark.parametrize("idx", [0, 2, 1])
def test_module_gradients_are_the_c_entry_s(idx):
    k = case(idx)
    c = k["c"]
    if c["b"] is None:
        emb = _CLIPVisionEmbeddings(clip_config(c["w"].shape[0], k["image"], k["patch"])).to(DEV).to(torch.bfloat16)
        load_embeddings(emb, c)
    else:
        emb = intern_embeddings(k)
    y, g = run_module(emb, c["pix"], c["gout"])
    assert torch.equal(y, c_forward(c, k["image"], k["patch"]))
    for name, p in module_params(emb).items():
        if p is None:
            continue
        assert g[name].shape == p.shape and g[name].dtype == torch.bfloat16
        assert torch.equal(g[name].reshape(-1), k["grads"][name].reshape(-1)), name


def test_frozen_subsets_accumulation_and_hygiene():
    k = case(0)
    c = k["c"]
    emb = intern_embeddings(k)
    full = {n: k["grads"][n].reshape(-1) for n in NAMES}
    for trainable in ("pos", "b"):
        for n, p in module_params(emb).items():
            p.requires_grad_(n == trainable)
        y, g = run_module(emb, c["pix"], c["gout"])
        assert y.shape == c["gout"].shape
        for n in NAMES:
            if n == trainable:
                assert torch.equal(g[n].reshape(-1), full[n]), n
            else:
                assert g[n] is None, n
    for p in emb.parameters():
        p.requires_grad_(False)
    y = emb(c["pix"])
    assert y.grad_fn is None and torch.equal(y, c_forward(c, k["image"], k["patch"]))
    for p in emb.parameters():
        p.requires_grad_(True)
        p.grad = None
    emb(c["pix"]).backward(c["gout"])
    emb(c["pix"]).backward(c["gout"])
    for n, p in module_params(emb).items():
        assert torch.equal(p.grad.reshape(-1), full[n] + full[n]), n
    # an in-place update between forward and backward
    y = emb(c["pix"])
    with torch.no_grad():
        emb.patch_embedding.weight.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(c["gout"])
    with pytest.raises(NotImplementedError, match="pixel_values"):
        emb(c["pix"].clone().requires_grad_())


def test_misaligned_pixels_and_side_stream():
    k = case(0)
    c = k["c"]
    emb = intern_embeddings(k)
    want = {n: k["grads"][n].reshape(-1) for n in NAMES}
    y0 = c_forward(c, k["image"], k["patch"])
    base = torch.zeros(c["pix"].numel() + 1, device=DEV, dtype=torch.bfloat16)
    pix_off = base[1:].view(c["pix"].shape)
    pix_off.copy_(c["pix"])
    assert pix_off.data_ptr() % 16 != 0
    y, g = run_module(emb, pix_off, c["gout"])
    assert torch.equal(y, y0)
    for n in NAMES:
        assert torch.equal(g[n].reshape(-1), want[n]), n
    s = torch.cuda.Stream()
    ps, gs = c["pix"].clone(), c["gout"].clone()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        y, g = run_module(emb, ps, gs)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(y, y0)
    for n in NAMES:
        assert torch.equal(g[n].reshape(-1), want[n]), n


# ---- 8: the tower from pixels ------------------------------------------------------------------------------------------------------------
HEADS, INTER, LAYERS = 2, 256, 2
EMB_KEYS = {"w": "embeddings.patch_embedding.weight", "b": "embeddings.patch_embedding.bias", "cls": "embeddings.class_embedding",
            "pos": "embeddings.position_embedding"}


def tower_autograd(c, layer_params, gout, dtype, device):
    """torch autograd of the restated embeddings + layer x LAYERS in `dtype` -> (out, {model parameter name: grad})"""
    to = lambda t: t.detach().to(device=device, dtype=dtype)
    pe = {k: to(c[k]).requires_grad_(True) for k in NAMES}
    pl = [{n: to(v).requires_grad_(True) for n, v in lp.items()} for lp in layer_params]
    x = E.embeddings(to(c["pix"]), pe["w"], pe["b"], pe["cls"], pe["pos"], 14)
    for lp in pl:
        x = VI.layer(lp, x, HEADS, VI.EPS)
    x.backward(to(gout))
    grads = {EMB_KEYS[k]: v.grad for k, v in pe.items()}
    for i, lp in enumerate(pl):
        grads.update({f"encoder.layers.{i}.{n}": v.grad for n, v in lp.items()})
    return x.detach(), grads


def tower_run(model, pix, gout):
    for p in model.parameters():
        p.grad = None
    out = model(pix).last_hidden_state
    out.backward(gout)
    return out.detach(), {n: p.grad.clone() for n, p in model.named_parameters()}


def test_tower_trains_from_pixels():
    k = case(0)
    c = k["c"]
    model = intern_model(c, 70, 14, layers=LAYERS, heads=HEADS, inter=INTER, seed=80).train()
    layer_params = [VI.make_params(128, INTER, seed=80 + i) for i in range(LAYERS)]      # (the values intern_model loaded)
    _, gout = VI.make_io(3, 26, 128, seed=8, device=DEV)
    assert any(p.requires_grad for p in model.parameters()) and torch.is_grad_enabled()
    # the default: the inference encoder, whatever the grad mode
    old = model(c["pix"], output_hidden_states=True)
    assert old.last_hidden_state.grad_fn is None and not old.last_hidden_state.requires_grad
    desc = model._build_plan()
    from visionllm_amd.vit_common import run_encoder
    with torch.no_grad():
        assert torch.equal(old.last_hidden_state, run_encoder(desc, c["pix"], LAYERS, 128, (-1,))[-1])
    model.native_training = True
    with torch.no_grad():
        assert torch.equal(model(c["pix"]).last_hidden_state, old.last_hidden_state)      # grad mode off: still the inference route
    res = model(c["pix"], output_hidden_states=True)
    assert res.last_hidden_state.grad_fn is not None and len(res.hidden_states) == LAYERS + 1
    assert all(h.requires_grad for h in res.hidden_states)
    assert torch.equal(res.hidden_states[0], old.hidden_states[0])
    assert torch.equal(res.last_hidden_state, old.last_hidden_state)      # (78 rows: the layer modules launch what the inference encoder launches)
    assert torch.equal(res.pooler_output, res.last_hidden_state[:, 0, :])
    assert model(c["pix"], return_dict=False)[0].shape == (3, 26, 128)
    y, g = tower_run(model, c["pix"], gout)
    y64, g64 = tower_autograd(c, layer_params, gout, torch.float64, "cpu")
    y16, g16 = tower_autograd(c, layer_params, gout, torch.bfloat16, DEV)
    assert set(g) == set(g64), set(g) ^ set(g64)
    bad = []
    for name, a, b, ref in [("out", y, y16, y64)] + [(n, g[n], g16[n], g64[n]) for n in sorted(g)]:
        assert a.dtype == torch.bfloat16 and a.shape == ref.shape, name
        rn, rt = VI.rel_rms(a.cpu(), ref), VI.rel_rms(b.cpu(), ref)
        print(f"tower {name:45s} native {rn:.4g}  torch bf16 {rt:.4g}  ratio {rn / rt:.3f}")
        if not rn <= 1.25 * rt:
            bad.append(f"{name}: {rn:.4g} > 1.25 x {rt:.4g}")
    assert not bad, bad
    # checkpointing off: the same bits
    model.encoder.gradient_checkpointing = False
    y2, g2 = tower_run(model, c["pix"], gout)
    assert torch.equal(y2, y)
    for n in g:
        assert torch.equal(g2[n], g[n]), n
    # pixel_embeds: the layer modules, under grad
    for p in model.parameters():
        p.grad = None
    e = old.hidden_states[0].clone().requires_grad_(True)
    out = model(pixel_embeds=e).last_hidden_state
    out.backward(gout)
    e2 = old.hidden_states[0].clone().requires_grad_(True)
    want = model.encoder(e2).last_hidden_state
    want.backward(gout)
    assert torch.equal(out, want) and torch.equal(e.grad, e2.grad)
    with torch.no_grad():
        assert torch.equal(model(pixel_embeds=old.hidden_states[0]).last_hidden_state, out)
