"""CPU: the boundary of the native query selection (include/vllm_hip.h, section f2e) -- symbols, descriptor layout, the size query, the
refusals of the entry and of its three kernels (refused calls only, fake device pointers: nothing is dereferenced, no device is touched),
and the module mirror where no GPU is needed: parameter names, a state-dict round trip, every reason ``native_selection_reasons`` has to
say no, the restated ``gen_encoder_output_proposals`` against a closed form, and the composed forward's shapes, dtypes and gathers."""
import ctypes
import dataclasses
import re
import subprocess

import pytest
import torch
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import query_selection as Q
from visionllm_amd.deformable_decoder import GroundingDinoMLPPredictionHead

import query_selection_inputs as I

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
GIB = 1 << 30
NEW = ("vllm_query_select_desc_sizeof", "vllm_query_select_workspace_bytes", "vllm_query_select_calls", "vllm_query_select_forward",
       "vllm_rowmax_dot_bf16", "vllm_topk_rows_f32", "vllm_query_select_tail_f32")
OWN_POINTERS = ("enc_output_w", "enc_output_b", "enc_output_norm_w", "enc_output_norm_b")
BOX_POINTERS = ("w0", "b0", "w1", "b1", "w2", "b2")
# the reference's parameter names for these members (OVGroundingDinoModel of modeling_ov_grounding_dino_mask_dn.py), in registration order
PARAMETER_NAMES = ["enc_output.weight", "enc_output.bias", "enc_output_norm.weight", "enc_output_norm.bias"] + \
                  [f"encoder_output_bbox_embed.layers.{i}.{n}" for i in range(3) for n in ("weight", "bias")]


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def last_error():
    return _lib.lib().vllm_last_error().decode()


def calls():
    return _lib.lib().vllm_query_select_calls()


def desc(C=256, mtl=256, L=4, eps=1e-5, box=(), **own):
    d = _lib.VllmQuerySelectDesc()
    d.d_model, d.max_text_len, d.n_levels, d.layer_norm_eps = C, mtl, L, eps
    for n in OWN_POINTERS:
        setattr(d, n, own.pop(n, PTR))
    for n in BOX_POINTERS:
        setattr(d.box_head, n, dict(box).get(n, PTR))
    assert not own, own
    return d


def query(d, B=2, S=161, Lt=9, k=30):
    return _lib.lib().vllm_query_select_workspace_bytes(ctypes.byref(d), B, S, Lt, k)


def forward(d, B=2, S=161, Lt=9, k=30, memory=PTR, pmask=PTR + GIB, text=PTR + 2 * GIB, tmask=PTR + 3 * GIB, shapes=PTR + 4 * GIB,
            lsi=PTR + 5 * GIB, idx=PTR + 6 * GIB, target=PTR + 7 * GIB, coords=PTR + 8 * GIB, ref=PTR + 9 * GIB, cls=PTR + 10 * GIB, scores=0,
            ws=PTR + 12 * GIB, ws_bytes=1 << 40):
    return _lib.lib().vllm_query_select_forward(ctypes.byref(d), vp(memory), vp(pmask), vp(text), vp(tmask), vp(shapes), vp(lsi), B, S, Lt, k,
                                                vp(idx), vp(target), vp(coords), vp(ref), vp(cls), vp(scores), vp(ws), ws_bytes, None)


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
    assert "f2e. The two-stage QUERY SELECTION" in hdr
    for n in ("vllm_query_select_forward", "vllm_rowmax_dot_bf16"):
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + n + r"\s*\(", hdr, flags=re.S), f"no 'Alignment' line directly above {n}"


def test_descriptor_mirror_has_the_library_size_and_the_header_order():
    L = _lib.lib()
    assert ctypes.sizeof(_lib.VllmQuerySelectDesc) == L.vllm_query_select_desc_sizeof()
    _lib.check_struct_layouts()
    hdr = open(_lib.HEADER).read()
    body = hdr[hdr.index("typedef struct VllmQuerySelectDesc {"):hdr.index("} VllmQuerySelectDesc;")]
    order = [re.search(r"\b" + n + r"\b", body).start() for n, _ in _lib.VllmQuerySelectDesc._fields_]
    assert order == sorted(order), "VllmQuerySelectDesc: field order differs from include/vllm_hip.h"
    assert calls() >= 0


def test_workspace_query_is_the_sum_of_its_pieces_and_refuses():
    L = _lib.lib()
    d = desc()
    a256 = lambda x: (x + 255) & ~255
    B, S, k, C, Lv = 2, 161, 30, 256, 4
    base = query(d)
    # extents, the object queries, the scores, the box head's two intermediates
    assert base == a256(B * Lv * 8) + a256(B * S * C * 2) + a256(B * S * 4) + 2 * a256(B * k * C * 2)
    assert query(d, B=3) > base and query(d, S=162) > base and query(d, k=31) > base and query(d, Lt=10) == base
    assert query(d, B=0) == 0 and query(d, k=0) == 0 and query(d, B=0, Lt=0) == 0
    for kw, word in ((dict(B=-1), "not negative"), (dict(k=-1), "not negative"), (dict(Lt=0), "Lt=0"), (dict(Lt=257), "Lt=257"), (dict(k=162), "k=162"),
                     (dict(S=4000, k=2049), "k=2049"), (dict(B=1 << 12, S=1 << 12), "2^31")):
        assert query(d, **kw) < 0 and word in last_error(), (kw, last_error())
    assert query(desc(mtl=8), Lt=9) < 0 and "max_text_len=8" in last_error()
    assert query(d, S=4000, k=2048) > 0
    assert L.vllm_query_select_workspace_bytes(None, 2, 161, 9, 30) < 0 and "null descriptor" in last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(C=0), "d_model"), (dict(C=32), "d_model"), (dict(C=96), "d_model"), (dict(C=576), "d_model"),
    (dict(mtl=0), "max_text_len"), (dict(mtl=257), "max_text_len"), (dict(L=0), "n_levels"), (dict(L=17), "n_levels"), (dict(eps=-1.0), "negative eps"),
] + [({name: 0}, "missing weights") for name in OWN_POINTERS] + [(dict(box={name: 0}), "missing weights") for name in BOX_POINTERS],
    ids=lambda v: None if isinstance(v, dict) else v.replace(" ", "_"))
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
    names = ("memory", "pmask", "text", "tmask", "shapes", "lsi", "idx", "target", "coords", "ref", "cls")
    for n in names:
        assert forward(d, **{n: 0}) == EINVAL and "null pointer" in last_error() and "workspace" not in last_error(), (n, last_error())
    base = {n: PTR + i * GIB for i, n in enumerate(names)}
    for n, off in (("memory", 8), ("text", 8), ("target", 8), ("coords", 8), ("ref", 8), ("shapes", 4), ("lsi", 4), ("idx", 4), ("cls", 2)):
        assert forward(d, **{n: base[n] + off}) == EINVAL and "query_select: misaligned memory" in last_error(), (n, last_error())
    assert forward(d, scores=PTR + 11 * GIB + 2) == EINVAL and "query_select: misaligned memory" in last_error()
    assert forward(d, shapes=base["shapes"] + 8, idx=base["idx"] + 8, cls=base["cls"] + 4, ws_bytes=0) == EINVAL and "workspace" in last_error()
    for name in OWN_POINTERS:
        assert forward(desc(**{name: PTR + 8})) == EINVAL and "misaligned weight or bias" in last_error(), name
    for name in BOX_POINTERS[:-1]:
        assert forward(desc(box={name: PTR + 8})) == EINVAL and "misaligned weight or bias" in last_error(), name
    assert forward(desc(box={"b2": PTR + 4})) == EINVAL and "misaligned weight or bias" in last_error()
    assert forward(desc(box={"b2": PTR + 8}), ws_bytes=0) == EINVAL and "workspace" in last_error()          # the four-element bias: 8 bytes do
    B, S, k, C = 2, 161, 30, 256
    for kw in (dict(target=PTR), dict(target=PTR + B * S * C * 2 - 16), dict(coords=PTR + 2 * GIB), dict(idx=PTR + GIB), dict(cls=PTR + 3 * GIB),
               dict(ref=PTR + 4 * GIB), dict(scores=PTR + 5 * GIB), dict(scores=PTR + 16)):
        assert forward(d, **kw) == EINVAL and "an output overlaps an input" in last_error(), (kw, last_error())
    for kw in (dict(coords=PTR + 7 * GIB), dict(ref=PTR + 8 * GIB + B * k * 16 - 16), dict(scores=PTR + 10 * GIB), dict(cls=PTR + 6 * GIB)):
        assert forward(d, **kw) == EINVAL and "two outputs overlap" in last_error(), (kw, last_error())
    assert forward(d, ref=PTR + 8 * GIB + B * k * 16, ws_bytes=0) == EINVAL and "workspace" in last_error()          # back to back is no overlap
    assert forward(d, target=PTR + 12 * GIB + 4096) == EINVAL and "overlaps the workspace" in last_error()
    for kw, word in ((dict(Lt=0), "Lt=0"), (dict(Lt=257), "Lt=257"), (dict(k=162), "k=162"), (dict(B=-1), "not negative"), (dict(B=1 << 12, S=1 << 12), "2^31")):
        assert forward(d, **kw) == EINVAL and word in last_error(), (kw, last_error())
    # B k == 0: nothing to do, whatever the pointers are
    assert forward(d, B=0, memory=0, target=0, ws=0, ws_bytes=0) == 0 and forward(d, k=0, idx=0, cls=0, ws=0, ws_bytes=0) == 0
    assert calls() == before          # no refused call reached a launch


def test_short_misaligned_and_null_workspaces_are_refused():
    d = desc()
    need = query(d)
    assert need > 0
    before = calls()
    base = PTR + 12 * GIB
    for w, n in ((base, need - 1), (base + 8, need), (base + 8, need + 4096), (0, need)):
        assert forward(d, ws=w, ws_bytes=n) == EINVAL
        assert "query_select: workspace" in last_error(), last_error()
    assert calls() == before


def test_the_kernels_refuse_what_they_cannot_run():
    """every refusal of the three exposed kernels is decided on the host: fake pointers, no device"""
    L = _lib.lib()

    def rowmax(q=PTR, text=PTR + GIB, tmask=PTR + 2 * GIB, B=2, S=37, Lt=5, C=64, scores=PTR + 3 * GIB):
        return L.vllm_rowmax_dot_bf16(vp(q), vp(text), vp(tmask), B, S, Lt, C, vp(scores), None)
    for C in (0, 32, 96, 576):
        assert rowmax(C=C) == EINVAL and "multiple of 64 in 64 .. 512" in last_error(), C
    for Lt in (0, 257, -1):
        assert rowmax(Lt=Lt) == EINVAL and "Lt=" in last_error(), Lt
    for kw in (dict(q=0), dict(text=0), dict(tmask=0), dict(scores=0)):
        assert rowmax(**kw) == EINVAL and "null pointer" in last_error(), kw
    for kw in (dict(q=PTR + 8), dict(text=PTR + GIB + 8), dict(scores=PTR + 3 * GIB + 2)):
        assert rowmax(**kw) == EINVAL and "misaligned operand" in last_error(), kw
    assert rowmax(scores=PTR + 16) == EINVAL and "overlaps an input" in last_error()
    assert rowmax(B=-1) == EINVAL and rowmax(S=-1) == EINVAL
    assert rowmax(B=0, q=0) == 0 and rowmax(S=0, scores=0) == 0

    def topk(scores=PTR, B=2, S=37, k=9, index=PTR + GIB):
        return L.vllm_topk_rows_f32(vp(scores), B, S, k, vp(index), None)
    for kw in (dict(k=38), dict(S=5000, k=2049)):
        assert topk(**kw) == EINVAL and "topk_rows: k=" in last_error(), kw
    for kw in (dict(scores=0), dict(index=0)):
        assert topk(**kw) == EINVAL and "null pointer" in last_error(), kw
    for kw in (dict(scores=PTR + 2), dict(index=PTR + GIB + 4)):
        assert topk(**kw) == EINVAL and "misaligned operand" in last_error(), kw
    assert topk(index=PTR + 8) == EINVAL and "overlaps scores" in last_error()
    assert topk(B=-1) == EINVAL and topk(k=-1) == EINVAL
    assert topk(B=0, scores=0) == 0 and topk(k=0, index=0) == 0

    def tail(h=PTR, ldh=64, W=PTR + GIB, b=PTR + 2 * GIB, idx=PTR + 3 * GIB, pmask=PTR + 4 * GIB, shapes=PTR + 5 * GIB, lsi=PTR + 6 * GIB, B=2, S=47,
             Lv=2, k=9, C=64, ext=PTR + 7 * GIB, coords=PTR + 8 * GIB, ref=PTR + 9 * GIB, valid=0):
        return L.vllm_query_select_tail_f32(vp(h), ldh, vp(W), vp(b), vp(idx), vp(pmask), vp(shapes), vp(lsi), B, S, Lv, k, C, vp(ext), vp(coords),
                                            vp(ref), vp(valid), None)
    for C in (0, 32, 96, 576):
        assert tail(C=C, ldh=1024) == EINVAL and "multiple of 64 in 64 .. 512" in last_error(), C
    for Lv in (0, 17):
        assert tail(Lv=Lv) == EINVAL and "L in 1 .. 16" in last_error(), Lv
    for kw in (dict(h=0), dict(W=0), dict(b=0), dict(idx=0), dict(pmask=0), dict(shapes=0), dict(lsi=0), dict(ext=0), dict(coords=0), dict(ref=0)):
        assert tail(**kw) == EINVAL and "null pointer" in last_error(), kw
    for kw in (dict(h=PTR + 8), dict(W=PTR + GIB + 8), dict(b=PTR + 2 * GIB + 4), dict(idx=PTR + 3 * GIB + 4), dict(ext=PTR + 7 * GIB + 2),
               dict(coords=PTR + 8 * GIB + 8), dict(ref=PTR + 9 * GIB + 8), dict(ldh=56), dict(ldh=68)):
        assert tail(**kw) == EINVAL and "misaligned operand" in last_error(), (kw, last_error())
    assert tail(ref=PTR + 8 * GIB + 16) == EINVAL and "outputs overlap" in last_error()
    assert tail(S=0) == EINVAL and "S=0" in last_error()
    assert tail(B=0, h=0) == 0 and tail(k=0, coords=0) == 0


# ---- the module mirror ----------------------------------------------------------------------------------------------------------------------------
def test_constructor_members_and_names():
    m = I.make_module()
    assert [n for n, _ in m.named_parameters()] == PARAMETER_NAMES
    assert isinstance(m.enc_output, nn.Linear) and isinstance(m.enc_output_norm, nn.LayerNorm)
    assert isinstance(m.encoder_output_bbox_embed, GroundingDinoMLPPredictionHead) and m.encoder_output_bbox_embed.num_layers == 3
    assert isinstance(m.encoder_output_class_embed, Q.GroundingDinoContrastiveEmbedding) and m.encoder_output_class_embed.max_text_len == I.MTL
    assert not list(m.encoder_output_class_embed.parameters()) and m.native_selection is False
    shared = GroundingDinoMLPPredictionHead(64, 64, 4, 3)
    assert Q.GroundingDinoQuerySelection(64, 8, bbox_embed=shared).encoder_output_bbox_embed is shared          # the decoder's shared head object
    from visionllm_amd import GroundingDinoQuerySelection
    assert GroundingDinoQuerySelection is Q.GroundingDinoQuerySelection


def test_state_dict_round_trip():
    a, b = I.make_module(), Q.GroundingDinoQuerySelection(I.C, I.MTL)
    sd = a.state_dict()
    assert list(sd) == PARAMETER_NAMES
    # a slice of a whole model's state-dict: other keys are the caller's to drop, these load strictly
    missing, unexpected = b.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    t = I.to(I.make_inputs(), "cpu", torch.float32)
    with torch.no_grad():
        x, y = I.call(a, t, 9), I.call(b.eval(), t, 9)
    for f in dataclasses.fields(x):
        u, v = getattr(x, f.name), getattr(y, f.name)
        assert (u is None and v is None) or torch.equal(u, v), f.name


def test_proposals_against_a_closed_form():
    m = I.make_module()
    t = I.to(I.make_inputs(), "cpu", torch.float32)
    with torch.no_grad():
        oq, prop = m.gen_encoder_output_proposals(t["memory"], ~t["mask_flatten"], t["spatial_shapes"])
    want, valid = I.closed_form_proposals(t["mask_flatten"], I.MAPS)
    assert prop.dtype == torch.float32 and prop.shape == (I.B, I.S, 4) and oq.shape == (I.B, I.S, I.C) and oq.dtype == torch.float32
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(prop), inf) and (prop[inf] > 0).all()
    assert torch.equal(inf.all(-1), inf.any(-1)) and torch.equal(inf.any(-1), ~valid | ~t["mask_flatten"])
    # the inputs' premise: padded rows, and unpadded rows with invalid proposals, in image 1 only
    assert (~t["mask_flatten"][1]).sum() > 0 and (t["mask_flatten"] & ~valid)[1].sum() == len(I.UNPADDED_OUTSIDE) and not inf[0].any()
    err = (prop.double()[~inf] - want[~inf]).abs().max().item()
    print(f"proposals: max |fp32 - closed form| {err:.3e}")
    assert err <= 2e-6          # fp32: a division, 1 - p and a log of values in (0.01, 0.99), |logit| < 4.6
    # a zero-filled row is LayerNorm(bias): every such row is the same row
    filled = inf.any(-1)
    rows = oq[filled]
    lin0 = m.enc_output_norm(m.enc_output.bias.detach())
    assert rows.shape[0] > 4 and torch.equal(rows, rows[:1].expand_as(rows)) and torch.allclose(rows[0], lin0, atol=1e-5, rtol=0)


def test_composed_forward_shapes_dtypes_and_gathers():
    m = I.make_module()
    for dtype in (torch.float32, torch.bfloat16):
        mm = I.as_bf16(m, "cpu") if dtype == torch.bfloat16 else m
        t = I.to(I.make_inputs(), "cpu", dtype)
        for k in I.KS:
            for qe in (False, True):
                with torch.no_grad():
                    o = I.call(mm, t, k, qe)
                assert o.enc_outputs_class.dtype == torch.float32 and o.enc_outputs_class.shape == (I.B, I.S, I.MTL)          # torch.full's dtype
                assert o.enc_outputs_coord_logits.dtype == torch.float32 and o.enc_outputs_coord_logits.shape == (I.B, I.S, 4)
                assert o.object_query_embedding.dtype == dtype and o.object_query_embedding.shape == (I.B, I.S, I.C)
                assert o.topk_proposals.dtype == torch.int64 and o.topk_proposals.shape == (I.B, k)
                assert o.target.dtype == dtype and o.target.shape == (I.B, k, I.C)
                assert o.reference_points is o.init_reference_points and o.reference_points.shape == (I.B, k, 4)
                idx = o.topk_proposals
                assert torch.equal(o.enc_topk_class_logits, torch.gather(o.enc_outputs_class, 1, idx[..., None].expand(-1, -1, I.MTL)))
                assert torch.equal(o.enc_topk_coords_logits, torch.gather(o.enc_outputs_coord_logits, 1, idx[..., None].expand(-1, -1, 4)))
                assert torch.equal(o.reference_points, o.enc_topk_coords_logits.sigmoid())
                if qe:
                    assert o.target_undetach is None and torch.equal(o.target, t["query_embeds"][:k][None].expand(I.B, -1, -1))
                else:
                    assert torch.equal(o.target, torch.gather(o.object_query_embedding, 1, idx[..., None].expand(-1, -1, I.C)))
                    assert o.target_undetach is not None and torch.equal(o.target_undetach, o.target)
                # masked tokens and the columns from Lt up hold -inf; the selection is by the row maximum
                assert torch.isinf(o.enc_outputs_class[:, :, I.LT:]).all() and torch.isinf(o.enc_outputs_class[1, :, 2]).all()
                top = o.enc_outputs_class.max(-1)[0]
                assert torch.equal(torch.gather(top, 1, idx).sort(-1, descending=True).values, top.sort(-1, descending=True).values[:, :k])
                if k == I.S:
                    assert torch.isinf(o.enc_topk_coords_logits).any() and (o.reference_points[torch.isinf(o.enc_topk_coords_logits)] == 1.0).all()


def test_every_reason_to_keep_the_composed_path():
    t32 = I.make_inputs()
    t = {k: I.fake(v) for k, v in t32.items()}
    with torch.no_grad():
        m = I.fake_module(I.make_module())
        for k in I.KS:
            assert I.reasons(m, t, k) == [] and I.reasons(m, t, k, True) == []          # the baseline: nothing to object to

        def one(why, mod=m, tt=t, k=9, **kw):
            got = I.reasons(mod, tt, k, **kw)
            assert any(why in r for r in got), (why, got)
            return got
        m.train()
        one("training mode")
        m.eval()
        one("full_outputs", full_outputs=True)
        one("parameters: bf16 on the GPU", mod=I.as_bf16(I.make_module(), "cpu"))                      # bf16, on the CPU
        f32 = I.fake_module(I.make_module()).float()
        one("parameters: bf16 on the GPU", mod=f32)
        one("vision_features / text_features: bf16 CUDA", tt=dict(t, memory=t32["memory"]))          # on the CPU
        one("vision_features / text_features: bf16 CUDA", tt=dict(t, text=I.fake(t32["text"].float())))
        one("of one batch", tt=dict(t, text=I.fake(t32["text"][:1].contiguous())))
        one("of one batch", tt=dict(t, memory=I.fake(t32["memory"][..., :32].contiguous())))
        one("of one batch", tt=dict(t, memory=I.fake(t32["memory"][0])))
        one("1 <= Lt <= max_text_len", tt=dict(t, text=I.fake(t32["text"][:, :0].contiguous()), text_token_mask=I.fake(t32["text_token_mask"][:, :0])))
        long = I.fake(torch.zeros(I.B, I.MTL + 1, I.C, dtype=torch.bfloat16))
        one("1 <= Lt <= max_text_len", tt=dict(t, text=long, text_token_mask=I.fake(torch.ones(I.B, I.MTL + 1, dtype=torch.bool))))
        for k in (0, I.S + 1, -1, 2.0):
            one("num_queries: 1 .. min(S, 2048)", k=k)
        one("mask_flatten: bool [B, S]", tt=dict(t, mask_flatten=I.fake(t32["mask_flatten"][:, :40])))
        one("mask_flatten: bool [B, S]", tt=dict(t, mask_flatten=I.fake(t32["mask_flatten"].float())))
        one("mask_flatten: bool [B, S]", tt=dict(t, mask_flatten=None))
        one("text_token_mask: bool [B, Lt]", tt=dict(t, text_token_mask=I.fake(t32["text_token_mask"][:, :4])))
        one("text_token_mask: bool [B, Lt]", tt=dict(t, text_token_mask=I.fake(t32["text_token_mask"].to(torch.uint8))))
        one("spatial_shapes", tt=dict(t, spatial_shapes=torch.tensor([[5, 7], [3, 5]])))
        one("spatial_shapes", tt=dict(t, spatial_shapes=torch.tensor([5, 7, 3, 4])))
        for bad in (nn.Linear(64, 4), GroundingDinoMLPPredictionHead(64, 64, 4, 2), GroundingDinoMLPPredictionHead(64, 32, 4, 3),
                    GroundingDinoMLPPredictionHead(64, 64, 2, 3)):
            mm = I.make_module()
            mm.encoder_output_bbox_embed = bad
            one("encoder_output_bbox_embed: a three-layer head of width d_model", mod=I.fake_module(mm))
        odd = Q.GroundingDinoQuerySelection(96, I.MTL).eval()
        one("d_model a multiple of 64 in 64 .. 512", mod=I.fake_module(odd), tt=dict(t, memory=I.fake(torch.zeros(I.B, I.S, 96, dtype=torch.bfloat16)),
                                                                                     text=I.fake(torch.zeros(I.B, I.LT, 96, dtype=torch.bfloat16))))
        nobias = I.make_module()
        nobias.enc_output = nn.Linear(I.C, I.C, bias=False)
        one("without bias", mod=I.fake_module(nobias))
    one("requires_grad under grad mode")                                       # grad mode, trainable parameters
    frozen = I.fake_module(I.make_module().requires_grad_(False))
    assert I.reasons(frozen, t, 9) == []                                       # frozen: grad mode alone is no reason
    x = I.fake(t32["memory"].float().requires_grad_(True).to(torch.bfloat16))
    assert x.requires_grad
    one("requires_grad under grad mode", mod=frozen, tt=dict(t, memory=x))


def test_the_switch_is_off_by_default_and_the_cpu_never_takes_the_native_call(monkeypatch):
    assert Q.GroundingDinoQuerySelection.native_selection is False
    m = I.make_module()
    t = I.to(I.make_inputs(), "cpu", torch.float32)
    monkeypatch.setattr(Q.GroundingDinoQuerySelection, "native_selection", True)
    before = calls()
    with torch.no_grad():
        on = I.call(m, t, 9)
        monkeypatch.setattr(Q.GroundingDinoQuerySelection, "native_selection", False)
        off = I.call(m, t, 9)
    assert calls() == before and I.reasons(m, t, 9) != []
    assert on.enc_outputs_class is not None and torch.equal(on.topk_proposals, off.topk_proposals) and torch.equal(on.target, off.target)
