"""CPU: the inputs of the Grounding-DINO encoder (include/vllm_hip.h, section f2h; visionllm_amd/gdino_inputs.py) where no GPU is needed --
symbols, the tagged descriptor against the library's sizeof and the C compiler's layout, the size queries, every refusal of the six new
entries (fake pointers: a refused call dereferences no device pointer and touches no device), the mirror's constructor against the
reference's for 1, 3, 4 and 5 levels, the mirror in fp64 against tests/golden/gdino_inputs.npz (made by RUNNING the reference,
tools/gen_golden_gdino_inputs.py), every reason that keeps the composed path, and the conditions the GPU tests' inputs must show."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from visionllm_amd import _lib
from visionllm_amd import gdino_inputs as G

import gdino_inputs_inputs as I

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gdino_inputs.npz")
ENTRIES = ("vllm_gdino_inputs_forward", "vllm_groupnorm_rows_bf16", "vllm_nchw_to_rows_bf16", "vllm_im2col3x3s2_bf16",
           "vllm_pixel_mask_levels_u8", "vllm_sine_pos_embed_rows_bf16")
NEW = ENTRIES + ("vllm_gdino_inputs_desc_sizeof", "vllm_gdino_inputs_calls", "vllm_gdino_inputs_workspace_bytes",
                 "vllm_groupnorm_rows_workspace_bytes")


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def err():
    return _lib.lib().vllm_last_error().decode()


def calls():
    return _lib.lib().vllm_gdino_inputs_calls()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def desc(C=64, n_levels=4, n_maps=2, c_in=(64, 128, 128, 64), **kw):
    d = _lib.VllmGdinoInputsDesc()
    d.d_model, d.n_levels, d.n_maps = C, n_levels, n_maps
    for i in range(8):
        d.c_in[i] = c_in[i] if i < len(c_in) else 0
        d.gn_eps[i] = 1e-5
        for name in ("conv_w", "conv_b", "gn_w", "gn_b"):
            getattr(d, name)[i] = PTR + 256 * i
    d.level_embed, d.dim_t = PTR, PTR
    for k, v in kw.items():
        if isinstance(v, tuple):          # (index, value) of an array member
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


A = dict(maps=(PTR, PTR + (1 << 16)), h=(7, 4), w=(5, 3), fmt=(0, 1), mask=PTR + (2 << 16), eb=8, B=2, H=29, W=19, src=PTR + (3 << 16),
         pos=PTR + (4 << 16), om=PTR + (5 << 16), vr=PTR + (6 << 16), ws=1 << 30, ws_bytes=1 << 40)


def forward(d, **kw):
    a = dict(A, **kw)
    maps = (ctypes.c_void_p * len(a["maps"]))(*a["maps"]) if a["maps"] is not None else None
    return _lib.lib().vllm_gdino_inputs_forward(
        ctypes.byref(d) if d is not None else None, maps, ints(*a["h"]) if a["h"] else None, ints(*a["w"]) if a["w"] else None,
        ints(*a["fmt"]) if a["fmt"] else None, vp(a["mask"]), a["eb"], a["B"], a["H"], a["W"], vp(a["src"]), vp(a["pos"]), vp(a["om"]), vp(a["vr"]),
        vp(a["ws"]), a["ws_bytes"], None)


def query(d, B=2, h=(7, 4), w=(5, 3), fmt=(0, 1)):
    return _lib.lib().vllm_gdino_inputs_workspace_bytes(ctypes.byref(d) if d is not None else None, B, ints(*h), ints(*w), ints(*fmt))


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    protos = _lib.parse_header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T vllm_" in line}
    for n in NEW:
        assert n in protos and n in exported, n
    assert _lib.header_abi_version() == 2 and _lib.lib().vllm_abi_version() == 2          # additions only
    hdr = open(_lib.HEADER).read()
    assert "f2h. The INPUTS of the Grounding-DINO encoder" in hdr and "ONE DEPARTURE" in hdr and '#include "vllm_hip_gdino_inputs.h"' in hdr
    for lines in (":2080-2111", ":529-564", ":2200-2209", ":2388-2439", ":502, :2406"):
        assert lines in hdr
    for n in ENTRIES:
        assert re.search(r"/\* Alignment(?:(?!\*/).)*\*/\s*int\s+" + n + r"\s*\(", hdr, flags=re.S), f"no 'Alignment' line directly above {n}"


def test_descriptor_has_the_library_size_and_the_c_compilers_layout(tmp_path):
    L = _lib.lib()
    structs = _lib.GDINO_INPUTS_STRUCTS
    assert list(structs) == ["VllmGdinoInputsDesc"]
    assert ctypes.sizeof(_lib.VllmGdinoInputsDesc) == L.vllm_gdino_inputs_desc_sizeof()
    f = dict(_lib.VllmGdinoInputsDesc._fields_)
    assert f["conv_w"] is ctypes.c_void_p * 8 and f["c_in"] is ctypes.c_int32 * 8 and f["gn_eps"] is ctypes.c_float * 8
    assert _lib.pointer_fields(_lib.VllmGdinoInputsDesc) == ("level_embed", "dim_t")
    protos = _lib.parse_header()
    with pytest.raises(RuntimeError, match="vllm_gdino_inputs_desc_sizeof"):          # the load insists on the export
        _lib._check_struct_layouts(L, {k: v for k, v in protos.items() if k != "vllm_gdino_inputs_desc_sizeof"})
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
    assert {k: int(v) for k, v in (ln.split() for ln in out.splitlines())} == want and len(want) == 13


def test_size_queries_are_monotone_in_the_batch_and_the_map_sizes():
    L = _lib.lib()
    d = desc()
    assert query(d, B=0) == 0
    by_b = [query(d, B=b) for b in (1, 2, 3, 8)]
    by_h = [query(d, h=(h, 4)) for h in (1, 7, 8, 40)]
    by_w = [query(d, w=(5, w)) for w in (1, 3, 4, 33)]
    for sizes in (by_b, by_h, by_w):
        # (pieces are rounded up to 256 bytes: two neighbouring sizes may need the same bytes, a larger one never fewer)
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes
    assert query(d, fmt=(1, 1)) < query(d, fmt=(0, 0))   # channels-last maps need no transpose buffer
    assert query(d, B=-1) < 0 and "B=-1" in err()
    assert query(None) < 0 and "null descriptor" in err()
    assert query(d, h=(0, 4)) < 0 and "map 0 is 0 x 5" in err()
    g = lambda b, hw, c: L.vllm_groupnorm_rows_workspace_bytes(b, hw, c)
    assert g(0, 35, 64) == 0 and g(2, 0, 64) == 0
    sizes = [g(b, hw, 64) for b, hw in ((1, 1), (1, 33), (2, 33), (2, 1000), (8, 28224))]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert g(1, 35, 96) < 0 and "C=96" in err() and g(-1, 35, 64) < 0


# ---- refusals: nothing is enqueued --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [
    (dict(C=96), "d_model=96"), (dict(C=576), "d_model=576"), (dict(n_levels=0), "n_levels=0"), (dict(n_levels=9), "n_levels=9"),
    (dict(n_maps=0), "n_maps=0"), (dict(n_maps=5), "n_maps=5"), (dict(c_in=(64, 100, 100, 64)), "c_in[1]=100"), (dict(c_in=(64, 128, 64, 64)), "c_in[2]=64"),
    (dict(c_in=(64, 128, 128, 128)), "c_in[3]=128"), (dict(gn_eps=(2, -1.0)), "negative eps"), (dict(conv_w=(1, 0)), "missing weights"),
    (dict(gn_b=(3, 0)), "missing weights"), (dict(conv_b=(0, PTR + 8)), "misaligned weight or bias"), (dict(level_embed=0), "missing level_embed"),
    (dict(dim_t=0), "missing level_embed / dim_t"), (dict(dim_t=PTR + 4), "misaligned level_embed / dim_t"),
])
def test_forward_refuses_a_bad_descriptor(kw, word):
    before = calls()
    assert forward(desc(**kw)) == EINVAL and word in err(), err()
    assert query(desc(**kw)) < 0
    assert calls() == before


def test_forward_refuses_bad_operands_and_workspaces():
    d = desc()
    before = calls()
    need = query(d)
    assert need > 0
    assert forward(None) == EINVAL and "null descriptor" in err()
    assert forward(d, B=0) == 0                                          # nothing to do
    assert forward(d, B=-1) == EINVAL and "B=-1" in err()
    assert forward(d, B=70000) == EINVAL and "B=70000" in err()
    assert forward(d, B=60000, h=(30000, 4), w=(30000, 3)) == EINVAL and "2^31" in err()
    assert forward(d, B=8, h=(2000, 4), w=(2000, 3)) == EINVAL and "a GEMM operand below 2^31 bytes" in err()
    for kw, word in ((dict(h=None), "null pointer (map_h"), (dict(fmt=None), "null pointer (map_h"), (dict(fmt=(2, 0)), "map_format[0]=2"),
                     (dict(h=(7, 0)), "map 1 is 0 x 3"), (dict(w=(-5, 3)), "map 0 is 7 x -5"), (dict(eb=4), "mask_elem_bytes=4"),
                     (dict(H=0), "pixel mask 0 x 19"), (dict(W=40000), "pixel mask 29 x 40000"), (dict(mask=0), "null pointer (pixel_mask)"),
                     (dict(mask=A["mask"] + 4), "misaligned pixel_mask"), (dict(maps=None), "null pointer (maps"), (dict(src=0), "null pointer (maps"),
                     (dict(pos=0), "null pointer (maps"), (dict(om=0), "null pointer (maps"), (dict(vr=0), "null pointer (maps"),
                     (dict(maps=(PTR, 0)), "null pointer (map 1)"), (dict(maps=(PTR + 8, PTR + (1 << 16))), "misaligned map 0"),
                     (dict(src=A["src"] + 8), "misaligned out_source"), (dict(pos=A["pos"] + 2), "misaligned out_source"),
                     (dict(vr=A["vr"] + 4), "misaligned out_source"), (dict(pos=A["src"] + 64), "two outputs overlap"),
                     (dict(om=A["pos"] + 3), "two outputs overlap"), (dict(src=A["maps"][0]), "an output overlaps map 0"),
                     (dict(pos=A["maps"][1] + 32), "an output overlaps map 1"), (dict(vr=A["mask"] + 8), "an output overlaps pixel_mask"),
                     (dict(ws=0), "null workspace"), (dict(ws=A["ws"] + 8), "misaligned workspace"), (dict(ws_bytes=need - 1), "workspace too small"),
                     (dict(ws=A["src"] - 256), "workspace overlaps an operand"), (dict(ws=A["maps"][1] - 256), "workspace overlaps an operand"),
                     (dict(ws=A["mask"] - 256), "workspace overlaps an operand")):
        assert forward(d, **kw) == EINVAL and word in err(), (kw, err())
    assert forward(d, mask=A["mask"] + 1, eb=1, ws_bytes=need - 1) == EINVAL and "workspace too small" in err()   # a byte mask: element alignment
    assert calls() == before


def test_kernel_entries_refuse_what_they_cannot_run():
    L = _lib.lib()
    gn = lambda x=PTR, ldx=64, gamma=PTR, beta=PTR, eps=1e-5, B=2, HW=35, C=64, out=PTR + (1 << 16), obs=35 * 64, ldo=64, ws=PTR + (1 << 18), wsb=1 << 30: \
        L.vllm_groupnorm_rows_bf16(vp(x), ldx, vp(gamma), vp(beta), eps, B, HW, C, vp(out), obs, ldo, vp(ws), wsb, None)
    need = L.vllm_groupnorm_rows_workspace_bytes(2, 35, 64)
    for kw, word in ((dict(C=96), "C=96"), (dict(C=32), "C=32"), (dict(C=576), "C=576"), (dict(B=-1), "B=-1"), (dict(HW=-1), "HW=-1"), (dict(B=70000), "B=70000"),
                     (dict(eps=-1.0), "negative eps"), (dict(x=0), "null pointer"), (dict(gamma=0), "null pointer"), (dict(beta=0), "null pointer"),
                     (dict(out=0), "null pointer"), (dict(x=PTR + 8), "misaligned operand"), (dict(gamma=PTR + 2), "misaligned operand"),
                     (dict(out=PTR + (1 << 16) + 4), "misaligned operand"), (dict(ldx=60), "ldx=60"), (dict(ldx=32), "ldx=32"), (dict(ldo=68), "ldo=68"),
                     (dict(obs=35 * 64 + 4), "out_batch_stride=2244"), (dict(obs=34 * 64), "out_batch_stride=2176"), (dict(ws=0), "null workspace"),
                     (dict(ws=PTR + (1 << 18) + 8), "misaligned workspace"), (dict(wsb=need - 1), "workspace too small"),
                     (dict(ws=PTR + 256), "workspace overlaps an operand"), (dict(ws=PTR + (1 << 16) - 256), "workspace overlaps an operand")):
        assert gn(**kw) == EINVAL and word in err(), (kw, err())
    assert gn(B=0) == 0 and gn(HW=0) == 0
    tr = lambda src=PTR, B=2, Cin=64, HW=35, out=PTR + (1 << 16), ld=64: L.vllm_nchw_to_rows_bf16(vp(src), B, Cin, HW, vp(out), ld, None)
    for kw, word in ((dict(Cin=0), "Cin=0"), (dict(Cin=96), "Cin=96"), (dict(B=-1), "B=-1"), (dict(HW=-2), "HW=-2"), (dict(B=1 << 15, HW=1 << 16), "2^31"),
                     (dict(src=0), "null pointer"), (dict(out=0), "null pointer"), (dict(src=PTR + 2), "misaligned operand"),
                     (dict(out=PTR + (1 << 16) + 8), "misaligned operand"), (dict(ld=56), "ld_out=56"), (dict(ld=68), "ld_out=68")):
        assert tr(**kw) == EINVAL and word in err(), (kw, err())
    assert tr(B=0) == 0 and tr(HW=0) == 0
    ic = lambda src=PTR, bs=35 * 64, ld=64, B=2, Hi=7, Wi=5, Cin=64, out=PTR + (1 << 16): L.vllm_im2col3x3s2_bf16(vp(src), bs, ld, B, Hi, Wi, Cin, vp(out), None)
    for kw, word in ((dict(Cin=0), "Cin=0"), (dict(Cin=12), "Cin=12"), (dict(B=-1), "B=-1"), (dict(Hi=-1), "Hi=-1"), (dict(Wi=40000), "Wi=40000"),
                     (dict(src=0), "null pointer"), (dict(out=0), "null pointer"), (dict(src=PTR + 8), "misaligned operand"),
                     (dict(out=PTR + (1 << 16) + 2), "misaligned operand"), (dict(ld=56), "ld_src=56"), (dict(ld=68), "ld_src=68"), (dict(bs=35 * 64 + 2), "src_batch_stride=2242")):
        assert ic(**kw) == EINVAL and word in err(), (kw, err())
    assert ic(B=0) == 0 and ic(Hi=0) == 0 and ic(Wi=0) == 0
    h, w = ints(7, 4), ints(5, 3)
    pm = lambda mask=PTR, eb=8, B=2, H=29, W=19, lh=h, lw=w, L_=2, om=PTR + (1 << 16), yc=PTR + (2 << 16), xc=PTR + (3 << 16), vr=PTR + (4 << 16): \
        L.vllm_pixel_mask_levels_u8(vp(mask), eb, B, H, W, lh, lw, L_, vp(om), vp(yc), vp(xc), vp(vr), None)
    for kw, word in ((dict(L_=0), "L=0"), (dict(L_=9), "L=9"), (dict(lh=None), "null pointer (level_h"), (dict(lw=None), "null pointer (level_h"),
                     (dict(lh=ints(0, 4)), "level 0 is 0 x 5"), (dict(B=-1), "B=-1"), (dict(B=60000, lh=ints(30000, 4), lw=ints(30000, 3)), "2^31"),
                     (dict(eb=2), "mask_elem_bytes=2"), (dict(H=0), "pixel mask 0 x 19"), (dict(mask=0), "null pointer (pixel_mask)"),
                     (dict(mask=PTR + 4), "misaligned pixel_mask"), (dict(om=0), "null pointer"), (dict(yc=0), "null pointer"), (dict(xc=0), "null pointer"),
                     (dict(vr=0), "null pointer"), (dict(yc=PTR + 2), "misaligned operand"), (dict(xc=PTR + 1), "misaligned operand"),
                     (dict(vr=PTR + 4), "misaligned operand")):
        assert pm(**kw) == EINVAL and word in err(), (kw, err())
    assert pm(B=0) == 0
    sp = lambda yc=PTR, xc=PTR, lh=h, lw=w, L_=2, B=2, C=64, le=PTR, dim_t=PTR, out=PTR + (1 << 16): \
        L.vllm_sine_pos_embed_rows_bf16(vp(yc), vp(xc), lh, lw, L_, B, C, vp(le), vp(dim_t), vp(out), None)
    for kw, word in ((dict(C=96), "C=96"), (dict(C=0), "C=0"), (dict(L_=0), "L=0"), (dict(L_=9), "L=9"), (dict(lh=None), "null pointer (level_h"),
                     (dict(lw=ints(5, -3)), "level 1 is 4 x -3"), (dict(B=-1), "B=-1"), (dict(yc=0), "null pointer"), (dict(xc=0), "null pointer"),
                     (dict(le=0), "null pointer"), (dict(dim_t=0), "null pointer"), (dict(out=0), "null pointer"), (dict(yc=PTR + 2), "misaligned operand"),
                     (dict(le=PTR + 8), "misaligned operand"), (dict(dim_t=PTR + 4), "misaligned operand"), (dict(out=PTR + 8), "misaligned operand")):
        assert sp(**kw) == EINVAL and word in err(), (kw, err())
    assert sp(B=0) == 0


# ---- the mirror against the reference -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels,in_channels", [(1, (64, 128, 256)), (3, (64, 128, 256)), (4, (64, 128, 256)), (5, (64, 128, 256)), (4, (64, 128))])
def test_constructor_matches_the_reference(n_levels, in_channels):
    """:2081-2111: one 1 x 1 entry per backbone map, then 3 x 3 / stride 2 / padding 1 entries, the first on the last map's channels, the
    later ones on d_model; a single level is one 1 x 1 entry on the LAST map's channels."""
    C = 64
    m = G.GroundingDinoEncoderInputs(I.config(C, n_levels), in_channels)
    n_maps = len(in_channels) if n_levels > 1 else 1
    chain = list(in_channels) if n_levels > 1 else [in_channels[-1]]
    kinds = [(1, 1, 0)] * n_maps
    for i in range(n_levels - n_maps):
        chain.append(in_channels[-1] if i == 0 else C)
        kinds.append((3, 2, 1))
    assert len(m.input_proj_vision) == len(chain) == max(n_levels, n_maps) and m.num_backbone_outs == n_maps
    for proj, cin, (k, s, p) in zip(m.input_proj_vision, chain, kinds):
        conv, gn = proj
        assert isinstance(proj, nn.Sequential) and isinstance(conv, nn.Conv2d) and isinstance(gn, nn.GroupNorm)
        assert (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) == (cin, C, (k, k), (s, s), (p, p))
        assert (gn.num_groups, gn.num_channels, gn.affine) == (32, C, True) and conv.bias is not None
    names = [f"input_proj_vision.{i}.{j}.{n}" for i in range(len(chain)) for j in (0, 1) for n in ("weight", "bias")]
    assert sorted(m.state_dict()) == sorted(["level_embed"] + names)
    assert tuple(m.level_embed.shape) == (n_levels, C)
    pe = m.position_embedding
    assert isinstance(pe, G.GroundingDinoSinePositionEmbedding) and (pe.embedding_dim, pe.temperature, pe.normalize, pe.scale) == (
        C // 2, I.TEMPERATURE, True, 2 * np.pi)
    with pytest.raises(ValueError, match="normalize should be True"):
        G.GroundingDinoSinePositionEmbedding(32, 20, normalize=False, scale=1.0)
    with pytest.raises(ValueError, match="Not supported"):
        G.GroundingDinoEncoderInputs(I.config(C, n_levels, position_embedding_type="fourier"), in_channels)


def test_package_exports_the_module():
    import visionllm_amd
    assert visionllm_amd.GroundingDinoEncoderInputs is G.GroundingDinoEncoderInputs
    assert visionllm_amd.GroundingDinoSinePositionEmbedding is G.GroundingDinoSinePositionEmbedding
    assert G.GroundingDinoEncoderInputs.native_inputs is False


@pytest.fixture(scope="module")
def golden():
    return {k: v for k, v in np.load(GOLDEN).items()}


@pytest.fixture(scope="module")
def golden_run(golden):
    m = G.GroundingDinoEncoderInputs(I.config(), I.IN_CHANNELS).double().eval()
    m.load_state_dict({k[len("sd."):]: torch.from_numpy(v).double() for k, v in golden.items() if k.startswith("sd.")}, strict=True)
    maps = [torch.from_numpy(golden[f"map{i}"]).double() for i in range(len(I.IN_CHANNELS))]
    with torch.no_grad():
        return m, maps, m(maps, torch.from_numpy(golden["pixel_mask"]))


def test_mirror_reproduces_the_reference_run(golden, golden_run):
    _, _, out = golden_run
    for name in ("mask_flatten", "spatial_shapes", "level_start_index", "valid_ratios"):
        got, want = getattr(out, name), torch.from_numpy(golden[name])
        assert got.dtype == want.dtype and torch.equal(got, want), name
    for name in ("source_flatten", "lvl_pos_embed_flatten"):
        got, want = getattr(out, name), torch.from_numpy(golden[name])
        assert got.dtype == want.dtype == torch.float64 and got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
    assert out.spatial_shapes.tolist() == [list(s) for s in I.LEVEL_SIZES] and out.valid_ratios.dtype == torch.float32
    # the inputs the golden was made from are the shared makers' (the GPU tests draw from the same)
    assert torch.equal(torch.from_numpy(golden["pixel_mask"]), I.pixel_mask())
    assert all(torch.equal(torch.from_numpy(golden[f"map{i}"]).double(), m) for i, m in enumerate(I.make_maps()))


def test_masks_are_downsampled_for_every_level_and_dtype(golden_run):
    m, maps, out = golden_run
    for dt in (torch.bool, torch.uint8):
        with torch.no_grad():
            again = m(maps, I.pixel_mask(dt))
        assert torch.equal(again.mask_flatten, out.mask_flatten) and torch.equal(again.valid_ratios, out.valid_ratios)
        assert torch.equal(again.lvl_pos_embed_flatten, out.lvl_pos_embed_flatten)
    start = 0
    for h, w in I.LEVEL_SIZES:
        assert torch.equal(out.mask_flatten[:, start:start + h * w].view(-1, h, w), m.downsample_mask(I.pixel_mask(), (h, w)))
        start += h * w


# ---- every reason that keeps the composed path ----------------------------------------------------------------------------------------------------
def test_reasons_to_keep_the_composed_path():
    m = I.make_module(dtype=torch.float32)
    maps, pm = I.make_maps(dtype=torch.float32), I.pixel_mask()
    has = lambda word, mod=m, maps_=maps, pm_=pm: any(word in r for r in mod.native_inputs_reasons(maps_, pm_))
    with torch.no_grad():
        # (on a box without a GPU the parameters' and the maps' reasons are always there; each further one is looked for by its words)
        assert has("parameters: bf16 on the GPU") and has("feature_maps: a list of 2 bf16 CUDA tensors")
        assert not has("training mode") and not has("requires_grad") and not has("position_embedding") and not has("d_model") and not has("input_proj_vision")
        m.train()
        assert has("training mode")
        m.eval()
    assert has("requires_grad under grad mode")
    for p in m.parameters():
        p.requires_grad_(False)
    assert not has("requires_grad under grad mode")
    maps[0].requires_grad_(True)
    assert has("requires_grad under grad mode")
    maps[0].requires_grad_(False)
    with torch.no_grad():
        keep = m.position_embedding
        m.position_embedding = G.GroundingDinoLearnedPositionEmbedding(32)
        assert has("a learned or un-normalised one keeps the composed path")
        m.position_embedding = G.GroundingDinoSinePositionEmbedding(32, 20, normalize=False)
        assert has("a learned or un-normalised one keeps the composed path")
        m.position_embedding = G.GroundingDinoSinePositionEmbedding(32, 20, normalize=True, scale=1.0)
        assert has("scale 2 pi")
        m.position_embedding = G.GroundingDinoSinePositionEmbedding(16, 20, normalize=True)
        assert has("embedding_dim d_model / 2")
        m.position_embedding = keep
        for C in (96, 32, 576):
            assert has("d_model a multiple of 64 in 64 .. 512", G.GroundingDinoEncoderInputs(I.config(C, 4), I.IN_CHANNELS)), C
        assert has("input_proj_vision.1.0: Cin 100 (a multiple of 64)", G.GroundingDinoEncoderInputs(I.config(64, 4), (64, 100)))
        assert has(f"levels: 1 <= backbone maps <= levels <= {G.MAX_LEVELS}", G.GroundingDinoEncoderInputs(I.config(64, 9), I.IN_CHANNELS))

        def with_entry(i, j, mod):
            mm = I.make_module(dtype=torch.float32)
            mm.input_proj_vision[i][j] = mod
            return mm
        assert has("input_proj_vision.0.1: GroupNorm(32, d_model)", with_entry(0, 1, nn.GroupNorm(16, 64)))
        assert has("input_proj_vision.3.1: GroupNorm(32, d_model)", with_entry(3, 1, nn.LayerNorm(64)))
        assert has("input_proj_vision.1.1: GroupNorm without affine", with_entry(1, 1, nn.GroupNorm(32, 64, affine=False)))
        assert has("input_proj_vision.0.0: a conv with groups or dilation", with_entry(0, 0, nn.Conv2d(64, 64, 1, groups=2)))
        assert has("input_proj_vision.2.0: a conv with groups or dilation", with_entry(2, 0, nn.Conv2d(128, 64, 3, stride=2, padding=1, dilation=2)))
        assert has("input_proj_vision.1.0: a conv without bias", with_entry(1, 0, nn.Conv2d(128, 64, 1, bias=False)))
        assert has("input_proj_vision.2.0: a 1 x 1 Conv2d", with_entry(2, 0, nn.Conv2d(128, 64, 3, stride=1, padding=1)))
        assert has("input_proj_vision.3.0: an extra level reads", with_entry(3, 0, nn.Conv2d(128, 64, 3, stride=2, padding=1)))
        assert has("feature_maps: a list of 2", maps_=maps[:1]) and has("feature_maps: a list of 2", maps_=maps[0])


def test_map_formats_and_the_shape_reasons():
    """the tensor-side reasons, asked of the helper and of stand-in tensors on the meta device (no GPU needed: no data is touched)"""
    x = torch.empty(2, 64, 7, 5)
    assert G._map_format(x) == 0 and G._map_format(x.to(memory_format=torch.channels_last)) == 1
    assert G._map_format(torch.empty(2, 64, 7, 9)[:, :, :, 2:7]) is None and G._map_format(x.permute(0, 1, 3, 2)) is None
    assert G._map_format(torch.empty(3, 64, 7, 5)[1:]) == 0                                        # an offset view is still one of the two
    assert G._map_format(torch.empty(3, 64, 7, 5).to(memory_format=torch.channels_last)[1:]) == 1
    m = I.make_module(dtype=torch.bfloat16)
    for p in m.parameters():
        p.requires_grad_(False)

    class OnGpu(torch.Tensor):   # a CPU tensor that says it is on the GPU: the reasons read properties only
        is_cuda = True

    gpu = lambda t: t.as_subclass(OnGpu)
    maps = [gpu(t) for t in I.make_maps(dtype=torch.bfloat16)]
    pm = gpu(I.pixel_mask())
    why = lambda maps_=maps, pm_=pm: [r for r in m.native_inputs_reasons(maps_, pm_) if not r.startswith("parameters:")]
    assert why() == []
    assert why(maps_=[maps[0], gpu(torch.empty(2, 128, 4, 6, dtype=torch.bfloat16)[:, :, :, 1:4])]) == [
        "feature_maps: contiguous NCHW or torch.channels_last (offset views of either are served; arbitrary strides are not)"]
    assert why(maps_=[maps[0], gpu(maps[1].contiguous(memory_format=torch.channels_last))]) == []
    assert why(maps_=[maps[0], gpu(maps[1].float())])[0].startswith("feature_maps: a list of 2 bf16 CUDA tensors")
    for bad in (gpu(I.pixel_mask().float()), gpu(I.pixel_mask(torch.int32)), gpu(I.pixel_mask()[0]), I.pixel_mask(), None):
        assert why(pm_=bad) == ["pixel_mask: a bool / uint8 / int64 CUDA tensor [B, H, W]"]
    assert why(pm_=gpu(I.pixel_mask(torch.bool))) == [] and why(pm_=gpu(I.pixel_mask(torch.uint8))) == []
    assert why(pm_=gpu(I.pixel_mask()[:1]))[0].startswith("shapes: the mask's and every map's batch agree")
    assert why(maps_=[maps[0], gpu(torch.empty(2, 64, 4, 3, dtype=torch.bfloat16))])[0].startswith("shapes: the mask's and every map's batch agree")
    assert why(maps_=[maps[0], gpu(torch.empty(2, 128, 0, 3, dtype=torch.bfloat16))])[0].startswith("shapes:")


def test_descriptor_is_cached_per_module_and_dropped_when_a_parameter_changes():
    """built once per (module, device); rebuilt when a parameter's storage moves or its version changes (the permuted 3 x 3 weights are
    copies: an in-place update must reach them).  The descriptor is host data: a CPU module fills one without touching a device."""
    m = I.make_module(dtype=torch.bfloat16)
    cpu = torch.device("cpu")
    st = m._native_state(cpu)
    d = st["desc"]
    assert m._native_state(cpu) is st
    assert (d.d_model, d.n_levels, d.n_maps) == (I.D_MODEL, I.N_LEVELS, len(I.IN_CHANNELS)) and list(d.c_in)[:4] == [64, 128, 128, 64]
    assert d.conv_w[0] == m.input_proj_vision[0][0].weight.data_ptr() and d.gn_b[3] == m.input_proj_vision[3][1].bias.data_ptr()   # no copy
    held = {t.data_ptr(): t for t in st["keep"]}
    for i in (2, 3):          # [C, Cin, 3, 3] -> [C, 3, 3, Cin], a pure permutation in bf16
        w = m.input_proj_vision[i][0].weight
        assert d.conv_w[i] != w.data_ptr() and torch.equal(held[d.conv_w[i]], w.detach().permute(0, 2, 3, 1))
    assert held[d.dim_t].dtype == torch.float32 and torch.equal(held[d.dim_t], m.position_embedding.dim_t(cpu))
    with torch.no_grad():
        m.input_proj_vision[2][0].weight.mul_(2.0)
    st2 = m._native_state(cpu)
    assert st2 is not st
    w = m.input_proj_vision[2][0].weight
    assert torch.equal({t.data_ptr(): t for t in st2["keep"]}[st2["desc"].conv_w[2]], w.detach().permute(0, 2, 3, 1))
    m.level_embed.data = m.level_embed.data.clone()
    st3 = m._native_state(cpu)
    assert st3 is not st2 and st3["desc"].level_embed == m.level_embed.data_ptr() and m._native_state(cpu) is st3


# ---- what the GPU tests rely on ---------------------------------------------------------------------------------------------------------------------
def test_conditions_on_the_gpu_tests_inputs(golden_run):
    m, maps, out = golden_run
    start = 0
    for level, (h, w) in enumerate(I.LEVEL_SIZES):
        mask = out.mask_flatten[:, start:start + h * w].view(-1, h, w)
        assert all(int(mask[b].sum()) >= 1 for b in range(I.B)), f"level {level}: an image without a valid cell"
        start += h * w
    lvl0 = out.mask_flatten[0, :35].view(7, 5)
    inner = [(y, x) for y in range(7) for x in range(5) if not lvl0[y, x] and lvl0[:, x].sum() > lvl0[:y, x].sum() and lvl0[y].sum() > lvl0[y, :x].sum()]
    assert inner, "the hole does not survive down-sampling on level 0"          # a masked cell with valid cells behind it in its row and its column
    assert 0 < float(out.valid_ratios.min()) and float(out.valid_ratios[0, 0].max()) < 1 and float(out.valid_ratios.max()) == 1
    # the group variances of every conv output (what GroupNorm divides by) lie in 5e-4 .. 1e2: at least 50 eps, so eps = 1e-5 does not decide
    # a result (the 1 x 1 level's groups are two values each: the small end), and no group is so wide that bf16 rounding of x decides it
    with torch.no_grad():
        srcs, prev = [], None
        for i, proj in enumerate(m.input_proj_vision):
            y = proj[0](maps[i] if i < 2 else maps[-1] if i == 2 else prev)
            srcs.append(y)
            prev = proj[1](y)
        for y in srcs:
            var = y.reshape(y.shape[0], 32, -1).var(dim=2, unbiased=False)
            assert 5e-4 <= float(var.min()) and float(var.max()) <= 1e2, (float(var.min()), float(var.max()))
