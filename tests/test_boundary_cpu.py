"""The boundary between libvllm_hip.so and its callers, checked without a GPU: the ctypes structs generated from include/vllm_hip.h
against the host C compiler's layout of that header, the name tuples derived from them, and every runtime option's rule for a value
on both routes (vllm_set_option and the environment)."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from visionllm_amd import _lib

EINVAL = -1


# ---- structs ----------------------------------------------------------------------------------------------------------------------------
def test_generated_structs_have_the_c_compilers_layout(tmp_path):
    """sizeof of every struct and offsetof of every member, as the host C compiler lays out include/vllm_hip.h, against the ctypes
    classes parsed from the same header."""
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if not cc:
        pytest.skip("no host C compiler")
    structs = _lib.STRUCTS
    assert list(structs) == list(_lib.parse_structs())
    assert len(structs) == 21 and len(re.findall(r"^typedef struct", open(_lib.HEADER).read(), flags=re.M)) == 21
    lines, want = [], {}
    for name, cls in structs.items():
        assert getattr(_lib, name) is cls
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        want[name] = ctypes.sizeof(cls)
        for member, _ in cls._fields_:
            lines.append(f'printf("{name}.{member} %zu\\n", offsetof({name}, {member}));')
            want[f"{name}.{member}"] = getattr(cls, member).offset
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vllm_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    subprocess.run([cc, "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(tmp_path / "layout")], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert len(want) > 300 and got == want
    # what the callers rely on beyond the layout: arrays of layers and box heads are typed pointers, a nested struct is that struct
    assert _lib.VllmVitDesc.layers.offset and dict(_lib.VllmVitDesc._fields_)["layers"] is ctypes.POINTER(_lib.VllmVitLayer)
    assert dict(_lib.VllmDeformDecoderDesc._fields_)["box_heads"] is ctypes.POINTER(_lib.VllmBoxHead)
    assert dict(_lib.VllmQuerySelectDesc._fields_)["box_head"] is _lib.VllmBoxHead
    assert dict(_lib.VllmBridgeDesc._fields_)["w"] is ctypes.c_void_p * 4


@pytest.mark.parametrize("member", ["unsigned long n", "struct Other *p", "int (*fn)(void)", "int a : 3", "Later x", "int n[]"])
def test_a_member_the_parser_cannot_read_is_an_error_not_a_gap(tmp_path, member):
    hdr = tmp_path / "h.h"
    hdr.write_text("typedef struct Good { int a, *b, c[2]; } Good;\ntypedef struct Bad {\n    int before;\n    " + member + ";\n} Bad;\n"
                   "typedef struct Later { int a; } Later;\n")
    with pytest.raises(ValueError) as e:
        _lib.parse_structs(str(hdr))
    assert "struct Bad" in str(e.value) and member in str(e.value)


def test_layout_check_runs_once_at_load_and_covers_every_struct():
    """lib() compares each struct with its vllm_<snake_case>_sizeof(); one without an export must lie by value in one that has it."""
    L = _lib.lib()
    protos = _lib.parse_header()
    _lib._check_struct_layouts(L, protos)
    uncovered = [n for n in _lib.STRUCTS if "vllm_" + re.sub(r"(?<!^)(?=[A-Z])", "_", n[4:]).lower() + "_sizeof" not in protos]
    assert uncovered == ["VllmBoxHead"]
    with pytest.raises(RuntimeError, match="VllmBoxHead"):             # nothing contains it once VllmQuerySelectDesc is unchecked
        _lib._check_struct_layouts(L, {k: v for k, v in protos.items() if k != "vllm_query_select_desc_sizeof"})
    assert _lib.check_struct_layouts() is None and _lib.lib() is L


# ---- name tuples ------------------------------------------------------------------------------------------------------------------------
REGION_PARAMS = ("conv1_w", "conv1_b", "ln1_w", "ln1_b", "conv2_w", "conv2_b", "ln2_w", "ln2_b", "conv3_w", "conv3_b", "up_w", "up_b")
CLIP_LAYER_PARAMS = ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
CLIP_SAVED = ("qkv", "ctx", "lse", "x1", "h1", "a1")
VIT_LAYER_PARAMS = ("norm1_w", "qkv_w", "qkv_b", "q_norm_w", "k_norm_w", "proj_w", "proj_b", "ls1", "norm2_w", "fc1_w", "fc1_b", "fc2_w",
                    "fc2_b", "ls2")
VIT_SAVED = ("qkv", "ctx", "lse", "y1", "x1", "h1", "a1", "y2")
REGION_SAVED = ("a1", "y1", "pre1", "g1", "y2", "pre2", "g2", "stem", "pooled")
MSDA_LINEARS = ("value_proj", "sampling_offsets", "attention_weights", "output_proj")


def test_name_tuples_equal_the_literals_they_replaced():
    """The tuples that walk a descriptor's pointers come from the struct's own member list; these are the literals they were before."""
    from visionllm_amd import _native_call, clip_vit, intern_vit, region_encoder
    assert _lib.REGION_PARAMS == REGION_PARAMS
    assert clip_vit._LAYER_PARAMS == CLIP_LAYER_PARAMS and clip_vit._SAVED == CLIP_SAVED
    assert intern_vit._LAYER_PARAMS == VIT_LAYER_PARAMS and intern_vit._SAVED == VIT_SAVED
    assert region_encoder._NATIVE_SAVED == REGION_SAVED
    assert _native_call.MSDA_LINEARS == MSDA_LINEARS
    for got in (_lib.REGION_PARAMS, clip_vit._LAYER_PARAMS, clip_vit._SAVED, intern_vit._LAYER_PARAMS, intern_vit._SAVED,
                region_encoder._NATIVE_SAVED, _native_call.MSDA_LINEARS):
        assert type(got) is tuple


# ---- runtime options --------------------------------------------------------------------------------------------------------------------
BOOLEANS = ("msda_layer_fused", "gemm_half_tail", "gemm_res_ring", "gemm_skinny", "dcnv3_bwd_tiled", "msda_layer_value_bf16")
DEFAULTS = dict({n: 1 for n in BOOLEANS}, dcnv3_tiled=1, gemm_direct_store=2, gemm_tile_rb=-1, msda_tiled=1, gemm_variant=0,
                deform_enc_ffn_slab_rows=0, attn_variant=32)
INT_MAX = 2 ** 31 - 1
# name -> [(value given, value that then reads back)], or for a rejected value (value given, EINVAL, fragment of the message)
SET_ROUTE = dict(
    {n: [(0, 0), (1, 1), (-1, 1), (0, 0), (2, 1), (INT_MAX, 1)] for n in BOOLEANS},          # v != 0
    dcnv3_tiled=[(0, 0), (3, 3), (4, 4), (5, 1), (2, 2), (-1, 1), (1, 1)],                     # 0..4, else the default 1
    gemm_direct_store=[(0, 0), (1, 1), (3, 2), (0, 0), (-1, 2), (2, 2)],                       # 0..2, else the default 2
    gemm_tile_rb=[(0, 0), (32, 32), (33, -1), (4, 4), (-2, -1), (-1, -1)],                     # -1..32, else the default -1
    msda_tiled=[(21, 21), (-1, EINVAL, "msda_tiled must be one of 0, 1, 21 (got -1)"), (0, 0), (2, EINVAL, "msda_tiled must be one of"),
                (22, EINVAL, "(got 22)"), (1, 1)],
    gemm_variant=[(4, 4), (3, EINVAL, "gemm_variant must be 0, 1, 2 or 4"), (1, 1), (5, EINVAL, "gemm_variant must be"),
                  (-1, EINVAL, "gemm_variant must be"), (2, 2), (0, 0)],
    deform_enc_ffn_slab_rows=[(4096, 4096), (-1, EINVAL, "deform_enc_ffn_slab_rows must be >= 0 (got -1)"), (INT_MAX, INT_MAX), (0, 0)],
    attn_variant=[(2, 2), (0xffff, 0xffff), (0x10000, 0), (0x10005, 5), (-1, 0xffff), (0, 0), (32, 32)],   # & 0xffff
)


def _read(name):
    """the option's value, left as it is (a set answers the previous value; the default is valid for every option)"""
    value = _lib.set_option(name, DEFAULTS[name])
    _lib.set_option(name, value)
    return value


def test_the_thirteen_options_and_their_defaults_are_the_table_above():
    assert sorted(SET_ROUTE) == sorted(DEFAULTS) and len(DEFAULTS) == 13


@pytest.mark.parametrize("name", sorted(SET_ROUTE))
def test_set_option_applies_the_options_rule_for_a_value(name):
    """vllm_set_option answers the previous effective value and stores what the option's rule makes of the value given: a boolean
    stores v != 0, a range stores its default for a value outside it, a mask stores the low 16 bits, and the three options that
    reject answer VLLM_EINVAL, name the option in the error text and keep the value they had."""
    L = _lib.lib()
    first = _read(name)
    try:
        current = first
        for given, want, *msg in SET_ROUTE[name]:
            got = _lib.set_option(name, given)
            if msg:
                assert got == EINVAL and want == EINVAL, (name, given, got)
                assert msg[0] in L.vllm_last_error().decode(), (name, given, L.vllm_last_error())
            else:
                assert got == current, (name, given, got, current)     # the previous effective value
                current = want
            assert _read(name) == current, (name, given)
    finally:
        _lib.set_option(name, first)
    assert _read(name) == first


def test_set_option_rejects_an_unknown_name():
    L = _lib.lib()
    assert _lib.set_option("no_such_option", 1) == EINVAL
    assert "unknown option no_such_option" in L.vllm_last_error().decode()
    assert L.vllm_set_option(None, 1) == EINVAL


# The environment gives an option its first value, by the same rule; a value the rule refuses gives the default on this route.  A boolean
# and the mask refuse nothing: for them the second column is a value that the rule turns into the default (non-zero; 32 above bit 15).
ENV_ROUTE = dict(
    {n: ("0", "2") for n in BOOLEANS},
    dcnv3_tiled=("3", "5"), gemm_direct_store=("1", "3"), gemm_tile_rb=("4", "33"), msda_tiled=("21", "2"), gemm_variant=("2", "3"),
    deform_enc_ffn_slab_rows=("4096", "-1"), attn_variant=("2", str(0x10000 + 32)),
)
_CHILD = """
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
defaults = json.loads(sys.argv[2])
print(json.dumps({n: L.vllm_set_option(n.encode(), d) for n, d in defaults.items()}))
"""


@pytest.mark.parametrize("column", [0, 1], ids=["valid", "invalid"])
def test_the_environment_gives_an_option_its_first_value(column):
    """A fresh process with VLLM_<NAME> set for all 13 options: each reads back the value given where it is valid (none is the default),
    and the default where it is not."""
    assert sorted(ENV_ROUTE) == sorted(DEFAULTS)
    env = dict(os.environ, **{"VLLM_" + n.upper(): v[column] for n, v in ENV_ROUTE.items()})
    out = subprocess.run([sys.executable, "-c", _CHILD, _lib.lib_path(), json.dumps(DEFAULTS)], env=env, check=True, capture_output=True,
                         text=True, timeout=60).stdout
    valid = {n: int(v[0]) for n, v in ENV_ROUTE.items()}
    assert all(valid[n] != DEFAULTS[n] for n in valid)
    assert json.loads(out) == (valid if column == 0 else DEFAULTS)


def test_text_that_is_no_number_in_the_environment():
    """The environment's text goes through atoi, so a boolean reads a word as 0; msda_layer_value_bf16 alone looks at the first character
    and is off only for a leading '0'."""
    names = ["gemm_skinny", "msda_layer_value_bf16"]
    got = {}
    for text in ("off", "01", ""):
        env = dict(os.environ, **{"VLLM_" + n.upper(): text for n in names})
        out = subprocess.run([sys.executable, "-c", _CHILD, _lib.lib_path(), json.dumps({n: 1 for n in names})], env=env, check=True,
                             capture_output=True, text=True, timeout=60).stdout
        got[text] = json.loads(out)
    assert got == {"off": dict(gemm_skinny=0, msda_layer_value_bf16=1), "01": dict(gemm_skinny=1, msda_layer_value_bf16=0),
                   "": dict(gemm_skinny=0, msda_layer_value_bf16=1)}


def test_option_ids_and_table_rows_are_in_one_order():
    """A getter reads the slot of its OptionId (kernels.hpp) and vllm_set_option writes the slot of the row's position (runtime.cpp):
    the enum and the table must name the same options in the same order."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visionllm_amd", "csrc")
    enum = re.search(r"enum OptionId : int \{(.*?)\};", open(os.path.join(csrc, "kernels.hpp")).read(), flags=re.S).group(1)
    ids = [t.strip() for t in enum.split(",") if t.strip()]
    rows = re.findall(r'^\s*\{"([a-z_0-9]+)", "(VLLM_[A-Z_0-9]+)", ', open(os.path.join(csrc, "runtime.cpp")).read(), flags=re.M)
    assert ids[-1] == "OPT_COUNT" and [i[len("OPT_"):].lower() for i in ids[:-1]] == [name for name, _ in rows]
    assert all(env == "VLLM_" + name.upper() for name, env in rows) and len(rows) == 13
