"""CPU: every host-only workspace-size query answers the byte counts it answered before the orchestrators shared one carver
(csrc/orchestrate.hpp).  The numbers are literals, recorded from the library as it was before that change: a layout struct that loses
or reorders a member, another rounding, or a threshold that moves shows up here without a GPU.  Where a size contains the partials
of a backward kernel (gemm_wgrad, the row-wise norm backwards) it depends on the device's compute-unit count: the literals are those
of 256 CUs -- an MI355X, and what the library assumes where no device answers."""
import ctypes

import pytest

from visionllm_amd import _lib

PTR = 1 << 20   # a 16-byte aligned non-null "pointer": the queries check the descriptors, they dereference nothing


def _fill(cls, ints, skip=()):
    """A descriptor with every pointer member set (``skip``: left null) and the scalar members from ``ints``."""
    d = cls()
    for name, ctype in cls._fields_:
        if name in ints:
            setattr(d, name, ints[name])
        elif ctype is ctypes.c_void_p and name not in skip:
            setattr(d, name, PTR)
    return d


def _bridge_desc(kind, depth, cin, cout, pixel_shuffle=0, skip_cls=0):
    d = _fill(_lib.VllmBridgeDesc, dict(kind=kind, depth=depth, in_features=cin, out_features=cout, pixel_shuffle=pixel_shuffle,
                                        skip_cls=skip_cls, ln_eps=1e-5))
    for i in range(depth):
        d.w[i] = PTR
        d.b[i] = PTR
    return d


LIN, MLP, IVL = _lib.BRIDGE_LINEAR, _lib.BRIDGE_MLP_GELU, _lib.BRIDGE_INTERNVL_MLP

# vllm_bridge_workspace_bytes(desc, n, T): (kind, depth, in, out, pixel_shuffle, n, T) -> bytes.  rows = n T (n T / 4 shuffled);
# 1024 rows is the stream-K threshold
BRIDGE_FWD = [
    ((LIN, 1, 1024, 4096, 0, 1, 1023), 0),
    ((LIN, 1, 1024, 4096, 0, 1, 1024), 83890176),
    ((LIN, 2, 1024, 4096, 0, 1, 1023), 16760832),
    ((LIN, 3, 1024, 4096, 0, 2, 512), 100667392),
    ((MLP, 1, 1024, 4096, 0, 3, 341), 0),
    ((MLP, 2, 1024, 4096, 0, 3, 341), 16760832),
    ((MLP, 2, 1024, 4096, 0, 4, 256), 100667392),
    ((MLP, 3, 1024, 4096, 0, 1, 1023), 16760832),
    ((MLP, 3, 1024, 4096, 0, 1, 1024), 100667392),
    ((IVL, 1, 4096, 4096, 0, 1, 1024), 92278784),
    ((IVL, 2, 4096, 4096, 0, 1, 1023), 25141248),
    ((IVL, 2, 4096, 4096, 0, 1, 1024), 109056000),
    ((IVL, 3, 4096, 4096, 0, 1, 1023), 25141248),
    ((IVL, 2, 12800, 4096, 1, 1, 4092), 69138432),   # pixel-shuffle: 1023 rows
    ((IVL, 2, 12800, 4096, 1, 4, 1024), 153096192),   # 1024 rows
    ((MLP, 2, 4096, 4096, 1, 5, 1024), 115347456),
    ((LIN, 1, 4096, 256, 1, 2, 16), 65536),
    ((IVL, 2, 4096, 4096, 0, 0, 1024), 0),   # no tiles
]

# vllm_bridge_backward_workspace_bytes(desc, rows, need_grad_x): (kind, depth, in, out, pixel_shuffle, rows, need_grad_x) -> bytes.
# A Linear bridge has depth 1 and the InternVL MLP depth 2; training takes no fused pixel-shuffle: -1 otherwise
BRIDGE_BWD = [
    ((LIN, 1, 1024, 4096, 0, 1023, 0), 33587200),
    ((LIN, 1, 1024, 4096, 0, 1023, 1), 41975808),
    ((LIN, 1, 1024, 4096, 0, 1024, 0), 117477376),
    ((LIN, 1, 1024, 4096, 0, 1024, 1), 125865984),
    ((LIN, 2, 1024, 4096, 0, 1024, 1), -1),
    ((LIN, 3, 1024, 4096, 0, 1024, 1), -1),
    ((MLP, 1, 1024, 4096, 0, 1023, 1), 41975808),
    ((MLP, 2, 1024, 4096, 0, 1023, 0), 75522048),
    ((MLP, 2, 1024, 4096, 0, 1023, 1), 75522048),
    ((MLP, 2, 1024, 4096, 0, 1024, 1), 159420416),
    ((MLP, 3, 1024, 4096, 0, 1023, 1), 83902464),
    ((MLP, 3, 1024, 4096, 0, 1024, 0), 167809024),
    ((MLP, 3, 1024, 4096, 0, 1024, 1), 167809024),
    ((IVL, 1, 4096, 4096, 0, 1024, 1), -1),
    ((IVL, 2, 4096, 4096, 0, 1023, 0), 67084288),
    ((IVL, 2, 4096, 4096, 0, 1023, 1), 67084288),
    ((IVL, 2, 12800, 4096, 0, 1024, 0), 275779584),
    ((IVL, 2, 12800, 4096, 0, 1024, 1), 275779584),
    ((IVL, 3, 4096, 4096, 0, 1024, 1), -1),
    ((IVL, 2, 4096, 4096, 0, 0, 1), 33587200),   # no rows
    ((IVL, 2, 4096, 4096, 1, 1024, 1), -1),   # pixel-shuffle
    ((MLP, 2, 1000, 4096, 0, 1024, 1), -1),   # in_features % 64
    ((MLP, 2, 1024, 4096, 0, -1, 1), -1),
]

# vllm_vit_layer_backward_workspace_bytes(desc, B, S): (hidden, heads, inter, qk_norm, B, S) -> bytes.  B S = 1024: stream-K threshold
LAYER_BWD = [
    ((128, 2, 256, False, 1, 1023), 3843584),
    ((128, 2, 256, False, 1, 1024), 87934976),
    ((128, 2, 256, True, 3, 341), 4629248),
    ((128, 2, 256, True, 4, 256), 88721408),
    ((128, 2, 256, False, 0, 577), 99328),
    ((128, 2, 256, True, 0, 577), 99328),
    ((3200, 25, 12800, False, 1, 1023), 160601600),
    ((3200, 25, 12800, True, 1, 1023), 180243200),
    ((3200, 25, 12800, False, 1, 1024), 244555776),
    ((3200, 25, 12800, True, 1, 1024), 264216576),
    ((3200, 25, 12800, True, 0, 1025), 81945600),
    ((3200, 25, 12800, True, 2, 1025), 347071232),
    ((128, 4, 256, False, 1, 1024), -1),   # head_dim 32
    ((128, 2, 250, False, 1, 1024), -1),   # inter % 64
    ((128, 2, 256, False, 1, 0), -1),   # S
]

# vllm_vit_embed_workspace_bytes(desc, n): (hidden, patch, image, n) -> bytes
EMBED = [
    ((128, 14, 70, 0), 84056064),
    ((128, 14, 70, 1), 84089344),
    ((128, 14, 70, 3), 84155904),
    ((3200, 14, 448, 0), 89637376),
    ((3200, 14, 448, 1), 123768576),
    ((3200, 14, 448, 3), 134597376),
    ((1024, 14, 448, 3), 115920640),
    ((1024, 14, 450, 1), -1),   # image % patch
    ((100, 14, 448, 1), -1),   # hidden % 64
    ((128, 14, 70, -1), -1),
]

# vllm_vit_workspace_bytes(desc, n): (arch, hidden, heads, inter, patch, image, kpad, n) -> bytes
CLIP, IVIT = _lib.ARCH_CLIP, _lib.ARCH_INTERNVIT
VIT = [
    ((CLIP, 1024, 16, 4096, 14, 336, 640, 1), 98881792),
    ((CLIP, 1024, 16, 4096, 14, 336, 640, 4), 143856128),
    ((IVIT, 1024, 16, 4096, 14, 448, 640, 1), 110522624),
    ((IVIT, 1024, 16, 4096, 14, 448, 640, 3), 163787264),
    ((IVIT, 3200, 25, 12800, 14, 448, 640, 1), 164134144),
    ((IVIT, 3200, 25, 12800, 14, 448, 640, 5), 485110016),
    ((CLIP, 3200, 25, 12800, 14, 70, 640, 2), 87958784),
    ((IVIT, 128, 2, 256, 14, 70, 640, 0), 83890176),
    ((IVIT, 128, 2, 256, 14, 70, 640, 7), 84603392),
    ((7, 1024, 16, 4096, 14, 448, 640, 1), -1),   # arch
    ((IVIT, 1024, 32, 4096, 14, 448, 640, 1), -1),   # head_dim 32
    ((IVIT, 1024, 16, 4096, 14, 448, 576, 1), -1),   # kpad < 3 patch^2
    ((IVIT, 1024, 16, 4096, 14, 448, 640, -1), -1),
]

# vllm_msda_layer_workspace_bytes(desc, B, Lq, S): (d_model, heads, levels, points, ref_dim, B, Lq, S) -> bytes
MSDA = [
    ((256, 8, 4, 4, 2, 2, 13294, 13294), 108904448),   # encoder self-attention: the queries are the value pyramid
    ((256, 8, 4, 4, 4, 2, 900, 13294), 32755712),   # decoder cross-attention
    ((256, 8, 3, 4, 2, 1, 1, 21), 24320),
    ((256, 8, 4, 4, 2, 0, 900, 13294), 0),
    ((250, 8, 4, 4, 2, 2, 900, 13294), -1),   # d_model % 64 (and % heads)
    ((256, 8, 4, 4, 3, 2, 900, 13294), -1),   # ref_dim
    ((256, 8, 4, 4, 2, 2, -1, 13294), -1),
]


def _bridge_fwd(kind, depth, cin, cout, ps, n, T):
    return _lib.lib().vllm_bridge_workspace_bytes(ctypes.byref(_bridge_desc(kind, depth, cin, cout, ps, skip_cls=ps)), n, T)


def _bridge_bwd(kind, depth, cin, cout, ps, rows, need_gx):
    return _lib.lib().vllm_bridge_backward_workspace_bytes(ctypes.byref(_bridge_desc(kind, depth, cin, cout, ps)), rows, need_gx)


def _layer_bwd(hidden, heads, inter, qkn, B, S):
    d = _fill(_lib.VllmVitLayerTrain, dict(hidden=hidden, heads=heads, inter=inter, eps=1e-6), skip=() if qkn else ("q_norm_w", "k_norm_w"))
    return _lib.lib().vllm_vit_layer_backward_workspace_bytes(ctypes.byref(d), B, S)


def _embed(hidden, patch, image, n):
    d = _fill(_lib.VllmVitEmbed, dict(hidden=hidden, patch=patch, image=image, pixel_is_f32=0))
    return _lib.lib().vllm_vit_embed_workspace_bytes(ctypes.byref(d), n)


def _vit(arch, hidden, heads, inter, patch, image, kpad, n):
    d = _fill(_lib.VllmVitDesc, dict(arch=arch, num_layers=0, hidden=hidden, heads=heads, inter=inter, patch=patch, image=image, kpad=kpad,
                                     act=_lib.EPI_GELU if arch != CLIP else _lib.EPI_QUICK_GELU, pixel_is_f32=0, eps=1e-6))
    return _lib.lib().vllm_vit_workspace_bytes(ctypes.byref(d), n)


def _msda(d_model, heads, levels, points, ref_dim, B, Lq, S):
    d = _fill(_lib.VllmMsdaLayerDesc, dict(d_model=d_model, n_heads=heads, n_levels=levels, n_points=points, ref_dim=ref_dim,
                                           use_4d_normalizer=0, geometry=0, reserved0=0))
    return _lib.lib().vllm_msda_layer_workspace_bytes(ctypes.byref(d), B, Lq, S)


TABLES = [("bridge_fwd", _bridge_fwd, BRIDGE_FWD), ("bridge_bwd", _bridge_bwd, BRIDGE_BWD), ("layer_bwd", _layer_bwd, LAYER_BWD),
          ("embed", _embed, EMBED), ("vit", _vit, VIT), ("msda", _msda, MSDA)]


@pytest.mark.parametrize("name,query,table", TABLES, ids=[t[0] for t in TABLES])
def test_workspace_sizes_are_the_recorded_ones(name, query, table):
    got = [(args, query(*args)) for args, _ in table]
    assert got == table


@pytest.mark.parametrize("act", [_lib.EPI_GELU, _lib.EPI_QUICK_GELU])
def test_clip_layer_sizes_are_those_of_an_internvit_layer_without_qk_norm(act):
    """One layout serves both layer families: without a QK-norm its qkn slot has no bytes, and LayerNorm's weight + bias partials are the
    size of the QK-norm's q + k partials.  So for every LAYER_BWD row without QK-norm (no rows and the refusals included)
    vllm_clip_layer_backward_workspace_bytes answers the InternViT number, whichever the activation."""
    rows = [(args, want) for args, want in LAYER_BWD if not args[3]]
    assert len(rows) == 8 and sum(want == -1 for _, want in rows) == 3
    got = []
    for (hidden, heads, inter, _, B, S), _ in rows:
        d = _fill(_lib.VllmClipLayerTrain, dict(hidden=hidden, heads=heads, inter=inter, act=act, eps=1e-5))
        got.append(_lib.lib().vllm_clip_layer_backward_workspace_bytes(ctypes.byref(d), B, S))
    assert got == [want for _, want in rows]


def test_null_descriptors_answer_minus_one():
    L = _lib.lib()
    assert L.vllm_bridge_workspace_bytes(None, 1, 1024) == -1
    assert L.vllm_bridge_backward_workspace_bytes(None, 1024, 1) == -1
    assert L.vllm_vit_layer_backward_workspace_bytes(None, 1, 1024) == -1
    assert L.vllm_vit_embed_workspace_bytes(None, 1) == -1
    assert L.vllm_vit_workspace_bytes(None, 1) == -1
    assert L.vllm_msda_layer_workspace_bytes(None, 1, 1, 1) == -1
