"""CPU: every workspace-taking entry of the C ABI refuses a workspace it cannot use BEFORE its first HIP call.

Only refused calls are made, with fake non-null pointers (the gates look at values, they dereference nothing), so nothing touches a
device.  For every entry: ``workspace_bytes`` one less than the size query's answer, a workspace pointer off by 8 (16-byte alignment is
what include/vllm_hip.h promises; the point-sample backward promises 8 and is tried at off-by-4) with the right size, and -- where the
query is positive -- a NULL workspace.  Each must return VLLM_EINVAL with ``workspace`` in vllm_last_error().

Three entries have a contract of their own, stated in the header, and are tried against THAT:
  * vllm_gemm_bf16_sk: NULL scratch means "no stream-K" (= vllm_gemm_bf16) and a scratch shorter than vllm_gemm_scratch_bytes() only
    keeps the stream-K route from being planned (gemm256_launch plans it when the slots of every CU fit); what is refused is a scratch
    that cannot hold the 4096 flag bytes and one 262144-byte slot, and a misaligned one.
  * vllm_bridge_forward_train / vllm_vit_layer_forward_train need only the head of the backward's workspace ([sk] / [sk][xn][qkn]); the
    sizes are derived here from the layout comments of bridge_train.cpp / layer_train.cpp, not read from the library.
  * the splice takes no byte count (vllm_splice_workspace_ints int32 words, element alignment): NULL is what can be refused."""
import ctypes

import pytest

from visionllm_amd import _lib

EINVAL = -1
PTR = 1 << 20          # 256-byte aligned, non-null
F32 = ctypes.c_float


def vp(addr):
    return ctypes.c_void_p(addr) if addr else None


def _fill(cls, ints, skip=()):
    d = cls()
    for name, ctype in cls._fields_:
        if name in ints:
            setattr(d, name, ints[name])
        elif ctype is ctypes.c_void_p and name not in skip:
            setattr(d, name, PTR)
    return d


def align256(x):
    return (x + 255) & ~255


# ---- one (name, need, call(ws_addr, ws_bytes), off) per entry ------------------------------------------------------------------------------
def _entries():
    L = _lib.lib()
    p = vp(PTR)
    E = []

    def add(name, need, call, off=8, null=True):
        E.append(pytest.param(need, call, off, null, id=name))

    # GEMM with the stream-K scratch: flags + one slot is the least it takes (module docstring)
    add("gemm_bf16_sk", 4096 + 262144,
        lambda w, n: L.vllm_gemm_bf16_sk(p, p, p, p, 4096, 1024, 1024, 1024, 1024, 1024, 0, None, None, 0, 0, vp(w), n, None), null=False)
    for M, N, K in ((4096, 1024, 256), (2300, 512, 512)):
        add(f"gemm_wgrad_{M}x{N}x{K}", L.vllm_gemm_wgrad_workspace_bytes(M, N, K),
            lambda w, n, M=M, N=N, K=K: L.vllm_gemm_wgrad_bf16(p, N, p, K, M, N, K, p, K, p, vp(w), n, None))
    for rows, C in ((300, 128), (64, 12800)):
        add(f"layernorm_backward_{rows}x{C}", L.vllm_layernorm_backward_workspace_bytes(rows, C),
            lambda w, n, rows=rows, C=C: L.vllm_layernorm_backward_bf16(p, C, p, C, p, 1e-5, rows, C, p, C, p, p, vp(w), n, None))
    for G in (1, 2):
        add(f"rmsnorm_backward_G{G}", L.vllm_rmsnorm_backward_workspace_bytes(300, 128, G),
            lambda w, n, G=G: L.vllm_rmsnorm_backward_bf16(p, 3 * 128, p, 3 * 128, p, p if G == 2 else None, G, 1e-6, 300, 128, p, 3 * 128, None, 0,
                                                           p, p if G == 2 else None, vp(w), n, None))
    add("layerscale_backward", L.vllm_layerscale_backward_workspace_bytes(300, 128),
        lambda w, n: L.vllm_layerscale_backward_bf16(p, 128, p, 128, p, 300, 128, p, 128, p, vp(w), n, None))
    for dt in ("bf16", "f16"):
        fn = getattr(L, f"vllm_attn_bwd_qkvpacked_{dt}")
        add(f"attn_bwd_{dt}", L.vllm_attn_bwd_workspace_bytes(2, 65, 2, 64),
            lambda w, n, fn=fn: fn(p, p, p, p, 2, 65, 2, 64, 0.125, p, vp(w), n, None))
    for dt in ("f32", "bf16"):
        fn = getattr(L, f"vllm_point_sample_mean_backward_{dt}")
        add(f"point_sample_mean_backward_{dt}", L.vllm_point_sample_backward_workspace_bytes(2, 9, 80, 80, 500),
            lambda w, n, fn=fn: fn(p, p, p, 2, 9, 80, 80, 500, p, vp(w), n, None), off=4)
    geo = (1, 8, 8, 2, 16, 3, 3, 1, 1, 1, 1, 1, 1)
    add("dcnv3_backward_f16", L.vllm_dcnv3_backward_f16_workspace(*geo),
        lambda w, n: L.vllm_dcnv3_backward_f16(p, p, p, p, *geo, 1.0, p, p, p, vp(w), n, None))

    md = _fill(_lib.VllmMsdaLayerDesc, dict(d_model=256, n_heads=8, n_levels=3, n_points=4, ref_dim=2, use_4d_normalizer=0, geometry=0, reserved0=0))
    add("msda_layer_forward", L.vllm_msda_layer_workspace_bytes(ctypes.byref(md), 2, 50, 252),
        lambda w, n: L.vllm_msda_layer_forward(ctypes.byref(md), p, p, p, None, p, p, 2, 50, 252, p, vp(w), n, None))

    vd = _fill(_lib.VllmVitDesc, dict(arch=_lib.ARCH_INTERNVIT, num_layers=0, hidden=128, heads=2, inter=256, patch=14, image=70, kpad=640,
                                      act=_lib.EPI_GELU, pixel_is_f32=0, eps=1e-6))
    hs = (ctypes.c_void_p * 1)(PTR)
    add("vit_forward", L.vllm_vit_workspace_bytes(ctypes.byref(vd), 7),
        lambda w, n: L.vllm_vit_forward(ctypes.byref(vd), p, 7, hs, vp(w), n, None))

    def bridge(kind, depth, cin, cout, ps=0):
        d = _fill(_lib.VllmBridgeDesc, dict(kind=kind, depth=depth, in_features=cin, out_features=cout, pixel_shuffle=ps, skip_cls=ps, ln_eps=1e-5))
        for i in range(depth):
            d.w[i] = PTR
            d.b[i] = PTR
        return d

    bi = bridge(_lib.BRIDGE_INTERNVL_MLP, 2, 512, 256, ps=1)
    add("bridge_forward_internvl_shuffle", L.vllm_bridge_workspace_bytes(ctypes.byref(bi), 3, 64),
        lambda w, n: L.vllm_bridge_forward(ctypes.byref(bi), p, 3, 64, 128, p, vp(w), n, None))
    bm = bridge(_lib.BRIDGE_MLP_GELU, 2, 1024, 4096)
    add("bridge_forward_mlp_1024_rows", L.vllm_bridge_workspace_bytes(ctypes.byref(bm), 4, 256),
        lambda w, n: L.vllm_bridge_forward(ctypes.byref(bm), p, 4, 256, 1024, p, vp(w), n, None))
    two = (ctypes.c_void_p * 4)(PTR, PTR, PTR, PTR)
    for kind, depth, name in ((_lib.BRIDGE_LINEAR, 1, "linear"), (_lib.BRIDGE_MLP_GELU, 2, "mlp"), (_lib.BRIDGE_INTERNVL_MLP, 2, "internvl")):
        bt = bridge(kind, depth, 128, 256)
        for gx in (0, 1):
            if kind == _lib.BRIDGE_LINEAR and not gx:
                assert L.vllm_bridge_backward_workspace_bytes(ctypes.byref(bt), 192, gx) == 0      # (nothing to refuse: the GPU file passes NULL)
                continue
            add(f"bridge_backward_{name}_gx{gx}", L.vllm_bridge_backward_workspace_bytes(ctypes.byref(bt), 192, gx),
                lambda w, n, bt=bt, gx=gx: L.vllm_bridge_backward(ctypes.byref(bt), p, 192, p, two, two, p, p if gx else None, two, two, p, p,
                                                                  vp(w), n, None))
    # the training forward takes the head of that workspace: [sk], which exists from 1024 rows on (bridge_train.cpp: "the sk slot first")
    bt = bridge(_lib.BRIDGE_MLP_GELU, 2, 128, 256)
    add("bridge_forward_train_1024_rows", L.vllm_gemm_scratch_bytes(),
        lambda w, n: L.vllm_bridge_forward_train(ctypes.byref(bt), p, 1024, p, two, two, None, vp(w), n, None))

    sv = _fill(_lib.VllmVitLayerSaved, {})
    gr = _fill(_lib.VllmVitLayerGrads, {})
    for qkn, B, S in ((True, 2, 37), (False, 3, 65), (True, 4, 256)):
        ld = _fill(_lib.VllmVitLayerTrain, dict(hidden=128, heads=2, inter=256, eps=1e-6), skip=() if qkn else ("q_norm_w", "k_norm_w"))
        g = gr if qkn else _fill(_lib.VllmVitLayerGrads, {}, skip=("q_norm_w", "k_norm_w"))
        tag = f"{'qkn' if qkn else 'plain'}_{B}x{S}"
        add(f"vit_layer_backward_{tag}", L.vllm_vit_layer_backward_workspace_bytes(ctypes.byref(ld), B, S),
            lambda w, n, ld=ld, g=g, B=B, S=S: L.vllm_vit_layer_backward(ctypes.byref(ld), p, B, S, p, ctypes.byref(sv), p, ctypes.byref(g),
                                                                         vp(w), n, None))
        # forward: [sk][xn][qkn] (layer_train.cpp, "forward: [sk][xn][qkn]"): the stream-K scratch from 1024 rows on, norm1(x) / norm2(x1)
        # [M, C] bf16, the post-norm q, k beside v [M, 3C] bf16 with QK-norm; every piece rounded up to 256 bytes
        M, C = B * S, 128
        fwd = (align256(L.vllm_gemm_scratch_bytes()) if M >= 1024 else 0) + align256(M * C * 2) + (align256(M * 3 * C * 2) if qkn else 0)
        add(f"vit_layer_forward_train_{tag}", fwd,
            lambda w, n, ld=ld, B=B, S=S: L.vllm_vit_layer_forward_train(ctypes.byref(ld), p, B, S, p, ctypes.byref(sv), vp(w), n, None))

    for n_t, image, patch, C in ((3, 70, 14, 128), (5, 224, 14, 256)):
        ed = _fill(_lib.VllmVitEmbed, dict(hidden=C, patch=patch, image=image, pixel_is_f32=0))
        need = L.vllm_vit_embed_workspace_bytes(ctypes.byref(ed), n_t)
        add(f"vit_embed_forward_{C}", need, lambda w, n, ed=ed, n_t=n_t: L.vllm_vit_embed_forward(ctypes.byref(ed), p, n_t, p, vp(w), n, None))
        add(f"vit_embed_backward_{C}", need,
            lambda w, n, ed=ed, n_t=n_t: L.vllm_vit_embed_backward(ctypes.byref(ed), p, n_t, p, p, p, p, p, vp(w), n, None))
    return E


try:
    ENTRIES, _NOT_BUILT = _entries(), None
except (RuntimeError, OSError) as e:      # (the library is not built: the session's other files still collect, the test below says why)
    ENTRIES, _NOT_BUILT = [], e


def test_every_entry_has_its_case():
    assert _NOT_BUILT is None, _NOT_BUILT
    assert len(ENTRIES) == 33


def refused(rc):
    msg = _lib.lib().vllm_last_error().decode()
    assert rc == EINVAL and "workspace" in msg, (rc, msg)


@pytest.mark.parametrize("need,call,off,null", ENTRIES)
def test_short_misaligned_and_null_workspaces_are_refused(need, call, off, null):
    assert need > 0, "the case is meant to need a workspace"
    refused(call(PTR, need - 1))
    refused(call(PTR + off, need))
    refused(call(PTR + off, need + 4096))      # room to spare does not excuse the pointer
    if null:
        refused(call(0, need))


def test_the_training_forwards_accept_the_head_of_the_backward_workspace():
    """[sk][xn][qkn] / [sk] are smaller than the backward's total: the sizes the refusals above use are below the query's answer, so a
    caller that sizes the forward by the layout comment is served and one byte less is not (the parametrised test)."""
    L = _lib.lib()
    by_id = {e.id: e.values[0] for e in ENTRIES}
    for tag in ("qkn_2x37", "plain_3x65", "qkn_4x256"):
        assert 0 < by_id[f"vit_layer_forward_train_{tag}"] < by_id[f"vit_layer_backward_{tag}"], tag
    assert by_id["vit_layer_forward_train_qkn_2x37"] == 74 * 128 * 2 + 74 * 3 * 128 * 2
    assert by_id["bridge_forward_train_1024_rows"] == L.vllm_gemm_scratch_bytes() == 4096 + 320 * 262144


def test_entries_that_need_no_workspace_accept_null():
    """Where the query answers 0 the header accepts NULL / 0: the gate must not fire.  The calls below are refused for ANOTHER reason (a
    null operand behind the workspace gate's place), so they still launch nothing; the error must not name the workspace."""
    L = _lib.lib()
    p = vp(PTR)
    assert L.vllm_gemm_wgrad_workspace_bytes(77, 64, 640) == 0
    assert L.vllm_point_sample_backward_workspace_bytes(4, 256, 24, 24, 2304) == 0
    assert L.vllm_gemm_wgrad_bf16(p, 64, p, 640, 77, 64, 640, None, 640, None, None, 0, None) == EINVAL
    assert b"workspace" not in L.vllm_last_error()
    assert L.vllm_point_sample_mean_backward_f32(p, p, None, 4, 256, 24, 24, 2304, p, None, 0, None) == EINVAL
    assert b"workspace" not in L.vllm_last_error()


def test_splice_refuses_a_null_workspace():
    L = _lib.lib()
    p = vp(PTR)
    assert L.vllm_splice_workspace_ints(2, 40, 3) > 0
    refused(L.vllm_splice_visual_tokens_bf16(p, 9, p, None, 2, 40, 3, 8, 64, p, None, None, None))
    refused(L.vllm_splice_visual_tokens_backward_bf16(None, p, 2, 40, 3, 8, 64, p, p, None))
