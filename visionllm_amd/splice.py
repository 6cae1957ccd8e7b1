"""Visual-token splice: writes the projector output into the ``<im_patch>`` slots of the LLM input embeddings
(VisionLLMv2/visionllmv2/model/modeling_visionllmv2.py:582-605).  The reference does it with boolean-mask indexing
(``image_features[has_image]``, ``inputs_embeds[selected] = inputs_embeds[selected] * 0.0 + vit_embeds``: two host
synchronisations, two full copies); here the whole splice -- slot list, ``has_image``, the tiles of the samples that have an image,
the token-count rule, the row movement -- is ONE native call (``vllm_splice_visual_tokens_bf16``, round 5; rounds 1-4:
``torch.nonzero`` + a scatter kernel).  The call itself does not synchronise; with ``check=True`` (the default, and what bench.py
times) the wrapper then reads the 4-int status word back, which IS a host synchronisation -- the one the reference's error
behaviour costs.  ``check=False`` skips it and hands the status tensor to the caller instead (``return_status=True``).
Under autograd the call is an in-place node with a native backward (``vllm_splice_visual_tokens_backward_bf16``): the LLM loss reaches
the projector through this statement and nothing else.
Limit: B <= 4096 samples per call (the slot scan is one block; the torch implementation of rounds 1-4 had none).

The other four token loops (``splice_emb_tokens``, ``gather_emb_hidden_states``, ``gather_region_image_features``,
``splice_region_tokens``) keep their index bookkeeping in torch and move rows with ``vllm_copy_rows_bf16``.  By default they are
forward-only and refuse inputs that require grad; ``native_backward=True`` runs each as an autograd node whose backward is at most
two native calls (``vllm_copy_rows_masked_bf16``: grad_out with the replaced rows zeroed; ``vllm_rows_segment_sum_bf16``: rows of
grad_out summed per destination through a CSR list the forward built)."""
import ctypes

import torch

from . import _lib


def splice_visual_tokens(inputs_embeds, input_ids, imp_token_id, image_features, split_sizes=None, check=True, return_status=False):
    """inputs_embeds [B, L, C] (bf16, CUDA, modified in place and returned), input_ids [B, L],
    image_features [n_tiles, T, C] in tile order, split_sizes: tiles per sample ('anyres' list input) or None.

    Mirrors the reference's handling of samples without an image (their tiles are dropped, :585-592) and of a
    token-count mismatch (:597-603): features are repeated when the slots are a whole multiple of them; any other mismatch
    raises, as the reference's second assignment does (and nothing has been written).  ``check=False`` skips reading the status
    word back (the only host synchronisation left) -- for callers that validated the prompt on the host, or capture the step in a
    graph; a mismatch then leaves ``inputs_embeds`` untouched, and ``return_status=True`` returns ``(inputs_embeds, status)`` with
    ``status`` the DEVICE int32 tensor ``[_, n_visual_tokens, mismatch, n_slots]`` so that it can be checked later
    (``splice_status_ok(status)``) without a synchronisation now."""
    B, L, C = inputs_embeds.shape
    if not inputs_embeds.is_cuda or inputs_embeds.dtype != torch.bfloat16 or not inputs_embeds.is_contiguous():
        raise RuntimeError("splice_visual_tokens: inputs_embeds must be a contiguous bf16 CUDA tensor")
    dev = inputs_embeds.device
    ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
    if tuple(ids.shape) != (B, L):
        raise RuntimeError(f"splice_visual_tokens: input_ids {tuple(ids.shape)} does not match inputs_embeds {(B, L, C)}")
    feats = image_features.to(device=dev, dtype=torch.bfloat16)
    if feats.dim() != 3 or feats.shape[-1] != C:
        raise RuntimeError(f"splice_visual_tokens: image_features must be [n_tiles, T, {C}], got {tuple(feats.shape)}")
    n_tiles, T = int(feats.shape[0]), int(feats.shape[1])
    tps = None
    if split_sizes is not None:
        if len(split_sizes) != B:
            raise RuntimeError("splice_visual_tokens: one split size per sample required")
        tps = (ctypes.c_int32 * B)(*[int(v) for v in split_sizes])   # host array: travels as a kernel argument
    ws = torch.empty(int(_lib.lib().vllm_splice_workspace_ints(B, L, n_tiles)), dtype=torch.int32, device=dev)
    if torch.is_grad_enabled() and (inputs_embeds.requires_grad or feats.requires_grad):
        # training: the same call as an in-place autograd node (a leaf inputs_embeds that requires grad fails in torch, as the
        # reference's index assignment does)
        inputs_embeds = _SpliceVisualTokens.apply(inputs_embeds, feats, ids, int(imp_token_id), tps, ws)
    else:
        _splice_forward(inputs_embeds, feats, ids, int(imp_token_id), tps, ws)
    if check:
        _, n_vit, bad, n_sel = (int(v) for v in ws[:4].cpu())
        if bad:
            raise RuntimeError(f"splice_visual_tokens: shape mismatch: {n_sel} <im_patch> slots cannot take {n_vit} visual tokens")
    if return_status:
        return inputs_embeds, ws[:4]
    return inputs_embeds


def _splice_forward(inputs_embeds, feats, ids, imp_token_id, tps, ws):
    """The native call: ``inputs_embeds`` written in place, ``ws`` filled (header, slot list, kept tiles)."""
    B, L, C = inputs_embeds.shape
    n_tiles, T = int(feats.shape[0]), int(feats.shape[1])
    dev = inputs_embeds.device
    feats = _lib.aligned(feats)   # (the entry point needs 16-byte aligned rows: views at another storage offset are copied)
    embeds = _lib.aligned(inputs_embeds)   # written in place: a view at another storage offset is staged and copied back
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vllm_splice_visual_tokens_bf16(_lib.ptr(ids), imp_token_id, _lib.ptr(feats), tps, B, L, n_tiles, T, C,
                                                             _lib.ptr(embeds), _lib.ptr(ws), None, _lib.current_stream(dev)),
                   "vllm_splice_visual_tokens_bf16")
    if embeds is not inputs_embeds:
        inputs_embeds.copy_(embeds)


class _SpliceVisualTokens(torch.autograd.Function):
    """The splice as an in-place autograd node.  The forward is the inference call; the workspace it fills (slot list, kept tiles,
    token-count rule) is all the backward needs: ONE native call on the current stream (``vllm_splice_visual_tokens_backward_bf16``),
    no second scan of ``input_ids``, no host read.  The gradient of ``inputs_embeds`` is ``grad_out`` with the overwritten rows
    zeroed; that of ``image_features`` gathers ``grad_out`` at the slots (summed in fp32 where the tokens were repeated), zero for
    the tiles of samples without an image.  A gradient nobody needs is not computed (NULL: no traffic).  The node returns only the
    embeddings (torch does not allow an in-place node on a view to have several outputs): the workspace, and with it the status
    word, is the caller's tensor."""

    @staticmethod
    def forward(ctx, inputs_embeds, feats, ids, imp_token_id, tps, ws):
        _splice_forward(inputs_embeds, feats, ids, imp_token_id, tps, ws)
        ctx.mark_dirty(inputs_embeds)
        ctx.save_for_backward(ws)
        ctx.feats_shape = tuple(feats.shape)
        return inputs_embeds

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (ws,) = ctx.saved_tensors
        n_tiles, T, C = ctx.feats_shape
        B, L = grad_out.shape[0], grad_out.shape[1]
        dev = grad_out.device
        g = _lib.aligned(grad_out)
        g_embeds = torch.empty_like(g) if ctx.needs_input_grad[0] else None          # (both are written completely by the call)
        g_feats = torch.empty(ctx.feats_shape, dtype=g.dtype, device=dev) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().vllm_splice_visual_tokens_backward_bf16(_lib.ptr(ws), _lib.ptr(g), B, L, n_tiles, T, C, _lib.ptr(g_embeds),
                                                                          _lib.ptr(g_feats), _lib.current_stream(dev)),
                       "vllm_splice_visual_tokens_backward_bf16")
        return g_embeds, g_feats, None, None, None, None


def splice_status_ok(status):
    """Deferred form of splice_visual_tokens' check: reads a status tensor returned with ``return_status=True`` (synchronises) and
    raises the reference's shape-mismatch error if that splice wrote nothing."""
    _, n_vit, bad, n_sel = (int(v) for v in status.cpu())
    if bad:
        raise RuntimeError(f"splice_visual_tokens: shape mismatch: {n_sel} <im_patch> slots cannot take {n_vit} visual tokens")
    return True


# ---- the other per-sample token loops around the LLM: index bookkeeping in torch, row movement
# ---- by ONE native kernel (vllm_copy_rows_bf16: dst[dst_idx[i]] = src[src_idx[i]]) ------------------------------------------
def _copy_rows(src, src_idx, dst, dst_idx, n):
    """dst / src: contiguous bf16 CUDA tensors viewed as rows of C; indices: int64 CUDA tensors or None (identity)."""
    C = src.shape[-1]
    if not (src.is_cuda and dst.is_cuda and src.dtype == torch.bfloat16 and dst.dtype == torch.bfloat16 and
            src.is_contiguous() and dst.is_contiguous() and dst.shape[-1] == C):
        raise RuntimeError("copy_rows: contiguous bf16 CUDA tensors with equal row length required")
    if n == 0:
        return dst
    si = None if src_idx is None else src_idx.to(torch.int64).contiguous()
    di = None if dst_idx is None else dst_idx.to(torch.int64).contiguous()
    # the entry point needs 16-byte aligned rows: a source view at another storage offset is copied, a destination one is staged
    # and copied back
    src, out = _lib.aligned(src), _lib.aligned(dst)
    with torch.cuda.device(dst.device):
        _lib.check(_lib.lib().vllm_copy_rows_bf16(_lib.ptr(src), _lib.ptr(si), _lib.ptr(out), _lib.ptr(di), int(n), C,
                                                  src.numel() // C, out.numel() // C, _lib.current_stream(dst.device)),
                   "vllm_copy_rows_bf16")
    if out is not dst:
        dst.copy_(out)
    return dst


def _wants_grad(native_backward, *tensors):
    """Whether a token loop called with ``native_backward`` runs as an autograd node: grad mode on and an input that requires grad."""
    return bool(native_backward) and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _segments(keys, rows, n_segments):
    """CSR form of 'destination row ``keys[i]`` receives source row ``rows[i]``' for ``vllm_rows_segment_sum_bf16``: (seg_ptr
    [n_segments + 1], src_idx [len(keys)]), both int64.  The terms of one destination keep the order they have in ``keys`` / ``rows``
    (stable sort), which fixes the order of the fp32 additions.  Pure torch, on the tensors' device; keys lie in [0, n_segments)."""
    keys = keys.to(torch.int64).reshape(-1)
    seg_ptr = torch.zeros(n_segments + 1, dtype=torch.int64, device=keys.device)
    seg_ptr[1:] = torch.bincount(keys, minlength=n_segments).cumsum(0)
    return seg_ptr, rows.to(torch.int64).reshape(-1)[torch.argsort(keys, stable=True)].contiguous()


def _segment_sum(src, seg_ptr, src_idx, dst_rows):
    """-> [dst_rows, C] bf16: row d is the fp32 sum of src[src_idx[seg_ptr[d] : seg_ptr[d + 1]]], rounded once; every row is written."""
    src = _lib.aligned(src)
    C = src.shape[-1]
    out = torch.empty((dst_rows, C), dtype=torch.bfloat16, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().vllm_rows_segment_sum_bf16(_lib.ptr(src), src.numel() // C, _lib.ptr(seg_ptr), _lib.ptr(src_idx),
                                                         src_idx.numel(), _lib.ptr(out), dst_rows, C, _lib.current_stream(src.device)),
                   "vllm_rows_segment_sum_bf16")
    return out


def _copy_rows_masked(src, zero_row):
    """-> src (aligned bf16 [..., C]) with the rows flagged in ``zero_row`` (uint8, one per row) stored as zeros."""
    C = src.shape[-1]
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().vllm_copy_rows_masked_bf16(_lib.ptr(src), _lib.ptr(zero_row), _lib.ptr(out), src.numel() // C, C,
                                                         _lib.current_stream(src.device)),
                   "vllm_copy_rows_masked_bf16")
    return out


def _emb_block_rows(pos, L, n_rows):
    """Tool tokens at ``pos`` [n, 2] (batch, position) -> (dst: the flattened rows behind each of them, src: the table row each takes)."""
    offs = torch.arange(1, n_rows + 1, device=pos.device)
    dst = ((pos[:, 0] * L + pos[:, 1])[:, None] + offs[None, :]).reshape(-1)             # flattened target rows
    src = offs.sub(1).repeat(pos.shape[0])                                               # table rows, repeated per tool token
    return dst, src


def _emb_owner_map(n_positions, writes):
    """Which global table row ends up at each flattened position: int32 [n_positions], -1 = not replaced.  ``writes``: (dst, src,
    base) per tool in the order of application, ``base`` the tool's table's first row in the concatenation of the distinct tables.  A
    later tool overwrites an earlier one -- the last-writer rule of the reference's sequential torch.cat.  Pure torch."""
    dev = writes[0][0].device if writes else None
    owner = torch.full((n_positions,), -1, dtype=torch.int32, device=dev)
    for dst, src, base in writes:
        owner[dst] = (src + base).to(torch.int32)
    return owner


def _emb_segments(owner, n_table_rows):
    """owner map -> (zero_row uint8 [n_positions], seg_ptr, src_idx): the rows the splice replaced, and per global table row the
    positions it was written to, ascending."""
    replaced = torch.nonzero(owner >= 0, as_tuple=False).reshape(-1)
    seg_ptr, src_idx = _segments(owner[replaced], replaced, n_table_rows)
    return (owner >= 0).to(torch.uint8), seg_ptr, src_idx


def splice_emb_tokens(input_ids, inputs_embeds, tool_tables, emb_token_id, num_embs, num_embs_gen=None, gen_tools=(),
                      native_backward=False):
    """[EMB] splice (modeling_visionllmv2.py:425-527), the form in which the [EMB] tokens are already present in
    ``input_ids`` (gap_len = num_embs: a prompt that carries them): behind every tool token the next ``num_embs`` rows of
    ``inputs_embeds`` are REPLACED by that tool's learned query table and the ids by the [EMB] id range.

    ``tool_tables``: ordered ``{tool_token_id: table [num_embs, C]}`` in the reference's order of application (det, seg,
    grd -> emb_embeddings_det; pose -> emb_embeddings_pose; gen -> emb_embeddings_gen; edit -> emb_embeddings_edit); tool ids
    listed in ``gen_tools`` use ``num_embs_gen`` rows and the single id ``emb_token_id`` (:436).  Returns
    (input_ids, inputs_embeds): ids as a new tensor, embeddings modified IN PLACE.  A table that would run past the end of
    the sequence raises (the reference's torch.stack of unequal lengths does).

    By default forward-only: raises when an input requires grad.  ``native_backward=True``: when one does, the splice is an in-place
    autograd node (the query tables are trained through this statement and nothing else): the embeddings' gradient is grad_out with the
    replaced rows zeroed, a table row's gradient sums grad_out over the positions that ended up holding it (a later tool overwrites an
    earlier one), tables that are the same tensor object get ONE gradient.  Two blocks of the same tool that overlap (a racing
    duplicate write in the forward) raise on that path, and all checks are made before anything is written."""
    B, L, C = inputs_embeds.shape
    if _wants_grad(native_backward, inputs_embeds, *tool_tables.values()):
        return _splice_emb_tokens_train(input_ids, inputs_embeds, tool_tables, emb_token_id, num_embs, num_embs_gen, gen_tools)
    if not native_backward:
        _no_grad_path("splice_emb_tokens", inputs_embeds, *tool_tables.values())
    ids = input_ids.clone()
    flat = inputs_embeds.view(B * L, C)
    for tool_id, table in tool_tables.items():
        n_rows = num_embs_gen if tool_id in gen_tools else num_embs
        if table.shape[0] != n_rows:
            raise RuntimeError(f"splice_emb_tokens: table of tool {tool_id} has {table.shape[0]} rows, expected {n_rows}")
        pos = torch.nonzero(input_ids == tool_id, as_tuple=False)            # [n, 2] (batch, position)
        if pos.numel() == 0:
            continue
        if int((pos[:, 1] + n_rows).max()) >= L:
            raise RuntimeError("splice_emb_tokens: [EMB] block runs past the end of the sequence")
        dst, src = _emb_block_rows(pos, L, n_rows)
        _copy_rows(table.detach().to(inputs_embeds.dtype).contiguous(), src, flat, dst, dst.numel())
        ids.view(-1)[dst] = _emb_ids(ids, emb_token_id, n_rows, tool_id in gen_tools).repeat(pos.shape[0])
    return ids, inputs_embeds


def _emb_ids(ids, emb_token_id, n_rows, gen):
    return (torch.full((n_rows,), emb_token_id, device=ids.device, dtype=ids.dtype) if gen else
            torch.arange(emb_token_id, emb_token_id + n_rows, device=ids.device, dtype=ids.dtype))


def _splice_emb_tokens_train(input_ids, inputs_embeds, tool_tables, emb_token_id, num_embs, num_embs_gen, gen_tools):
    """The training path of splice_emb_tokens: the same row copies in the same order, inside one in-place node."""
    B, L, C = inputs_embeds.shape
    ids = input_ids.clone()
    tables, bases, writes, n_table_rows = [], [], [], 0        # distinct tables (by object) and their first global row
    for tool_id, table in tool_tables.items():
        n_rows = num_embs_gen if tool_id in gen_tools else num_embs
        if table.shape[0] != n_rows:
            raise RuntimeError(f"splice_emb_tokens: table of tool {tool_id} has {table.shape[0]} rows, expected {n_rows}")
        ti = next((i for i, t in enumerate(tables) if t is table), None)
        if ti is None:
            ti = len(tables)
            tables.append(table)
            bases.append(n_table_rows)
            n_table_rows += n_rows
        pos = torch.nonzero(input_ids == tool_id, as_tuple=False)
        if pos.numel() == 0:
            continue
        lin = pos[:, 0] * L + pos[:, 1]                                      # ascending (nonzero lists row-major)
        gap = (lin[1:] - lin[:-1]).min() if lin.numel() > 1 else lin.new_tensor(n_rows)
        end, gap = torch.stack([(pos[:, 1] + n_rows).max(), gap]).tolist()   # the ONE host read per tool
        if end >= L:
            raise RuntimeError("splice_emb_tokens: [EMB] block runs past the end of the sequence")
        if gap < n_rows:
            raise RuntimeError(f"splice_emb_tokens: two tool tokens {tool_id} are closer than their {n_rows} [EMB] rows: the blocks "
                               "overlap, which has no defined gradient")
        dst, src = _emb_block_rows(pos, L, n_rows)
        writes.append((dst, src, bases[ti], ti))
        ids.view(-1)[dst] = _emb_ids(ids, emb_token_id, n_rows, tool_id in gen_tools).repeat(pos.shape[0])
    if not writes:
        return ids, inputs_embeds
    owner = _emb_owner_map(B * L, [w[:3] for w in writes])
    zero_row, seg_ptr, src_idx = _emb_segments(owner, n_table_rows)
    out = _SpliceEmbTokens.apply(inputs_embeds, [(w[3], w[1], w[0]) for w in writes], zero_row, seg_ptr, src_idx, bases, *tables)
    return ids, out


class _SpliceEmbTokens(torch.autograd.Function):
    """The [EMB] splice as an in-place autograd node.  Forward: the row copies of the plain path, tool by tool.  Backward, from the
    node's own tensors (no host read, no second scan of input_ids): the masked copy for the embeddings, ONE segment sum over the rows
    of all distinct tables for the tables, sliced per table and cast to the table's dtype."""

    @staticmethod
    def forward(ctx, inputs_embeds, plan, zero_row, seg_ptr, src_idx, bases, *tables):
        B, L, C = inputs_embeds.shape
        flat = inputs_embeds.view(B * L, C)
        for ti, src, dst in plan:
            _copy_rows(tables[ti].detach().to(inputs_embeds.dtype).contiguous(), src, flat, dst, dst.numel())
        ctx.mark_dirty(inputs_embeds)
        ctx.save_for_backward(zero_row, seg_ptr, src_idx)
        ctx.tables = [(b, tuple(t.shape), t.dtype) for b, t in zip(bases, tables)]
        return inputs_embeds

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        zero_row, seg_ptr, src_idx = ctx.saved_tensors
        C = grad_out.shape[-1]
        g = _lib.aligned(grad_out)
        g_embeds = _copy_rows_masked(g, zero_row) if ctx.needs_input_grad[0] else None
        g_tables = [None] * len(ctx.tables)
        if any(ctx.needs_input_grad[6:]):
            all_rows = _segment_sum(g.view(-1, C), seg_ptr, src_idx, seg_ptr.numel() - 1)
            g_tables = [all_rows[b:b + shape[0]].to(dtype).reshape(shape) if need else None
                        for (b, shape, dtype), need in zip(ctx.tables, ctx.needs_input_grad[6:])]
        return (g_embeds, None, None, None, None, None, *g_tables)


def gather_emb_hidden_states(hidden_states, input_ids, emb_token_id, num_embs, native_backward=False):
    """[EMB] hidden states -> the det head's text_query (modeling_visionllmv2.py:775-787): returns
    (text_query [B, max_patches, num_embs, C] zero padded, text_query_masks [B, max_patches] bool), or (None, None) when no
    [EMB] token is present.  The reference loops over the batch; here the k-th selected token of sample b goes to row
    b * max_patches * num_embs + k in one native row copy (one host read of the patch counts, as the reference's .max()).
    By default forward-only; ``native_backward=True`` makes text_query an autograd node when ``hidden_states`` requires grad (the det /
    pose head losses reach the LLM through it): a kept [EMB] row takes its text_query row's gradient, every other row is zero."""
    B, L, C = hidden_states.shape
    if not native_backward:
        _no_grad_path("gather_emb_hidden_states", hidden_states)
    sel = (input_ids >= emb_token_id) & (input_ids <= emb_token_id + num_embs - 1)
    counts = sel.sum(-1)
    total = int(counts.sum())
    if total == 0:
        return None, None
    num_patches = counts // num_embs
    max_p = int(num_patches.max())
    out_shape = (B, max_p, num_embs, C)
    masks = torch.arange(max_p, device=hidden_states.device)[None, :] < num_patches[:, None]
    if max_p == 0:
        return torch.zeros(out_shape, dtype=hidden_states.dtype, device=hidden_states.device), masks
    rank = sel.cumsum(-1) - 1                                                   # position of a selected token within its sample
    keep = sel & (rank < (num_patches * num_embs)[:, None])                     # (the reference's reshape(-1, num_embs, C) needs whole patches)
    # a sample with 0 < count < num_embs is SKIPPED by the reference (num_patches == 0, :783-786); one with whole patches
    # plus a remainder fails its reshape(-1, num_embs, C)
    if bool(((counts % num_embs != 0) & (num_patches > 0)).any()):
        raise RuntimeError("gather_emb_hidden_states: a sample's [EMB] tokens are not a whole number of patches")
    src = torch.nonzero(keep.reshape(-1), as_tuple=False).reshape(-1)
    b_of = src // L
    dst = b_of * (max_p * num_embs) + rank.reshape(-1)[src]
    if _wants_grad(native_backward, hidden_states):
        # backward: row src[i] of grad_hidden_states is row dst[i] of grad_text_query -- segments of one term, every other row empty
        seg_ptr, src_idx = _segments(src, dst, B * L)
        return _GatherEmbHiddenStates.apply(hidden_states, src, dst, out_shape, seg_ptr, src_idx), masks
    return _gather_emb_rows(hidden_states, src, dst, out_shape), masks


def _gather_emb_rows(hidden_states, src, dst, out_shape):
    B, L, C = hidden_states.shape
    out = torch.zeros(out_shape, dtype=hidden_states.dtype, device=hidden_states.device)
    _copy_rows(hidden_states.contiguous().view(B * L, C), src, out.view(-1, C), dst, src.numel())
    return out


class _GatherEmbHiddenStates(torch.autograd.Function):
    """text_query as an autograd node: the forward is the plain path's row copy, the backward ONE segment sum that writes every row of
    grad_hidden_states (no zero-fill); the gradient arriving at the zero-padded patches is ignored."""

    @staticmethod
    def forward(ctx, hidden_states, src, dst, out_shape, seg_ptr, src_idx):
        ctx.save_for_backward(seg_ptr, src_idx)
        ctx.in_shape = tuple(hidden_states.shape)
        return _gather_emb_rows(hidden_states.detach(), src, dst, out_shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        seg_ptr, src_idx = ctx.saved_tensors
        B, L, C = ctx.in_shape
        g = _lib.aligned(grad_out)
        return _segment_sum(g.view(-1, C), seg_ptr, src_idx, B * L).view(B, L, C), None, None, None, None, None


def _no_grad_path(what, *tensors):
    """The default (``native_backward=False``) path of the four token loops is the bare row mover: refuse to cut a gradient silently (the reference trains emb_embeddings_*
    through the [EMB] splice, back-propagates the det-head loss through the [EMB] hidden states into the LLM
    (modeling_visionllmv2.py:775-787) and the region features into the region encoder)."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what}: forward-only (inference / prefill) -- an input requires grad; run it under "
                           "torch.no_grad() or keep the reference's torch indexing for training")


def region_tile_index(split_sizes, num_regions, num_splits=None, n_images=None):
    """Which tile (row of the concatenated tile batch) feeds each region, as a Python list -- the index arithmetic of the
    reference's three input conventions (modeling_visionllmv2.py:626-676):
      * 'anyres' (``split_sizes``: tiles per sample, ``num_splits`` None): the LAST tile of the sample (the global image),
        once per region of the sample;
      * mmic data (``num_splits``: per sample, tiles per image): the global tile of each image (cumulative sums - 1), the
        first ``num_regions[i]`` of them (one region per image);
      * 'pad' (``split_sizes`` None): image i itself, once per region.
    ``len(split_sizes)`` (or ``n_images``) may be a multiple of ``len(num_regions)``: generate() with num_beams > 1 (:617-621)."""
    num_regions = [int(n) for n in num_regions]
    n_samples = len(split_sizes) if split_sizes is not None else int(n_images)
    if len(num_regions) == 0 or n_samples % len(num_regions) != 0:
        raise RuntimeError(f"region_tile_index: {n_samples} samples vs {len(num_regions)} region lists")
    num_regions = num_regions * (n_samples // len(num_regions))
    tiles = []
    if split_sizes is None:
        for i, n in enumerate(num_regions):
            tiles += [i] * n
        return tiles
    split_sizes = [int(x) for x in split_sizes]
    if any(x <= 0 for x in split_sizes):
        raise RuntimeError(f"region_tile_index: every sample needs at least one tile (split_sizes = {split_sizes})")
    off = 0
    for i, (n_tiles, n) in enumerate(zip(split_sizes, num_regions)):
        if num_splits is not None:
            per_image = [int(x) for x in num_splits[i]]
            if sum(per_image) != n_tiles or any(x <= 0 for x in per_image):
                raise RuntimeError(f"region_tile_index: num_splits[{i}] = {per_image} does not add up to {n_tiles} tiles")
            if n > len(per_image):
                raise RuntimeError(f"region_tile_index: sample {i} has {n} regions but {len(per_image)} images")
            last, acc = [], 0
            for x in per_image:
                acc += x
                last.append(off + acc - 1)
            tiles += last[:n]
        else:
            tiles += [off + n_tiles - 1] * n
        off += n_tiles
    return tiles


def gather_region_images(images, num_regions, num_splits=None):
    """all_images of the region branch (modeling_visionllmv2.py:626-643): [n_all_regions, 3, h, w] -- one image per region.
    ``images``: list of per-sample tile stacks ('anyres' / mmic) or one [B, 3, h, w] tensor ('pad').  Pixels feed the region
    encoder's conv stem (torch), so this is a plain index_select."""
    if isinstance(images, (list, tuple)):
        tiles = region_tile_index([len(x) for x in images], num_regions, num_splits)
        cat = torch.cat(list(images), dim=0)
    else:
        tiles = region_tile_index(None, num_regions, n_images=images.shape[0])
        cat = images
    return cat.index_select(0, torch.as_tensor(tiles, dtype=torch.long, device=cat.device))


def _region_segments(tile_of_region, n_tiles, S1):
    """CSR list of the region gather's backward for one level shape: row (tile, 1 + t) of grad_hidden_states sums rows r * T + t of
    grad_out over the regions r of that tile, ascending; CLS rows and the rows of a tile no region reads are empty.  Pure torch."""
    T = S1 - 1
    t = torch.arange(T, device=tile_of_region.device)
    keys = (tile_of_region[:, None] * S1 + 1 + t[None, :]).reshape(-1)       # the forward's source row of output row r * T + t
    return _segments(keys, torch.arange(keys.numel(), device=keys.device), n_tiles * S1)


def _gather_region_rows(hs, src, n_regions):
    hs = hs.contiguous()
    n, S1, C = hs.shape
    out = torch.empty((n_regions, S1 - 1, C), dtype=hs.dtype, device=hs.device)   # every row is written: src covers all of it
    _copy_rows(hs.view(n * S1, C), src, out.view(-1, C), None, src.numel())
    return out


class _GatherRegionFeatures(torch.autograd.Function):
    """One level of the region feature selection as an autograd node: the backward is ONE segment sum that writes every row of
    grad_hidden_states[level], CLS rows and unread tiles as zeros."""

    @staticmethod
    def forward(ctx, hs, src, n_regions, seg_ptr, src_idx):
        ctx.save_for_backward(seg_ptr, src_idx)
        ctx.in_shape = tuple(hs.shape)
        return _gather_region_rows(hs.detach(), src, n_regions)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        seg_ptr, src_idx = ctx.saved_tensors
        n, S1, C = ctx.in_shape
        g = _lib.aligned(grad_out)
        return _segment_sum(g.view(-1, C), seg_ptr, src_idx, n * S1).view(n, S1, C), None, None, None, None


def gather_region_image_features(hidden_states, split_sizes, num_regions, levels=(-3, -2, -1), num_splits=None, native_backward=False):
    """Region branch, feature selection (modeling_visionllmv2.py:644-676): for every region the features of ITS image's
    global tile without CLS, at the last three encoder levels (see region_tile_index for the three input conventions;
    ``split_sizes`` None = 'pad').  hidden_states: indexable of [n_tiles, 1 + T, C] bf16; -> list of [n_all_regions, T, C]
    (one native row gather per level).  By default forward-only; with ``native_backward=True`` every level that requires grad is an
    autograd node of its own (the region branch's gradient into the tower): a tile's row sums the gradients of the regions that
    read it, in fp32 and in ascending region order."""
    outs = []
    dev = hidden_states[levels[0]].device
    n_tiles = hidden_states[levels[0]].shape[0]
    tiles = region_tile_index(split_sizes, num_regions, num_splits, n_images=n_tiles)
    if split_sizes is not None and sum(int(x) for x in split_sizes) != n_tiles:
        raise RuntimeError(f"gather_region_image_features: split_sizes add up to {sum(split_sizes)}, the encoder saw {n_tiles} tiles")
    tile_of_region = torch.tensor(tiles, device=dev, dtype=torch.int64)
    segments = {}                                                # the backward's CSR list, shared by the levels of one shape
    for lv in levels:
        hs = hidden_states[lv]
        if not native_backward:
            _no_grad_path("gather_region_image_features", hs)
        n, S1, C = hs.shape
        T = S1 - 1
        src = (tile_of_region[:, None] * S1 + 1 + torch.arange(T, device=dev)[None, :]).reshape(-1)
        if _wants_grad(native_backward, hs):
            if S1 not in segments:
                segments[S1] = _region_segments(tile_of_region, n, S1)
            outs.append(_GatherRegionFeatures.apply(hs, src, tile_of_region.numel(), *segments[S1]))
        else:
            outs.append(_gather_region_rows(hs, src, tile_of_region.numel()))
    return outs


def splice_region_tokens(inputs_embeds, input_ids, reg_token_id, region_features, native_backward=False):
    """<region> slots (modeling_visionllmv2.py:688-695): inputs_embeds[input_ids == reg_token_id] = region_features, in place.
    By default forward-only; with ``native_backward=True`` and an input that requires grad the splice is an in-place autograd node
    (the LLM loss reaches the region encoder through this statement and nothing else): the embeddings' gradient is grad_out with the
    slot rows zeroed, region feature i takes grad_out at slot i (in its own dtype and shape).  A leaf ``inputs_embeds`` that requires
    grad fails with torch's in-place error, as in the visual splice."""
    B, L, C = inputs_embeds.shape
    if not native_backward:
        _no_grad_path("splice_region_tokens", inputs_embeds, region_features)
    slot = (input_ids == reg_token_id).reshape(-1)
    dst = torch.nonzero(slot, as_tuple=False).reshape(-1)
    n_feats = region_features.numel() // C
    if dst.numel() != n_feats:
        raise RuntimeError(f"splice_region_tokens: {dst.numel()} <region> slots cannot take {n_feats} region features")
    if _wants_grad(native_backward, inputs_embeds, region_features):
        return _SpliceRegionTokens.apply(inputs_embeds, region_features, slot.to(torch.uint8), dst)
    return _splice_region_rows(inputs_embeds, region_features, dst)


def _splice_region_rows(inputs_embeds, region_features, dst):
    B, L, C = inputs_embeds.shape
    feats = region_features.to(inputs_embeds.dtype).reshape(-1, C).contiguous()
    _copy_rows(feats, None, inputs_embeds.view(B * L, C), dst, dst.numel())
    return inputs_embeds


class _SpliceRegionTokens(torch.autograd.Function):
    """The <region> splice as an in-place autograd node.  The backward uses the slot flags and the slot list the forward computed (no
    second scan of input_ids, no host read): a masked copy for the embeddings, a row gather for the region features -- at most two
    native calls, neither made when nobody needs its output."""

    @staticmethod
    def forward(ctx, inputs_embeds, region_features, zero_row, dst):
        _splice_region_rows(inputs_embeds, region_features.detach(), dst)
        ctx.mark_dirty(inputs_embeds)
        ctx.save_for_backward(zero_row, dst)
        ctx.feats = (tuple(region_features.shape), region_features.dtype)
        return inputs_embeds

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        zero_row, dst = ctx.saved_tensors
        C = grad_out.shape[-1]
        g = _lib.aligned(grad_out)
        g_embeds = _copy_rows_masked(g, zero_row) if ctx.needs_input_grad[0] else None
        g_feats = None
        if ctx.needs_input_grad[1]:
            shape, dtype = ctx.feats
            g_feats = torch.empty((dst.numel(), C), dtype=g.dtype, device=g.device)   # (every row is written: one per slot)
            _copy_rows(g.view(-1, C), dst, g_feats, None, dst.numel())
            g_feats = g_feats.to(dtype).reshape(shape)
        return g_embeds, g_feats, None, None
