"""The four token loops around the LLM under training (forward + backward) at the model's shapes:
  [EMB] side: 8 x 4096 positions x 4096 channels; every sample carries one det and one pose tool token, each followed by its 4 [EMB]
  ids, and sample 3 also a gen token followed by 64 (128 replaced rows; tables of 4 / 4 / 64 rows);
  region side: split_sizes [5] * 8 (40 tiles), 2 regions per sample (16 regions, each reading its sample's global tile), 576 tokens x
  1024 channels at 3 levels, and 16 <region> slots in the 8 x 4096 x 4096 embeddings.
For each of splice_emb_tokens, gather_emb_hidden_states, gather_region_image_features and splice_region_tokens:
  (a) native: the function with native_backward=True under autograd, forward + backward through Python;
  (b) torch's bf16 autograd of the reference's statements (modeling_visionllmv2.py:432-527, 775-787, 644-681, 688-698), written out
      below, on the same tensors -- what the reference runs, independent of the code under test;
and (c) each new kernel alone through the C ABI at the shapes the four backwards launch it with, as a share of the measured float4-copy
rate of 6.29 TB/s: bytes from shapes (source rows read + destination rows written; a zeroed row is written but not read).
The in-place splices start from a non-leaf clone of the embeddings in (a) and (b) alike, and every path ends with backward() into the
leaves.  Device events around >= --seconds of work per timing after warm-up, the paths alternated in one process, three rounds; the
minimum and all rounds are printed, and the shader clock sampled meanwhile (bench.py's ClockSampler).

    python tools/bench_token_loops_train.py [--seconds 0.5]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import ClockSampler  # noqa: E402
from visionllm_amd import _lib  # noqa: E402
from visionllm_amd import splice as S  # noqa: E402

HBM = 6.29e12          # measured float4 copy rate of the MI355X, bytes / s
B, L, C = 8, 4096, 4096
DET, POSE, GEN, E0, NE, NG, REG = 60, 61, 62, 100, 4, 64, 77
SPLIT, REGIONS, T, CR, LEVELS = [5] * 8, [2] * 8, 576, 1024, 3


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters   # us


# ---- (b): the reference's statements, re-typed --------------------------------------------------------------------------------------------
def composed_emb_splice(input_ids, inputs_embeds, tables):
    new_ids, new_embeds = [], []
    for cur_ids, cur_embeds in zip(input_ids, inputs_embeds):
        ids_b, emb_b = cur_ids, cur_embeds
        for tool_id, table in tables.items():
            gap = NG if tool_id == GEN else NE
            emb_ids = (E0 * torch.ones(NG, dtype=torch.long, device=cur_ids.device) if tool_id == GEN
                       else torch.arange(E0, E0 + NE, dtype=torch.long, device=cur_ids.device))
            for start in torch.where(cur_ids == tool_id)[0]:
                ids_b = torch.cat([ids_b[: start + 1], emb_ids, ids_b[start + gap + 1:]], dim=0)
                emb_b = torch.cat([emb_b[: start + 1], table.to(emb_b.dtype), emb_b[start + gap + 1:]], dim=0)
        new_ids.append(ids_b)
        new_embeds.append(emb_b)
    return torch.stack(new_ids, dim=0), torch.stack(new_embeds, dim=0)


def composed_text_query(hidden_states, input_ids):
    sel = (input_ids >= E0) & (input_ids <= E0 + NE - 1)
    num_patches = sel.sum(-1) // NE
    max_p = int(num_patches.max())
    text_query = torch.zeros((B, max_p, NE, C), dtype=hidden_states.dtype, device=hidden_states.device)
    masks = torch.zeros(B, max_p, dtype=torch.bool, device=hidden_states.device)
    for b in range(B):
        if num_patches[b] != 0:
            text_query[b, :num_patches[b]] = hidden_states[b, sel[b], :].reshape(-1, NE, C)
            masks[b, :num_patches[b]] = 1
    return text_query, masks


def composed_region_features(hidden_states):
    outs = []
    for hs in hidden_states:
        per_sample = torch.split(hs, SPLIT, dim=0)
        glob = torch.stack([x[-1, 1:] for x in per_sample], dim=0)
        outs.append(torch.cat([glob[i][None].repeat_interleave(REGIONS[i], dim=0) for i in range(B)]))
    return outs


def composed_region_splice(inputs_embeds, input_ids, region_features):
    flat = inputs_embeds.reshape(B * L, C)
    mask = (input_ids == REG).reshape(-1)
    temp = torch.zeros_like(flat)
    temp[mask] = region_features.to(flat.dtype)
    m = mask.to(flat.dtype).unsqueeze(-1)
    return (flat * (1 - m) + temp * m).reshape(B, L, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L_ = _lib.lib()
    torch.manual_seed(0)
    bf = torch.bfloat16
    leaf = lambda *shape: torch.randn(*shape, device=dev).to(bf).requires_grad_(True)   # noqa: E731

    # [EMB] side
    ids = torch.randint(200, 300, (B, L), device=dev)
    for b in range(B):
        ids[b, 100 + b], ids[b, 900 + b] = DET, POSE
        ids[b, 101 + b:105 + b] = ids[b, 901 + b:905 + b] = torch.arange(E0, E0 + NE, device=dev)
    ids[3, 2000], ids[3, 2001:2001 + NG] = GEN, E0
    emb, g_emb = leaf(B, L, C), torch.randn(B, L, C, device=dev).to(bf)
    tabs = {"det": leaf(NE, C), "pose": leaf(NE, C), "gen": leaf(NG, C)}
    tables = {DET: tabs["det"], POSE: tabs["pose"], GEN: tabs["gen"]}
    hidden = leaf(B, L, C)
    # region side
    n_tiles, n_regions = sum(SPLIT), sum(REGIONS)
    levels = [leaf(n_tiles, 1 + T, CR) for _ in range(LEVELS)]
    g_levels = [torch.randn(n_regions, T, CR, device=dev).to(bf) for _ in range(LEVELS)]
    reg_ids = torch.randint(200, 300, (B, L), device=dev)
    for b in range(B):
        reg_ids[b, 50 + b], reg_ids[b, 3000 + b] = REG, REG
    reg_feats = leaf(n_regions, C)

    def clear(*leaves):
        for t in leaves:
            t.grad = None

    def emb_native():
        clear(emb, *tabs.values())
        S.splice_emb_tokens(ids, emb.clone(), tables, E0, NE, NG, gen_tools=(GEN,), native_backward=True)[1].backward(g_emb)

    def emb_torch():
        clear(emb, *tabs.values())
        composed_emb_splice(ids, emb.clone(), tables)[1].backward(g_emb)

    with torch.no_grad():
        ids_spliced, _ = S.splice_emb_tokens(ids, emb.detach().clone(), tables, E0, NE, NG, gen_tools=(GEN,))
    tq_shape = composed_text_query(hidden.detach(), ids_spliced)[0].shape
    g_tq = torch.randn(tq_shape, device=dev).to(bf)

    def tq_native():
        clear(hidden)
        S.gather_emb_hidden_states(hidden, ids_spliced, E0, NE, native_backward=True)[0].backward(g_tq)

    def tq_torch():
        clear(hidden)
        composed_text_query(hidden, ids_spliced)[0].backward(g_tq)

    def feats_native():
        clear(*levels)
        torch.autograd.backward(S.gather_region_image_features(levels, SPLIT, REGIONS, native_backward=True), g_levels)

    def feats_torch():
        clear(*levels)
        torch.autograd.backward(composed_region_features(levels), g_levels)

    def reg_native():
        clear(emb, reg_feats)
        S.splice_region_tokens(emb.clone(), reg_ids, REG, reg_feats, native_backward=True).backward(g_emb)

    def reg_torch():
        clear(emb, reg_feats)
        composed_region_splice(emb.clone(), reg_ids, reg_feats).backward(g_emb)

    pairs = {"splice_emb_tokens": (emb_native, emb_torch, [emb, *tabs.values()]), "gather_emb_hidden_states": (tq_native, tq_torch, [hidden]),
             "gather_region_image_features": (feats_native, feats_torch, levels), "splice_region_tokens": (reg_native, reg_torch, [emb, reg_feats])}
    for name, (nat, ref, leaves) in pairs.items():      # the two paths agree before anything is timed (sums: to bf16 rounding)
        nat()
        got = [t.grad.clone() for t in leaves]
        ref()
        for a, t in zip(got, leaves):
            # (loose on purpose: torch adds the uses of a table row one by one in bf16; the tests hold the native sums to their bound)
            assert torch.allclose(a.float(), t.grad.float(), rtol=5e-2, atol=0.1), f"{name}: native and torch gradients differ"

    # (c): the kernels alone, at the shapes the four backwards launch them with
    st = _lib.current_stream(dev)
    P = _lib.ptr
    kernels, nbytes = {}, {}

    def masked(flag, what):
        out = torch.empty_like(g_emb)
        kernels[what] = lambda: _lib.check(L_.vllm_copy_rows_masked_bf16(P(g_emb), P(flag), P(out), B * L, C, st))
        nbytes[what] = (2 * B * L - int(flag.sum())) * C * 2

    def segsum(src, seg_ptr, src_idx, dst_rows, what):
        cols = src.shape[-1]
        out = torch.empty(dst_rows, cols, dtype=bf, device=dev)
        kernels[what] = lambda: _lib.check(L_.vllm_rows_segment_sum_bf16(P(src), src.numel() // cols, P(seg_ptr), P(src_idx), src_idx.numel(), P(out),
                                                                        dst_rows, cols, st))
        nbytes[what] = (src_idx.numel() + dst_rows) * cols * 2

    writes, base = [], 0
    for tool_id, table in tables.items():
        n_rows = table.shape[0]
        writes.append((*S._emb_block_rows(torch.nonzero(ids == tool_id, as_tuple=False), L, n_rows), base))
        base += n_rows
    zero_row, seg_ptr, src_idx = S._emb_segments(S._emb_owner_map(B * L, writes), base)
    masked(zero_row, "copy_rows_masked (grad of the embeddings, 128 of 32768 rows zeroed)")
    segsum(g_emb, seg_ptr, src_idx, base, "rows_segment_sum (grad of the 72 table rows, 128 terms)")
    sel = (ids_spliced >= E0) & (ids_spliced <= E0 + NE - 1)
    kept = torch.nonzero(sel.reshape(-1), as_tuple=False).reshape(-1)
    tq_row = (kept // L) * (tq_shape[1] * NE) + (sel.cumsum(-1) - 1).reshape(-1)[kept]
    segsum(g_tq, *S._segments(kept, tq_row, B * L), B * L, "rows_segment_sum (grad of the hidden states, 32768 rows, 128 of one term)")
    tile_of_region = torch.tensor(S.region_tile_index(SPLIT, REGIONS), device=dev)
    segsum(g_levels[0], *S._region_segments(tile_of_region, n_tiles, 1 + T), n_tiles * (1 + T),
           "rows_segment_sum (grad of one tower level, 23080 rows x 1024, 9216 terms)")

    paths = {}
    for name, (nat, ref, _) in pairs.items():
        paths[name + ": native"], paths[name + ": torch"] = nat, ref
    paths.update(kernels)
    iters = {}
    for k, f in paths.items():              # warm-up, and the iteration count that fills --seconds
        for _ in range(3):
            f()
        iters[k] = max(10, math.ceil(args.seconds * 1e6 / timed(f, 5)))
    rounds = {k: [] for k in paths}
    clk = ClockSampler(dev)
    sampled = clk.has_sysfs()
    if sampled:
        clk.start()
    for _ in range(3):                      # alternated
        for k, f in paths.items():
            rounds[k].append(timed(f, iters[k]))
    clocks = clk.stop() if sampled else None
    out = {"lib": os.path.relpath(_lib.lib_path(), ROOT), "hbm_copy_bytes_per_s": HBM,
           "clocks": clocks if clocks else "no amdgpu hwmon files readable: clock not sampled",
           "shape": {"B": B, "L": L, "C": C, "replaced_rows": int(zero_row.sum()), "tiles": n_tiles, "regions": n_regions, "T": T, "C_region": CR,
                     "levels": LEVELS, "text_query": list(tq_shape)}}
    for k, t in rounds.items():
        out[k] = {"us": round(min(t), 1), "all_us": [round(u, 1) for u in t], "iters": iters[k]}
    for k in kernels:
        out[k]["bytes"] = nbytes[k]
        out[k]["us_at_the_copy_rate"] = round(nbytes[k] / HBM * 1e6, 1)
        out[k]["share_of_hbm_copy_rate"] = round(nbytes[k] / (min(rounds[k]) * 1e-6) / HBM, 3)
    for name in pairs:
        out[name + ": native_over_torch"] = round(min(rounds[name + ": native"]) / min(rounds[name + ": torch"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
