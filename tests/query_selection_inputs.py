"""Module, inputs and the fp64 yardstick of the query selection's tests (test_query_selection_cpu.py, test_query_selection_gpu.py).

One model: d_model 64, 2 levels [[5, 7], [3, 4]] (S = 47), B 2, Lt 5 of max_text_len 8.  As in deform_decoder_inputs every parameter is the
module's own initial value plus 0.2 randn rounded to bf16, so that the fp64 module and the bf16 module hold the same numbers; the last
layer of the box head is scaled by 0.02 (deltas of a few tenths of a logit, as a trained head gives).

Image 0 is unpadded.  Image 1 is padded so that its valid extents (the unpadded cells of column 0 and of row 0: 3 x 4 of 5 x 7, 2 x 3 of
3 x 4) are smaller than its maps, and four cells outside those extents are left unpadded: their proposals exceed 0.99, so the image has
padded rows AND unpadded rows with invalid proposals.  One text token of image 1 is masked.

The yardstick (``reference``) is the mirror's own composed ``forward`` on a ``.double()`` CPU copy.  It never calls the native library.
Nothing here touches torch.cuda at import."""
import copy
import functools

import torch
from torch import nn

from visionllm_amd import query_selection as Q

C, MAPS, B, LT, MTL = 64, [(5, 7), (3, 4)], 2, 5, 8
S = sum(h * w for h, w in MAPS)
LSI = [0, 35]
EXTENTS = {0: [(5, 7), (3, 4)], 1: [(3, 4), (2, 3)]}          # image -> per level (valid_height, valid_width)
UNPADDED_OUTSIDE = [(0, 4, 6), (0, 3, 2), (0, 1, 5), (1, 2, 3)]          # (level, y, x) of image 1: real cells outside its extents
KS = (9, S)          # S: every row is selected, the invalid ones too


def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((p + 0.2 * torch.randn(p.shape, generator=g)).to(torch.bfloat16).float())


def make_module():
    """-> the module in fp32 (eval mode) whose parameters are bf16 values"""
    torch.manual_seed(41)
    m = Q.GroundingDinoQuerySelection(C, MTL)
    _perturb(m, 141)
    with torch.no_grad():
        for p in m.encoder_output_bbox_embed.layers[-1].parameters():
            p.copy_((0.02 * p).to(torch.bfloat16).float())
    return m.eval()


def as_bf16(m, device):
    return copy.deepcopy(m).to(device).to(torch.bfloat16).eval()


def real_mask():
    """mask_flatten: bool [B, S], True = a real cell (the model's convention)"""
    real = torch.ones(B, S, dtype=torch.bool)
    for l, (H, W) in enumerate(MAPS):
        vh, vw = EXTENTS[1][l]
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        real[1, LSI[l]:LSI[l] + H * W] = ((ys < vh) & (xs < vw)).flatten()
    for l, y, x in UNPADDED_OUTSIDE:
        real[1, LSI[l] + y * MAPS[l][1] + x] = True
    return real


@functools.lru_cache(maxsize=None)
def make_inputs():
    """-> dict of CPU tensors: memory [B, S, C] and text [B, Lt, C] (bf16), mask_flatten (bool [B, S], True = real), text_token_mask (bool
    [B, Lt], True = a real token), spatial_shapes (int64), query_embeds [S, C] (bf16; a test slices the rows it needs).  Cached: leave it
    unchanged."""
    g = torch.Generator().manual_seed(400)
    memory = torch.randn(B, S, C, generator=g).to(torch.bfloat16)
    text = torch.randn(B, LT, C, generator=g).to(torch.bfloat16)
    qe = torch.randn(S, C, generator=g).to(torch.bfloat16)
    tmask = torch.ones(B, LT, dtype=torch.bool)
    tmask[1, 2] = False
    return dict(memory=memory, text=text, mask_flatten=real_mask(), text_token_mask=tmask, spatial_shapes=torch.tensor(MAPS, dtype=torch.int64),
                query_embeds=qe)


def to(t, device, dtype=None):
    """the dict on ``device``; floating tensors cast to ``dtype`` where given"""
    out = {}
    for k, v in t.items():
        v = v.to(device)
        out[k] = v.to(dtype) if dtype is not None and v.is_floating_point() else v
    return out


def call(m, t, k, with_query_embeds=False, **kw):
    return m(t["memory"], t["text"], t["mask_flatten"], t["text_token_mask"], t["spatial_shapes"], k,
             t["query_embeds"][:k] if with_query_embeds else None, **kw)


def reasons(m, t, k, with_query_embeds=False, **kw):
    return m.native_selection_reasons(t["memory"], t["text"], t["mask_flatten"], t["text_token_mask"], t["spatial_shapes"], k,
                                      t["query_embeds"][:k] if with_query_embeds else None, **kw)


@functools.lru_cache(maxsize=None)
def reference():
    """-> the QuerySelectionOutput of the fp64 module on the bf16-valued inputs (its full tensors are what the tests gather from; k = S).
    Computed once on the CPU; leave it unchanged."""
    m = copy.deepcopy(make_module()).double()
    with torch.no_grad():
        return call(m, to(make_inputs(), "cpu", torch.float64), S)


def closed_form_proposals(real, maps):
    """gen_encoder_output_proposals' second result said again, cell by cell in fp64 -> (logits [B, S, 4] with +inf where the reference
    fills, valid flags [B, S] of the proposals alone)"""
    Bn = real.shape[0]
    Sn = sum(h * w for h, w in maps)
    out = torch.empty(Bn, Sn, 4, dtype=torch.float64)
    valid = torch.empty(Bn, Sn, dtype=torch.bool)
    for b in range(Bn):
        s0 = 0
        for l, (H, W) in enumerate(maps):
            vh = sum(bool(real[b, s0 + y * W]) for y in range(H))
            vw = sum(bool(real[b, s0 + x]) for x in range(W))
            for y in range(H):
                for x in range(W):
                    p = [(x + 0.5) / vw if vw else float("inf"), (y + 0.5) / vh if vh else float("inf"), 0.05 * 2.0 ** l, 0.05 * 2.0 ** l]
                    ok = all(0.01 < v < 0.99 for v in p)
                    s = s0 + y * W + x
                    valid[b, s] = ok
                    for c in range(4):
                        out[b, s, c] = torch.log(torch.tensor(p[c] / (1 - p[c]), dtype=torch.float64)) if ok and real[b, s] else float("inf")
            s0 += H * W
    return out, valid


def stable_topk(scores, k):
    """the documented order: value descending, ties by ascending index, NaN greatest"""
    return torch.sort(scores.cpu(), dim=-1, descending=True, stable=True).indices[..., :k]


class FakeCuda(torch.Tensor):
    """a CPU tensor that says it is on the GPU: the reasons are decided from dtypes, shapes and flags alone"""
    @property
    def is_cuda(self):
        return True


def fake(t):
    return None if t is None else t.as_subclass(FakeCuda)


def fake_module(m):
    m = as_bf16(m, "cpu")
    for mod in m.modules():
        for k, p in list(mod._parameters.items()):
            if p is not None:
                mod._parameters[k] = nn.Parameter(p.data, requires_grad=p.requires_grad).as_subclass(FakeCuda)
    return m
