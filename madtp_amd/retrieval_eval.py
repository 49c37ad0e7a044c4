"""Retrieval evaluation on the device: the CLIP driver's evaluate() (compress_retrieval_clip_dtp.py:78-124) and every
retrieval driver's itm_eval() (:127-171) - recall@1/5/10 in both directions.

The reference builds the [n_img, n_txt] similarity matrix, copies it and its transpose to the host and runs one np.argsort
per row.  The metric only needs "how many keys score above the ground truth", which hip.rank_embeds counts in the epilogue
of the products (no matrix) and hip.rank_scores counts in one pass over a given score matrix (BLIP's re-ranked ones).

Tie rule (the reference's default argsort leaves it open): rank = #{j != t : s_j > s_t} + #{j > t : s_j == s_t}, the position of
t in np.argsort(s, kind="stable")[::-1].  At most MAX_TARGETS ground-truth keys per row."""
from collections import namedtuple

import numpy as np
import torch

from . import controller, harness, hip, workloads
from .runtime import require_gpu

MAX_TARGETS = 16

Targets = namedtuple("Targets", "i2t_ptr i2t_idx t2i_ptr t2i_idx")


def _rows(mapping, n, what):
    """dict {row: target(s)} or a list indexed by row -> list of target lists"""
    if isinstance(mapping, dict):
        missing = [r for r in range(n) if r not in mapping]
        if missing:
            raise ValueError(f"{what}: no entry for row {missing[0]}")
        rows = [mapping[r] for r in range(n)]
    else:
        rows = list(mapping)
        if len(rows) != n:
            raise ValueError(f"{what}: {len(rows)} rows, expected {n}")
    out = []
    for x in rows:
        if torch.is_tensor(x) or isinstance(x, np.ndarray):
            x = x.tolist()
        out.append([int(t) for t in x] if isinstance(x, (list, tuple)) else [int(x)])
    return out


def _csr(rows, nk, what):
    ptr = [0]
    idx = []
    for r, targets in enumerate(rows):
        if len(targets) > MAX_TARGETS:
            raise ValueError(f"{what}: row {r} has {len(targets)} targets, at most {MAX_TARGETS} are supported")
        for t in targets:
            if not 0 <= t < nk:
                raise ValueError(f"{what}: row {r} names key {t} outside [0, {nk})")
        idx.extend(targets)
        ptr.append(len(idx))
    return torch.tensor(ptr, dtype=torch.int32), torch.tensor(idx, dtype=torch.int32)


def target_lists(txt2img, img2txt, n_img, n_txt, device=None):
    """The datasets' ground truth as CSR int32 tensors for both directions -> Targets(i2t_ptr, i2t_idx, t2i_ptr, t2i_idx).
    img2txt: per image the list of its captions (list of lists, or dict); txt2img: per caption its image (list, or dict; a list
    of images per caption is taken too).  Validated on the host: ValueError for an index outside the other side's range or
    more than MAX_TARGETS targets in a row."""
    i2t = _csr(_rows(img2txt, n_img, "img2txt"), n_txt, "img2txt")
    t2i = _csr(_rows(txt2img, n_txt, "txt2img"), n_img, "txt2img")
    out = Targets(i2t[0], i2t[1], t2i[0], t2i[1])
    return out if device is None else Targets(*(t.to(device) for t in out))


def rank_embeds(q, keys, tgt_ptr, tgt_idx):
    """(rank_row, rank_tgt, score_tgt) of the targets among <q_r, keys_j>; device tensors only (hip.rank_embeds)."""
    return hip.rank_embeds(q, keys, tgt_ptr, tgt_idx)


def rank_scores(scores, tgt_ptr, tgt_idx):
    """(rank_row, rank_tgt) of the targets in a dense f32 score matrix; device tensors only (hip.rank_scores)."""
    return hip.rank_scores(scores, tgt_ptr, tgt_idx)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def recall_metrics(ranks_i2t, ranks_t2i):
    """itm_eval's nine-key dict from the per-row ranks (image -> text: the best of the image's captions)."""
    ri, rt = _np(ranks_i2t), _np(ranks_t2i)
    tr1, tr5, tr10 = (100.0 * len(np.where(ri < k)[0]) / len(ri) for k in (1, 5, 10))
    ir1, ir5, ir10 = (100.0 * len(np.where(rt < k)[0]) / len(rt) for k in (1, 5, 10))
    tr_mean = (tr1 + tr5 + tr10) / 3
    ir_mean = (ir1 + ir5 + ir10) / 3
    r_mean = (tr_mean + ir_mean) / 2
    return {'txt_r1': tr1, 'txt_r5': tr5, 'txt_r10': tr10, 'txt_r_mean': tr_mean,
            'img_r1': ir1, 'img_r5': ir5, 'img_r10': ir10, 'img_r_mean': ir_mean, 'r_mean': r_mean}


def itm_eval(scores_i2t, scores_t2i, txt2img, img2txt):
    """The drivers' itm_eval(scores_i2t, scores_t2i, txt2img, img2txt) -> the nine-key dict.  Device tensors are ranked where
    they are (a view whose rows are not contiguous, such as sims.t(), from a row-major copy); numpy arrays (what
    blip_retrieval.evaluate() returns) are uploaded first.  Two lists.CandidateLists (evaluate(scores="lists")) are ranked as
    lists (madtp_lists_rank): the same ranks, and no matrix is formed."""
    from .lists import CandidateLists
    if isinstance(scores_i2t, CandidateLists) or isinstance(scores_t2i, CandidateLists):
        if not (isinstance(scores_i2t, CandidateLists) and isinstance(scores_t2i, CandidateLists)):
            raise ValueError("itm_eval: one argument is a CandidateLists, the other is not")
        n_img, n_txt = scores_i2t.shape[0], scores_t2i.shape[0]
        if (scores_i2t.nk, scores_t2i.nk) != (n_txt, n_img):
            raise ValueError(f"the lists are over {scores_i2t.nk} texts and {scores_t2i.nk} images, expected {n_txt} and {n_img}")
        t = target_lists(txt2img, img2txt, n_img, n_txt, device=scores_i2t.device)
        return recall_metrics(scores_i2t.rank(t.i2t_ptr, t.i2t_idx)[0], scores_t2i.rank(t.t2i_ptr, t.t2i_idx)[0])

    def dev(m):
        if not torch.is_tensor(m):
            m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda()
        m = require_gpu(m, "score matrix")
        return m if m.stride(-1) == 1 else m.contiguous()  # a driver passes sims.t(): ranked from a row-major copy
    si, st = dev(scores_i2t), dev(scores_t2i)
    n_img, n_txt = si.shape
    if tuple(st.shape) != (n_txt, n_img):
        raise ValueError(f"scores_t2i is {tuple(st.shape)}, expected {(n_txt, n_img)}")
    t = target_lists(txt2img, img2txt, n_img, n_txt, device=si.device)
    ri, _ = rank_scores(si, t.i2t_ptr, t.i2t_idx)
    rt, _ = rank_scores(st, t.t2i_ptr, t.t2i_idx)
    return recall_metrics(ri, rt)


class _ClipPairs:
    """The analytic counter of both CLIP towers (workloads.clip_tower_flops) per image-text pair at the geometry of a given model,
    for controller.workload_gflops: lens = {"vit": [(samples, per-layer lengths), ...], "text": [...]}, one entry per batch."""

    def __init__(self, model):
        v = model.visual
        self.patch, self.width, self.text_width = v.patch_size, v.conv1.out_channels, model.transformer.width
        self.n0, self.ctx = (v.input_resolution // v.patch_size) ** 2 + 1, model.context_length

    def flops(self, lens):
        def mean(batches, count):
            return sum(b * count(l) for b, l in batches) / sum(b for b, _ in batches)
        return (mean(lens["vit"], lambda l: workloads.clip_tower_flops(l, self.n0, self.width, patch_in=3 * self.patch ** 2))
                + mean(lens["text"], lambda l: workloads.clip_tower_flops(l, self.ctx, self.text_width)))


class ClipEval:
    """What clip_evaluate() leaves on the device: the normalised embeddings, the per-layer token counts of every batch and the
    GFLOPs per image-text pair they imply."""

    def __init__(self, image_embeds, text_embeds, gflops, vit_lens, txt_lens):
        self.image_embeds, self.text_embeds, self.gflops = image_embeds, text_embeds, gflops
        self.vit_lens, self.txt_lens = vit_lens, txt_lens

    def ranks(self, txt2img, img2txt):
        """((rank_row, rank_tgt, score_tgt) image -> text, the same text -> image)"""
        t = target_lists(txt2img, img2txt, self.image_embeds.shape[0], self.text_embeds.shape[0], device=self.image_embeds.device)
        return (rank_embeds(self.image_embeds, self.text_embeds, t.i2t_ptr, t.i2t_idx),
                rank_embeds(self.text_embeds, self.image_embeds, t.t2i_ptr, t.t2i_idx))

    def metrics(self, txt2img, img2txt):
        """itm_eval's dict; no similarity matrix is formed."""
        i2t, t2i = self.ranks(txt2img, img2txt)
        return recall_metrics(i2t[0], t2i[0])

    def search(self, k, direction="i2t", coarse=None):
        """(values f32 [n,k], indices int64 [n,k]): the k best texts of every image ("i2t") or images of every text ("t2i"),
        best first, in the order ranks() counts in (search.topk_embeds); no similarity matrix is formed.  coarse="bf16": the
        same answer through the certified bf16 shortlist (k <= 128)."""
        from . import search
        if direction not in ("i2t", "t2i"):
            raise ValueError(f"direction = {direction!r}: expected 'i2t' or 't2i'")
        q, keys = (self.image_embeds, self.text_embeds) if direction == "i2t" else (self.text_embeds, self.image_embeds)
        return search.topk_embeds(q, keys, k) if coarse is None else search.topk_embeds(q, keys, k, coarse=coarse)

    def score_matrices(self):
        """the reference's return value: (sims, sims.T, GFLOPs) with the matrices as numpy arrays"""
        ft = self.text_embeds
        pad = (-ft.shape[0]) % 128
        w = torch.cat([ft, ft.new_zeros(pad, ft.shape[1])], 0) if pad else ft
        sims = hip.gemm(self.image_embeds.contiguous(), w.contiguous(), n=ft.shape[0])
        return sims.cpu().numpy(), sims.t().cpu().numpy(), self.gflops


def _clip_tokens(model, text, device):
    if torch.is_tensor(text):
        return text.to(device=device, dtype=torch.int64)
    if model.tokenize is not None:
        return model.tokenize(text).to(device=device, dtype=torch.int64)
    raise TypeError("dataset.text must yield int tensors [n, context] of token ids or model.tokenize must be set")


@torch.no_grad()
def clip_evaluate(model, data_loader, device, config, temperature=0, text_bs=256):
    """compress_retrieval_clip_dtp.py evaluate() :78-124 -> ClipEval.  The embeddings stay on the device; .metrics() ranks them
    there and .score_matrices() gives the reference's (sims, sims.T, GFLOPs) triple.  GFLOPs: the analytic per-pair count of
    both towers (controller.workload_gflops) at the observed per-layer token counts, averaged over the samples - the
    reference's fvcore count of the TRAINING forward is out of scope, as in blip_retrieval.evaluate."""
    model.eval()
    pairs = _ClipPairs(model)
    texts = data_loader.dataset.text
    num_text = len(texts)
    text_embeds, image_embeds, lens = [], [], {"vit": [], "text": []}
    for i in range(0, num_text, text_bs):  # :89-94
        ids = _clip_tokens(model, texts[i:min(num_text, i + text_bs)], device)
        out, _ = model.encode_text(ids, model.space_dict, temperature)
        text_embeds.append(out / out.norm(dim=1, keepdim=True))
        lens["text"].append((ids.shape[0], harness.token_lengths(workloads._traces(model.transformer.resblocks), ids.shape[1])))
    for image, _caption, _img_id in data_loader:  # :98-102
        feat, _ = model.encode_image(require_gpu(image.to(device), "image"), model.space_dict, temperature)
        image_embeds.append(feat / feat.norm(dim=1, keepdim=True))
        lens["vit"].append((image.shape[0], harness.token_lengths(workloads._traces(model.visual.transformer.resblocks), pairs.n0)))
    return ClipEval(torch.cat(image_embeds, 0).contiguous(), torch.cat(text_embeds, 0).contiguous(),
                    controller.workload_gflops(pairs, lens), [l for _, l in lens["vit"]], [l for _, l in lens["text"]])
