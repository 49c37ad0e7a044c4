"""The retrieval rank rule restated on the host in float64, and the seeded inputs of the retrieval-evaluation tests.

rank of target t in a row of scores s = #{j != t : s_j > s_t} + #{j > t : s_j == s_t}: the position of t in
np.argsort(s, kind="stable")[::-1].  (A stable ascending sort keeps equal scores in index order; reversed, the larger index
comes first.)"""
import numpy as np
import torch
import torch.nn.functional as F


def positions(row):
    """position of every column in argsort(row, kind='stable')[::-1]"""
    order = np.argsort(np.asarray(row), kind="stable")[::-1]
    pos = np.empty(len(order), dtype=np.int64)
    pos[order] = np.arange(len(order))
    return pos


def csr(lists):
    """list of target lists -> (ptr, idx) int32 arrays"""
    ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    idx = np.array([t for x in lists for t in x], dtype=np.int32)
    return ptr, idx


def ranks(scores, lists):
    """(rank_row [nq], rank_tgt [n_targets]) of a score matrix [nq, nk] for per-row target lists; a row without a target: nk"""
    nq, nk = scores.shape
    rank_row = np.full(nq, nk, dtype=np.int64)
    rank_tgt = []
    for r in range(nq):
        pos = positions(scores[r])
        for t in lists[r]:
            rank_tgt.append(int(pos[t]))
            rank_row[r] = min(rank_row[r], int(pos[t]))
    return rank_row, np.array(rank_tgt, dtype=np.int64)


def recall_dict(ranks_i2t, ranks_t2i):
    def r_at(rk, k):
        return 100.0 * len(np.where(rk < k)[0]) / len(rk)
    tr1, tr5, tr10 = (r_at(ranks_i2t, k) for k in (1, 5, 10))
    ir1, ir5, ir10 = (r_at(ranks_t2i, k) for k in (1, 5, 10))
    tr_mean = (tr1 + tr5 + tr10) / 3
    ir_mean = (ir1 + ir5 + ir10) / 3
    return {"txt_r1": tr1, "txt_r5": tr5, "txt_r10": tr10, "txt_r_mean": tr_mean, "img_r1": ir1, "img_r5": ir5, "img_r10": ir10,
            "img_r_mean": ir_mean, "r_mean": (tr_mean + ir_mean) / 2}


def itm_eval(scores_i2t, scores_t2i, txt2img, img2txt):
    """recall@1/5/10 in both directions from two score matrices, ties by the rule above"""
    n_img, n_txt = scores_i2t.shape
    ri, _ = ranks(scores_i2t, [list(img2txt[i]) for i in range(n_img)])
    rt, _ = ranks(scores_t2i, [[int(txt2img[j])] for j in range(n_txt)])
    return recall_dict(ri, rt)


def pairing(n_img, cap):
    """caption j belongs to image j // cap"""
    img2txt = [list(range(i * cap, (i + 1) * cap)) for i in range(n_img)]
    txt2img = [j // cap for j in range(n_img * cap)]
    return txt2img, img2txt


def exact_features(n_img, cap, D, seed=0):
    """Entries k / 8 with k in -4 .. 4; caption j copies its image on a random 0.05 (1 + j % 4) share of the features.  Every dot
    product is a multiple of 1 / 64 below 2^8: exact in f32 in any summation order, with frequent ties."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(-4, 5, (n_img, D), generator=g).float() / 8
    txt = torch.randint(-4, 5, (n_img * cap, D), generator=g).float() / 8
    for j in range(n_img * cap):
        m = torch.rand(D, generator=g) < 0.05 * (1 + j % 4)
        txt[j, m] = img[j // cap, m]
    return img, txt


LEVELS = [2, 8, 16, 30, 60]


def realistic_features(n_img, cap, D, seed=7):
    """unit-norm image features; caption j = normalize(img + lvl randn / sqrt(D)) with the noise level cycling over LEVELS"""
    g = torch.Generator().manual_seed(seed)
    img = F.normalize(torch.randn(n_img, D, generator=g, dtype=torch.float64), dim=-1)
    j = torch.arange(n_img * cap)
    lvl = torch.tensor(LEVELS, dtype=torch.float64)[torch.clamp((j % cap) + (j // cap) % 5, max=4)]
    noise = torch.randn(n_img * cap, D, generator=g, dtype=torch.float64) / D ** 0.5
    txt = F.normalize(img[j // cap] + lvl[:, None] * noise, dim=-1)
    return img.float(), txt.float()
