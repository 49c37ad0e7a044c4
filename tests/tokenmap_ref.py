"""The token map restated in numpy and float64, from the definitions of csrc/madtp_tokenmap.h and not from the kernel: a pruned layer
with input length n_in and k kept tokens has k + 1 slots, slot i < k holds input position indices[b, i], slot k is the merged token
over indices_sort[b, k:n_in] with the weights score_j / (sum of the pruned scores + 1e-8); an unpruned layer is the identity.  Shared
by tests/test_tokenmap_cpu.py and tests/test_tokenmap_gpu.py, with the seeded records both run on."""
import numpy as np

EPS = float(np.float32(1e-8))  # the constant as the f32 kernels hold it

# (B, n0, L) of every test, and per shape the k of each layer (None: the layer did not prune).  Between them: an unpruned layer in the
# middle (63, 65, 196, 900), k = 1 (3, 63, 65), n_in - k = 2 (3: 3 -> 1, 64: 64 -> 62 and 31 -> 29, 65: 45 -> 43, 900: 301 -> 299), a merged slot kept by the next layer
# and one merged again (forced by the scores, see records()), a pruned set whose scores are all 0 (64, layer 1), samples with
# different orders (every B > 1: the scores are per sample; 65 and 196 also shuffle the slot order of indices), record tensors wider
# than k (63, 196, 900), more than 256 positions (900: every lane owns several), n0 + 1 not a multiple of anything.
SHAPES = [(1, 3, 1), (2, 63, 3), (3, 64, 4), (2, 65, 5), (2, 196, 12), (1, 900, 12)]
KS = {
    (1, 3, 1): [1],
    (2, 63, 3): [40, None, 1],
    (3, 64, 4): [62, 30, 29, 5],
    (2, 65, 5): [44, 43, None, 17, 1],
    (2, 196, 12): [150, 134, 115, None, 102, 87, 77, 75, None, 73, 71, 60],
    (1, 900, 12): [700, 640, None, 500, 498, 300, 299, 258, 255, 130, 64, 63],
}
WIDE = {(2, 63, 3), (2, 196, 12), (1, 900, 12)}      # indices / indices_sort / score are [B, n0] buffers, the first columns count
SHUFFLED = {(2, 65, 5), (2, 196, 12)}                # indices in a seeded order instead of ascending
ZERO_LAYER = {(3, 64, 4): 1}                         # the layer whose pruned scores are all 0


def scores(shape, l, n, rng):
    """f32 [B, n]: positive scores; the merged slot of the layer before (the last position) ranks first in even layers (it is kept)
    and last in odd ones (it is merged again)"""
    B = shape[0]
    s = rng.random((B, n), dtype=np.float32) + np.float32(0.05)
    if l > 0:
        s[:, n - 1] = np.float32(9.0) if l % 2 == 0 else np.float32(0.01)
    return s


def select(score, k, zero_pruned=False):
    """What madtp_token_select returns for one layer, restated: the stable descending order, the kept positions ascending.
    zero_pruned: the scores of the pruned positions are set to 0 first (they still rank last: every other score is positive).
    -> (score, indices [B, k], indices_sort [B, n])"""
    order = np.argsort(-score.astype(np.float64), axis=1, kind="stable")
    if zero_pruned:
        score = score.copy()
        np.put_along_axis(score, order[:, k:], np.float32(0), axis=1)
        order = np.argsort(-score.astype(np.float64), axis=1, kind="stable")  # (the zeros tie: lower position first)
    return score, np.sort(order[:, :k], axis=1).astype(np.int64), order.astype(np.int64)


def records(shape, seed=0):
    """seeded numpy records of one shape, as the product path's select would leave them (tests on the GPU make theirs with the
    kernels and use only KS / WIDE / SHUFFLED / ZERO_LAYER and scores())"""
    B, n0, L = shape
    rng = np.random.default_rng(1000 * n0 + seed)
    out, n = [], n0
    for l, k in enumerate(KS[shape]):
        if k is None:
            out.append(None)
            continue
        sc, ind, srt = select(scores(shape, l, n, rng), k, ZERO_LAYER.get(shape) == l)
        out.append(pack(shape, sc, ind, srt, k, n, rng))
        n = k + 1
    return out


def pack(shape, sc, ind, srt, k, n, rng):
    """one layer's record dict: shuffled slot order and wide buffers where the shape asks for them"""
    B, n0, _ = shape
    if shape in SHUFFLED:
        ind = np.stack([r[rng.permutation(k)] for r in ind])
    if shape in WIDE:
        wide = lambda a, fill: np.concatenate([a, np.full((B, n0 - a.shape[1]), fill, a.dtype)], axis=1)
        ind, srt, sc = wide(ind, -1), wide(srt, 1 << 40), wide(sc, np.float32(np.nan))
    return {"pruned": True, "k": k, "indices": np.ascontiguousarray(ind), "indices_sort": np.ascontiguousarray(srt),
            "score": np.ascontiguousarray(sc)}


def compose(recs, n0):
    """-> dict(slot int [B, L, n0], coef f64 [B, L, n0], depth int [B, n0], n_out [L], pruned [L]).  A record without
    'indices_sort' merges the complement of indices; without 'score' the coef of a merged position is NaN (the reference's recorded
    traces hold the indices only)."""
    L = len(recs)
    B = next(int(np.asarray(r["indices"]).shape[0]) for r in recs if r is not None and r.get("pruned"))
    slot, coef = np.zeros((B, L, n0), np.int64), np.zeros((B, L, n0), np.float64)
    depth, n_out, pruned = np.zeros((B, n0), np.int64), [], []
    cur_s, cur_c = np.tile(np.arange(n0), (B, 1)), np.ones((B, n0))
    alone = np.ones((B, n0), bool)
    n = n0
    for l, rec in enumerate(recs):
        if rec is None or not rec.get("pruned"):
            pruned.append(False)
        else:
            pruned.append(True)
            ind = np.asarray(rec["indices"])
            k = int(rec.get("k", ind.shape[1]))
            assert 1 <= k < n, (l, k, n)
            for b in range(B):
                kept = ind[b, :k]
                merged = np.asarray(rec["indices_sort"])[b, k:n] if rec.get("indices_sort") is not None else np.setdiff1d(np.arange(n), kept)
                assert sorted(np.concatenate([kept, merged]).tolist()) == list(range(n)), (l, b)
                new_slot, w = np.full(n, k), np.ones(n)
                new_slot[kept] = np.arange(k)
                if rec.get("score") is not None:
                    s = np.asarray(rec["score"])[b, :n].astype(np.float64)
                    w[merged] = s[merged] / (s[merged].sum() + EPS)
                else:
                    w[merged] = np.nan
                cur_c[b] = cur_c[b] * w[cur_s[b]]
                alone[b] &= new_slot[cur_s[b]] < k
                cur_s[b] = new_slot[cur_s[b]]
            n = k + 1
        slot[:, l], coef[:, l] = cur_s, cur_c
        depth[alone] = l + 1
        n_out.append(n)
    return {"slot": slot, "coef": coef, "depth": depth, "n_out": n_out, "pruned": pruned}


def kept_sets(depth, l):
    """per sample the set of positions kept at layer l: depth > l"""
    return [set(np.nonzero(row > l)[0].tolist()) for row in np.asarray(depth)]


def push(x, slot, coef, n_out):
    """y[b, s] = sum of coef[b, p] x[b, p] over slot[b, p] == s, in float64"""
    B, n0, C = x.shape
    y = np.zeros((B, n_out, C))
    for b in range(B):
        np.add.at(y[b], slot[b], coef[b][:, None] * x[b].astype(np.float64))
    return y


def push_abs(x, slot, coef, n_out):
    """sum of |coef x| per cell of y, and the number of positions of every slot: what the rounding bound of a push is made of"""
    cells = np.stack([np.bincount(s, minlength=n_out) for s in slot])
    return push(np.abs(x), slot, np.abs(coef), n_out), cells


def pull(v, slot, coef=None):
    out = np.take_along_axis(v, slot[:, :, None], axis=1)
    return out if coef is None else out * coef[:, :, None]


def agree(depth_a, depth_b, L):
    """int [B, L, 2] by set arithmetic"""
    out = np.zeros((len(depth_a), L, 2), np.int64)
    for l in range(L):
        for b, (a, c) in enumerate(zip(kept_sets(depth_a, l), kept_sets(depth_b, l))):
            out[b, l] = len(a & c), len(a | c)
    return out


def shade(images, depth, grid, levels):
    """out = (pix * level[depth[patch]] + 127) // 255 in integers"""
    B, H, W, _ = images.shape
    gh, gw = grid
    lv = np.asarray(levels, np.int64)[np.clip(depth, 0, len(levels) - 1)].reshape(B, gh, gw)
    lv = np.repeat(np.repeat(lv, H // gh, axis=1), W // gw, axis=2)[..., None]
    return ((images.astype(np.int64) * lv + 127) // 255).astype(np.uint8)
