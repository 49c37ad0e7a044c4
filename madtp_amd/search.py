"""Retrieval search on the device (include/madtp_search.h, csrc/search.hip): the top-k gallery items of every query.

    values, indices = search.topk_embeds(q, keys, k)     # f32 [nq,D] x f32 [nk,D] -> f32 [nq,k], int64 [nq,k]; no [nq,nk] matrix
    values, indices = search.topk_scores(scores, k)      # the same selection on a given dense f32 [nq,nk] matrix
    index = search.EmbeddingIndex(keys)                  # a gallery and its workspace, kept across calls
    values, indices = index.search(q, k);  index.add(more_keys)
    values, indices = search.topk_embeds(q, keys, k, coarse="bf16")   # the same bits through a certified bf16 shortlist, k <= 128
    index = search.EmbeddingIndex(keys, coarse="bf16")   # ... with the gallery's bf16 rows and statistics kept

Order (the contract of the header): score descending, equal scores by key index descending - position p of a row is element p of
np.argsort(s, kind="stable")[::-1], the rule of retrieval_eval.rank_embeds, whose score_tgt bits the values are.  NaN ranks below
every number; for k > nk the tail of a row is index -1, value -inf.  1 <= k <= MAX_K, D % 64 == 0, 64 <= D <= 1024.  Device
tensors only: a CPU tensor raises, there is no fallback."""
import os

import torch

from . import abi, hip

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_search.h")
# the one declaration of the search entry points; lib() is hip.load()'s handle with them set on it (no GPU needed)
SIGNATURES, DEFINES, lib = abi.bind("madtp_search.h", "madtp_search_abi_version")
ABI_VERSION = DEFINES["MADTP_SEARCH_ABI_VERSION"]
MAX_K = DEFINES["MADTP_TOPK_MAX_K"]
# the coarse route (include/madtp_csearch.h, csrc/search_coarse.hip); clib() is the same handle with its entry points set as well
CSIGNATURES, CDEFINES, clib = abi.bind("madtp_csearch.h", "madtp_csearch_abi_version", needs=lib)
COARSE_ABI_VERSION = CDEFINES["MADTP_CSEARCH_ABI_VERSION"]
COARSE_MAX_K = CDEFINES["MADTP_CTOPK_MAX_K"]
COARSE_ACC_FACTOR = CDEFINES["MADTP_CTOPK_ACC_FACTOR"]
SHORTLISTS = (64, 128, 256)

def _check_k(k, what):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k = {k} outside [1, {MAX_K}]")
    return k


def _rows16(t, name):
    """a GPU f32 row-major 2-D view the kernels can read in place (16-byte aligned rows), else its contiguous copy -> (t, ld)"""
    ld = hip._rank_rows(t, name)
    if ld % 4 != 0 or t.data_ptr() % 16 != 0:
        t = t.contiguous()
        ld = t.shape[1]
    return t, ld


def _topk_embeds(q, keys, k, ws=None):
    k = _check_k(k, "topk_embeds")
    (q, ldq), (keys, ldk) = _rows16(q, "topk_embeds: q"), _rows16(keys, "topk_embeds: keys")
    nq, D = q.shape
    nk = keys.shape[0]
    if keys.shape[1] != D or keys.device != q.device:
        raise RuntimeError("topk_embeds: q and keys disagree on the feature dimension or the device")
    if D % 64 != 0 or not 64 <= D <= 1024:
        raise ValueError(f"topk_embeds: D = {D} must be a multiple of 64 in [64, 1024]")
    h = lib()
    need = int(h.madtp_topk_workspace(nq, nk, D, k))
    if ws is None or ws.numel() * 8 < need or ws.device != q.device:
        ws = torch.empty(need // 8, dtype=torch.int64, device=q.device)
    values = torch.empty(nq, k, dtype=torch.float32, device=q.device)
    indices = torch.empty(nq, k, dtype=torch.int32, device=q.device)
    with torch.cuda.device(q.device):
        hip._check(h.madtp_topk_embeds(q.data_ptr(), ldq, keys.data_ptr(), ldk, nq, nk, D, k, values.data_ptr(), indices.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 8, hip._stream()), "madtp_topk_embeds")
    return values, indices.long(), ws


def check_coarse(coarse, k, what, shortlist=None):
    """-> the shortlist size m of a coarse search, or a ValueError for what the coarse route does not take (before any GPU use)"""
    if coarse != "bf16":
        raise ValueError(f"{what}: coarse = {coarse!r}: expected None or 'bf16'")
    k = int(k)
    if not 1 <= k <= COARSE_MAX_K:
        raise ValueError(f"{what}: k = {k} outside [1, {COARSE_MAX_K}] of the coarse route (coarse=None takes k up to {MAX_K})")
    if shortlist is None:
        return next(m for m in SHORTLISTS if m >= 2 * k)
    m = int(shortlist)
    if m not in SHORTLISTS or m < 2 * k:
        raise ValueError(f"{what}: shortlist = {m}: expected one of {SHORTLISTS} and at least 2 k = {2 * k}")
    return m


def _check_D(D, what):
    if D % 64 != 0 or not 64 <= D <= 1024:
        raise ValueError(f"{what}: D = {D} must be a multiple of 64 in [64, 1024]")


def prepare(x, out16=None, out_stats=None):
    """f32 rows [n,D] -> (bf16 rows [n,D], round to nearest even; statistics f32 [n,4] = |x|, |x - x16|, |x16| rounded up, and the
    flag of a row no certificate may rest on) - madtp_coarse_prepare.  out16 / out_stats: contiguous row slices to write into."""
    x, ld = _rows16(x, "prepare: x")
    n, D = x.shape
    _check_D(D, "prepare")
    x16 = torch.empty(n, D, dtype=torch.bfloat16, device=x.device) if out16 is None else out16
    stats = torch.empty(n, 4, dtype=torch.float32, device=x.device) if out_stats is None else out_stats
    with torch.cuda.device(x.device):
        hip._check(clib().madtp_coarse_prepare(x.data_ptr(), ld, n, D, x16.data_ptr(), stats.data_ptr(), hip._stream()),
                   "madtp_coarse_prepare")
    return x16, stats


def summary(stats, out=None):
    """statistics [n,4] -> the gallery summary f32 [4] = (Y, dY, Y16, flag), their column maxima (madtp_coarse_summary).  With
    `out`, an existing summary, the maximum also runs over it: rows appended to a gallery are folded in."""
    fold = out is not None
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=stats.device)
    with torch.cuda.device(stats.device):
        hip._check(clib().madtp_coarse_summary(stats.data_ptr(), stats.shape[0], out.data_ptr(), int(fold), hip._stream()),
                   "madtp_coarse_summary")
    return out


class SearchInfo:
    """What a coarse search reports per query row.  Device tensors; nothing here synchronises but n_fallback / fallback_rows.
        certified          bool [nq]     the exact top-k was proven to lie inside the shortlist
        threshold          f32 [nq]      c_m, the m-th best coarse score (-inf when fewer than m keys exist)
        bound              f32 [nq]      E_r of include/madtp_csearch.h
        fallback_position  int32 [nq]    the row's place in the list of rows the exact route took, or -1
        shortlist_indices  int64 [nq,m]  the shortlist, best coarse score first (-1 past the last key)
        shortlist_coarse   f32 [nq,m]    its coarse scores (-inf there)"""

    def __init__(self, info, sl_idx, sl_coarse, count):
        self.certified = info[:, 0] != 0
        self.threshold = info[:, 1].view(torch.float32)
        self.bound = info[:, 2].view(torch.float32)
        self.fallback_position = info[:, 3]
        self.shortlist_indices = sl_idx.long()
        self.shortlist_coarse = sl_coarse
        self._count = count

    @property
    def n_fallback(self):
        """the number of rows the exact route took (a device-to-host copy: this synchronises)"""
        return int(self._count.item())

    @property
    def fallback_rows(self):
        """the ascending list of those rows, int64 (synchronises)"""
        pos = self.fallback_position
        rows = torch.nonzero(pos >= 0).flatten()
        return rows[torch.argsort(pos[rows])]


def _ctopk_embeds(q, keys, k, m, gallery=None, ws=None, return_info=False):
    """gallery: (keys16, summary) of `keys` from prepare() / summary(), made here when absent"""
    (q, ldq), (keys, ldk) = _rows16(q, "topk_embeds: q"), _rows16(keys, "topk_embeds: keys")
    nq, D = q.shape
    nk = keys.shape[0]
    if keys.shape[1] != D or keys.device != q.device:
        raise RuntimeError("topk_embeds: q and keys disagree on the feature dimension or the device")
    _check_D(D, "topk_embeds")
    h = clib()
    if gallery is None:
        keys16, kstats = prepare(keys)
        gallery = (keys16, summary(kstats))
    keys16, ksum = gallery
    need = int(h.madtp_ctopk_workspace(nq, nk, D, k, m))
    if ws is None or ws.numel() * 8 < need or ws.device != q.device:
        ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=q.device)
    values = torch.empty(nq, k, dtype=torch.float32, device=q.device)
    indices = torch.empty(nq, k, dtype=torch.int32, device=q.device)
    info = torch.empty(nq, 4, dtype=torch.int32, device=q.device)
    sl_idx = torch.empty(nq, m, dtype=torch.int32, device=q.device) if return_info else None
    sl_coarse = torch.empty(nq, m, dtype=torch.float32, device=q.device) if return_info else None
    with torch.cuda.device(q.device):
        hip._check(h.madtp_ctopk_embeds(q.data_ptr(), ldq, keys.data_ptr(), ldk, keys16.data_ptr(), ksum.data_ptr(), nq, nk, D, k, m,
                                        values.data_ptr(), indices.data_ptr(), info.data_ptr(),
                                        sl_idx.data_ptr() if return_info else None, sl_coarse.data_ptr() if return_info else None,
                                        ws.data_ptr(), ws.numel() * 8, hip._stream()), "madtp_ctopk_embeds")
    out = (values, indices.long())
    if return_info:  # (the count is copied on the stream: the workspace may serve the next call)
        out += (SearchInfo(info, sl_idx, sl_coarse, ws[:1].view(torch.int32)[:1].clone()),)
    return out, ws


def topk_embeds(q, keys, k, coarse=None, shortlist=None, return_info=False):
    """(values f32 [nq,k], indices int64 [nq,k]) of the k largest <q_r, keys_j> per row, best first (madtp_topk_embeds).  Rows may
    be strided (unit stride in the last dimension).
    coarse="bf16" (include/madtp_csearch.h): the same values and indices, bit for bit, by another route - a shortlist of
    `shortlist` keys per row (64, 128 or 256, at least 2 k; the default is the smallest) from bf16 scores, scored again exactly;
    rows whose certificate fails go through the exact kernels in the same call.  k <= COARSE_MAX_K.  return_info=True appends a
    SearchInfo."""
    if coarse is None:
        if shortlist is not None or return_info:
            raise ValueError("topk_embeds: shortlist= and return_info= belong to coarse='bf16'")
        return _topk_embeds(q, keys, k)[:2]
    m = check_coarse(coarse, k, "topk_embeds", shortlist)
    return _ctopk_embeds(q, keys, int(k), m, return_info=return_info)[0]


def coarse_bound(q, keys):
    """E_r of include/madtp_csearch.h restated on the host in float64, f64 [nq]: for every key j, the exact route's score of
    (r, j) and the coarse stage's differ by at most E_r.  (The device evaluates the same expression in f32 from statistics it
    rounded up, so its bound is this one or slightly more.)"""
    q, keys = q.detach().cpu().float(), keys.detach().cpu().float()
    D = q.shape[1]
    q16, k16 = q.bfloat16().double(), keys.bfloat16().double()
    qd, kd = q.double(), keys.double()
    u = 2.0 ** -24
    Y, dY, Y16 = kd.norm(dim=1).max(), (kd - k16).norm(dim=1).max(), k16.norm(dim=1).max()
    a, b, nq_ = (qd - q16).norm(dim=1), q16.norm(dim=1), qd.norm(dim=1)
    E = a * Y + b * dY + (D + 2) * u * nq_ * Y + COARSE_ACC_FACTOR * D * u * b * Y16
    return E * (1 + 2.0 ** -10) + (3 * D + 8) * 2.0 ** -126


def topk_scores(scores, k):
    """The same pair from a dense f32 score matrix [nq,nk] (madtp_topk_scores).  A view whose rows are not contiguous, such as
    sims.t(), is taken from a row-major copy."""
    k = _check_k(k, "topk_scores")
    if torch.is_tensor(scores) and scores.dim() == 2 and scores.stride(-1) != 1 and scores.shape[1] > 1:
        scores = scores.contiguous()
    ld = hip._rank_rows(scores, "topk_scores: scores")
    nq, nk = scores.shape
    values = torch.empty(nq, k, dtype=torch.float32, device=scores.device)
    indices = torch.empty(nq, k, dtype=torch.int32, device=scores.device)
    with torch.cuda.device(scores.device):
        hip._check(lib().madtp_topk_scores(scores.data_ptr(), ld, nq, nk, k, values.data_ptr(), indices.data_ptr(), hip._stream()),
                   "madtp_topk_scores")
    return values, indices.long()


class EmbeddingIndex:
    """A gallery of f32 embeddings [n, D] on the device and the workspace of its searches, kept across calls.  add() appends rows
    (the storage doubles when it is full, so n adds copy O(n) rows); search() is topk_embeds over the rows held so far.
    coarse="bf16": the index also keeps the gallery's bf16 rows and its summary (prepare() / summary()); add() converts the new
    rows alone and folds their statistics in, and search() takes the certified shortlist route."""

    def __init__(self, keys, coarse=None):
        if coarse is not None and coarse != "bf16":
            raise ValueError(f"EmbeddingIndex: coarse = {coarse!r}: expected None or 'bf16'")
        hip._rank_rows(keys, "EmbeddingIndex: keys")
        self._store = keys.contiguous().clone()
        self._n = keys.shape[0]
        self._ws = None
        self._coarse = coarse
        if coarse is not None:
            self._store16, self._stats = prepare(self._store)
            self._summary = summary(self._stats)

    def __len__(self):
        return self._n

    @property
    def keys(self):
        return self._store[:self._n]

    @property
    def coarse_summary(self):
        """f32 [4]: (Y, dY, Y16, flag) of the rows held so far (coarse="bf16")"""
        return self._summary

    def add(self, keys):
        hip._rank_rows(keys, "EmbeddingIndex.add: keys")
        if keys.shape[1] != self._store.shape[1] or keys.device != self._store.device:
            raise RuntimeError("EmbeddingIndex.add: the rows disagree with the gallery on the feature dimension or the device")
        n = self._n + keys.shape[0]
        if n > self._store.shape[0]:
            def grow(old):
                grown = torch.empty(max(n, 2 * old.shape[0]), old.shape[1], dtype=old.dtype, device=old.device)
                grown[:self._n] = old[:self._n]
                return grown
            self._store = grow(self._store)
            if self._coarse is not None:
                self._store16, self._stats = grow(self._store16), grow(self._stats)
        self._store[self._n:n] = keys
        if self._coarse is not None:
            prepare(self._store[self._n:n], self._store16[self._n:n], self._stats[self._n:n])
            summary(self._stats[self._n:n], out=self._summary)
        self._n = n
        return self

    def search(self, q, k, return_info=False):
        if self._coarse is None:
            if return_info:
                raise ValueError("EmbeddingIndex.search: return_info= belongs to coarse='bf16'")
            values, indices, self._ws = _topk_embeds(q, self.keys, k, self._ws)
            return values, indices
        m = check_coarse(self._coarse, k, "EmbeddingIndex.search")
        out, self._ws = _ctopk_embeds(q, self.keys, int(k), m, (self._store16[:self._n], self._summary), self._ws, return_info)
        return out
