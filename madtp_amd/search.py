"""Retrieval search on the device (include/madtp_search.h, csrc/search.hip): the top-k gallery items of every query.

    values, indices = search.topk_embeds(q, keys, k)     # f32 [nq,D] x f32 [nk,D] -> f32 [nq,k], int64 [nq,k]; no [nq,nk] matrix
    values, indices = search.topk_scores(scores, k)      # the same selection on a given dense f32 [nq,nk] matrix
    index = search.EmbeddingIndex(keys)                  # a gallery and its workspace, kept across calls
    values, indices = index.search(q, k);  index.add(more_keys)

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


def topk_embeds(q, keys, k):
    """(values f32 [nq,k], indices int64 [nq,k]) of the k largest <q_r, keys_j> per row, best first (madtp_topk_embeds).  Rows may
    be strided (unit stride in the last dimension)."""
    return _topk_embeds(q, keys, k)[:2]


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
    (the storage doubles when it is full, so n adds copy O(n) rows); search() is topk_embeds over the rows held so far."""

    def __init__(self, keys):
        hip._rank_rows(keys, "EmbeddingIndex: keys")
        self._store = keys.contiguous().clone()
        self._n = keys.shape[0]
        self._ws = None

    def __len__(self):
        return self._n

    @property
    def keys(self):
        return self._store[:self._n]

    def add(self, keys):
        hip._rank_rows(keys, "EmbeddingIndex.add: keys")
        if keys.shape[1] != self._store.shape[1] or keys.device != self._store.device:
            raise RuntimeError("EmbeddingIndex.add: the rows disagree with the gallery on the feature dimension or the device")
        n = self._n + keys.shape[0]
        if n > self._store.shape[0]:
            grown = torch.empty(max(n, 2 * self._store.shape[0]), self._store.shape[1], dtype=torch.float32, device=self._store.device)
            grown[:self._n] = self._store[:self._n]
            self._store = grown
        self._store[self._n:n] = keys
        self._n = n
        return self

    def search(self, q, k):
        values, indices, self._ws = _topk_embeds(q, self.keys, k, self._ws)
        return values, indices
