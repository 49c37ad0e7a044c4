"""numpy restatement of include/madtp_lists.h: the dense row a candidate list stands for, the rank rule on that row, and the sort
as np.lexsort with the contract's keys (madtp_search.h)."""
import numpy as np


def held(idx, nk):
    return (idx >= 0) & (idx < nk)


def to_dense(idx, val, nk, fill=-100.0):
    """idx int64 [n,k], val f32 [n,k] -> f32 [n,nk]: val of the slot that holds j, fill for a key in no slot"""
    idx, val = np.asarray(idx), np.asarray(val, dtype=np.float32)
    dense = np.full((idx.shape[0], nk), fill, dtype=np.float32)
    for r in range(idx.shape[0]):
        m = held(idx[r], nk)
        dense[r, idx[r][m]] = val[r][m]
    return dense


def rank_in_row(row, t):
    """rank(t) = #{j != t : s_j > s_t} + #{j > t : s_j == s_t}, IEEE comparisons (a NaN on either side counts nothing)"""
    j = np.arange(row.shape[0])
    with np.errstate(invalid="ignore"):
        return int(((row > row[t]) & (j != t)).sum() + ((row == row[t]) & (j > t)).sum())


def ranks(dense, tgt_ptr, tgt_idx):
    """(rank_row, rank_tgt) int32 of CSR targets on dense rows: nk for a target outside [0, nk) and for a row without targets"""
    n, nk = dense.shape
    rank_row = np.full(n, nk, dtype=np.int32)
    rank_tgt = np.full(len(tgt_idx), nk, dtype=np.int32)
    for r in range(n):
        for p in range(tgt_ptr[r], tgt_ptr[r + 1]):
            if 0 <= tgt_idx[p] < nk:
                rank_tgt[p] = rank_in_row(dense[r], int(tgt_idx[p]))
                rank_row[r] = min(rank_row[r], rank_tgt[p])
    return rank_row, rank_tgt


def sort(idx, val, nk):
    """every row best first: filled before empty, numbers before NaN, value descending (-0 = +0), key index descending; empty
    slots come out as (-1, -inf).  -> (idx int64 [n,k], val f32 [n,k]) with the input's value bits"""
    idx, val = np.asarray(idx), np.asarray(val, dtype=np.float32)
    out_idx, out_val = np.full_like(idx, -1), np.full_like(val, -np.inf)
    for r in range(idx.shape[0]):
        m = held(idx[r], nk)
        v = np.where(val[r] == 0, np.float32(0), val[r]).astype(np.float64)
        nan = np.isnan(v)
        # np.lexsort: the LAST key is the primary one
        order = np.lexsort((-idx[r], np.where(nan, 0.0, -v), nan, ~m))
        cnt = int(m.sum())
        out_idx[r, :cnt] = idx[r][order][:cnt]
        out_val[r, :cnt] = val[r][order][:cnt]
    return out_idx, out_val
