"""madtp_lists_rank and madtp_lists_sort on a real MI355X (madtp_amd/lists.py): the ranks against madtp_rank_scores on the dense
rows the lists stand for and against the numpy restatement (tests/lists_ref.py), the order against the restatement's lexsort.
Everything is compared for equality: integer ranks, key indices, and values that are copies of the input's."""
import functools

import numpy as np
import pytest
import torch

from tests import lists_ref

pytestmark = pytest.mark.gpu
SHAPES = [(3, 1, 2), (5, 4, 4), (7, 4, 5), (33, 64, 257), (65, 256, 1285), (4, 256, 256)]
SPECIALS = np.array([-100.0, -150.0, 0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)


def _lib():
    from madtp_amd import build, hip
    build.build(verbose=False)
    hip.load()


@functools.lru_cache(maxsize=None)
def _case(n, k, nk, nan=True):
    """-> (idx [n,k], val [n,k], tgt_ptr, tgt_idx) as numpy arrays.  Scores are integers from a range of 5 (ties everywhere) with
    -100 (the fill), a value below it, both zeros, both infinities and NaN planted in one slot in eight; row 0 has every slot it can
    fill filled, the last row none, the others lose a slot in five.  Rows take 1 and 16 targets in turn (nk at most): key 0, key
    nk - 1, a key in a slot, a key in none where there is one, then random keys; the first row also names a key outside [0, nk)."""
    rng = np.random.RandomState(1000 * n + 10 * k + nk % 7)
    idx = np.full((n, k), -1, dtype=np.int64)
    val = rng.randint(0, 5, (n, k)).astype(np.float32)
    specials = SPECIALS if nan else SPECIALS[:-1]
    plant = rng.rand(n, k) < 0.125
    val[plant] = specials[rng.randint(0, len(specials), int(plant.sum()))]
    ptr, tgt = [0], []
    for r in range(n):
        m = min(k, nk)
        slots = rng.permutation(k)[:m]  # (filled slots are anywhere in the row, not in front)
        idx[r, slots] = rng.permutation(nk)[:m]
        if r == n - 1 and n > 1:
            idx[r] = -1
        elif r > 0:
            idx[r, rng.rand(k) < 0.2] = -1
        held = idx[r][idx[r] >= 0]
        free = np.setdiff1d(np.arange(nk), held)
        want = 1 if r % 2 == 0 else min(16, nk)
        pool = [0, nk - 1] + ([int(held[0])] if len(held) else []) + ([int(free[len(free) // 2])] if len(free) else [])
        pool = pool[r % len(pool):] + pool[:r % len(pool)] + rng.permutation(nk).tolist()
        row = list(dict.fromkeys(pool))[:want]
        if r == 0 and want < 16:
            row.append(nk)  # out of range: reported as rank nk, and no minimum
        tgt += row
        ptr.append(len(tgt))
    return idx, val, np.array(ptr, dtype=np.int32), np.array(tgt, dtype=np.int32)


def _lists(idx, val, nk):
    """CandidateLists on the device whose val is a strided view (rows k + 3 apart)"""
    from madtp_amd import lists
    n, k = idx.shape
    wide = torch.full((n, k + 3), 777.0, device="cuda")
    wide[:, :k] = torch.from_numpy(val).cuda()
    return lists.CandidateLists(torch.from_numpy(idx).cuda(), wide[:, :k], nk)


def _same_values(a, b):
    """equality of f32 tensors with NaN equal to NaN (and -0 equal to +0)"""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("n,k,nk", SHAPES)
def test_rank_equals_the_dense_kernel_and_the_restatement(n, k, nk):
    from madtp_amd import retrieval_eval
    _lib()
    idx, val, ptr, tgt = _case(n, k, nk)
    assert np.isnan(val).any() or n * k < 64
    cl = _lists(idx, val, nk)
    assert cl.val.stride(0) == k + 3 and cl.validate() is cl
    dptr, dtgt = torch.from_numpy(ptr).cuda(), torch.from_numpy(tgt).cuda()
    rank_row, rank_tgt = cl.rank(dptr, dtgt)
    dense = cl.to_dense()
    assert np.array_equal(dense.cpu().numpy(), lists_ref.to_dense(idx, val, nk), equal_nan=True)
    want_row, want_tgt = retrieval_eval.rank_scores(dense, dptr, dtgt)
    assert torch.equal(rank_tgt, want_tgt) and torch.equal(rank_row, want_row)
    ref_row, ref_tgt = lists_ref.ranks(lists_ref.to_dense(idx, val, nk), ptr, tgt)
    assert torch.equal(rank_tgt.cpu(), torch.from_numpy(ref_tgt)) and torch.equal(rank_row.cpu(), torch.from_numpy(ref_row))
    # the row of empty slots only: every key scores the fill, so key t has the nk - 1 - t keys above it before it
    if n > 1:
        last = slice(ptr[n - 1], ptr[n])
        assert rank_tgt[last].cpu().tolist() == [nk - 1 - t for t in tgt[last]]
    # two identical calls, identical bits
    again_row, again_tgt = cl.rank(dptr, dtgt)
    assert torch.equal(again_row, rank_row) and torch.equal(again_tgt, rank_tgt)


def test_rank_without_targets_and_with_another_fill():
    from madtp_amd import lists, retrieval_eval
    _lib()
    idx, val, ptr, tgt = _case(7, 4, 5)
    cl = _lists(idx, val, 5)
    none = cl.rank(torch.zeros(8, dtype=torch.int32, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"))
    assert none[0].tolist() == [5] * 7 and none[1].numel() == 0
    dptr, dtgt = torch.from_numpy(ptr).cuda(), torch.from_numpy(tgt).cuda()
    for fill in (2.0, float("inf"), float("-inf"), float("nan"), 0.0):  # a fill inside the scores' range ties with slots
        other = lists.CandidateLists(cl.idx, cl.val, 5, fill=fill)
        got, want = other.rank(dptr, dtgt), retrieval_eval.rank_scores(other.to_dense(), dptr, dtgt)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), fill


@pytest.mark.parametrize("n,k,nk", SHAPES + [(9, 2, 40), (9, 3, 40), (17, 65, 300)])
def test_sort_equals_the_restatement(n, k, nk):
    _lib()
    idx, val, _, _ = _case(n, k, nk)
    cl = _lists(idx, val, nk)
    s = cl.sorted()
    want_idx, want_val = lists_ref.sort(idx, val, nk)
    assert s.idx.dtype == torch.int64 and s.val.dtype == torch.float32 and s.nk == nk and s.fill == cl.fill
    assert torch.equal(s.idx.cpu(), torch.from_numpy(want_idx))
    assert _same_values(s.val.cpu(), torch.from_numpy(want_val))
    assert not torch.signbit(s.val[s.val == 0]).any()  # a zero comes out as +0
    again = cl.sorted()
    assert torch.equal(again.idx, s.idx) and torch.equal(again.val.view(torch.int32), s.val.view(torch.int32))
    r = max(1, k // 2)
    top = cl.top(r)
    assert top.shape == (n, r) and torch.equal(top.idx, s.idx[:, :r]) and _same_values(top.val, s.val[:, :r])
    assert torch.equal(cl.idx.cpu(), torch.from_numpy(idx))  # the input is left as it was


def test_sort_orders_equal_values_by_index_descending():
    from madtp_amd import lists
    _lib()
    for k in (1, 2, 3, 64, 65, 256):
        g = torch.Generator().manual_seed(k)
        idx = torch.stack([torch.randperm(1000, generator=g)[:k] for _ in range(3)])
        s = lists.CandidateLists(idx.cuda(), torch.full((3, k), 2.5, device="cuda"), 1000).sorted()
        assert torch.equal(s.idx.cpu(), idx.sort(dim=1, descending=True).values) and (s.val == 2.5).all()


@pytest.mark.parametrize("n,k,nk", [(7, 4, 5), (33, 64, 257), (65, 256, 1285)])
def test_a_target_above_the_fill_sits_at_its_rank(n, k, nk):
    """the cross-check of the two kernels on NaN-free rows: position rank of .sorted() holds the target"""
    _lib()
    idx, val, ptr, tgt = _case(n, k, nk, nan=False)
    assert not np.isnan(val).any()
    cl = _lists(idx, val, nk)
    _, rank_tgt = cl.rank(torch.from_numpy(ptr).cuda(), torch.from_numpy(tgt).cuda())
    s, rank_tgt = cl.sorted().idx.cpu().numpy(), rank_tgt.cpu().numpy()
    checked = 0
    for r in range(n):
        for p in range(ptr[r], ptr[r + 1]):
            slot = np.where(idx[r] == tgt[p])[0]
            if len(slot) and val[r, slot[0]] > -100.0:
                assert rank_tgt[p] < k and s[r, rank_tgt[p]] == tgt[p], (r, p)
                checked += 1
    assert checked >= n // 2


def test_validate_names_the_row():
    from madtp_amd import lists
    _lib()
    idx, val, _, _ = _case(33, 64, 257)
    twice = idx.copy()
    row = np.where(twice[3] >= 0)[0]
    twice[3, row[5]] = twice[3, row[1]]
    with pytest.raises(ValueError, match=f"row 3 holds key {twice[3, row[1]]} twice"):
        _lists(twice, val, 257).validate()
    beyond = idx.copy()
    beyond[2, 7] = 257
    beyond[9, 0] = 300
    with pytest.raises(ValueError, match="row 2 holds index 257 outside"):
        _lists(beyond, val, 257).validate()
    with pytest.raises(ValueError, match="k = 300"):
        lists.CandidateLists(torch.zeros(2, 300, dtype=torch.int64, device="cuda"), torch.zeros(2, 300, device="cuda"), 1000)
