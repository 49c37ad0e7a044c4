"""Retrieval search on a real MI355X (csrc/search.hip, madtp_amd/search.py): madtp_topk_embeds / madtp_topk_scores against the
restatement of the order, np.argsort(s, kind="stable")[::-1][:k] on float64 scores (score descending, equal scores by index
descending), and against the shipped ranking kernel, whose rank of a target is its position in that order.

Tolerances.  Exact inputs (small integers: every dot product is an integer below 2^13, exact in f32 in any order): indices and
values must EQUAL the float64 ones.  Realistic inputs (unit-norm rows): position p is pinned to the float64 order where the
float64 gaps to positions p - 1 and p + 1 are >= GAP = 2e-6, the top-k SET where the gap between positions k - 1 and k is; GAP
is the separation tests/test_retrieval_eval_gpu.py uses (10x the f32-vs-float64 score error of such inputs).  The pinned shares
asserted below (95 % of positions, 90 % of boundaries) are no tolerances: they keep the test from skipping its way to green."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GAP = 2e-6


@pytest.fixture(scope="module")
def search():
    from madtp_amd import build, hip, search as s
    build.build(verbose=False)
    hip.load()
    assert torch.cuda.is_available()
    return s


def order_ref(s, k):
    """rows of float64 scores -> (indices int64 [n,k], -1 filled): the contract's order.  NaN below every number, by index
    descending among themselves (np.argsort puts NaN last, so the reversed stable order would put it FIRST: they are split off)."""
    out = np.full((s.shape[0], k), -1, dtype=np.int64)
    for r, row in enumerate(s):
        nan = np.isnan(row)
        numbers = np.flatnonzero(~nan)
        order = np.concatenate([numbers[np.argsort(row[numbers], kind="stable")[::-1]], np.flatnonzero(nan)[::-1]])[:k]
        out[r, :len(order)] = order
    return out


def values_ref(s, idx):
    v = np.full(idx.shape, -np.inf)
    for r in range(idx.shape[0]):
        ok = idx[r] >= 0
        v[r, ok] = s[r, idx[r, ok]]
    return v


def check_exact(s64, values, indices, k, what=""):
    want = order_ref(s64, k)
    got_i, got_v = indices.cpu().numpy(), values.cpu().numpy()
    assert got_i.dtype == np.int64 and got_v.dtype == np.float32 and got_i.shape == got_v.shape == want.shape, what
    assert np.array_equal(got_i, want), what
    assert np.array_equal(got_v.astype(np.float64), values_ref(s64, want), equal_nan=True), what


@functools.lru_cache(maxsize=None)
def exact_inputs(nq, nk, D, seed, lo=-2, hi=3):
    """integer features in [lo, hi): |<q, key>| <= 4 * 1024 = 2^12 - every product and partial sum is an exact f32 integer"""
    rng = np.random.default_rng(seed)
    q = torch.from_numpy(rng.integers(lo, hi, (nq, D)).astype(np.float32))
    keys = torch.from_numpy(rng.integers(lo, hi, (nk, D)).astype(np.float32))
    s64 = (q.double() @ keys.double().t()).numpy()
    assert np.array_equal((q @ keys.t()).numpy().astype(np.float64), s64)  # the recipe: f32 is exact here
    return q, keys, s64


@functools.lru_cache(maxsize=None)
def real_inputs(nq, nk, D):
    rng = np.random.default_rng(7)
    q, keys = rng.standard_normal((nq, D)), rng.standard_normal((nk, D))
    q, keys = q / np.linalg.norm(q, axis=1, keepdims=True), keys / np.linalg.norm(keys, axis=1, keepdims=True)
    q, keys = torch.from_numpy(q.astype(np.float32)), torch.from_numpy(keys.astype(np.float32))
    return q, keys, (q.double() @ keys.double().t()).numpy()


def splits_of(search, nq, nk, D=64, k=1):
    """The key splits the launch uses, read from the library's own workspace size: search.hip sizes it as 8 k bytes x 32 rows x
    min(rowtiles * by_keys, 1023 + rowtiles) with by_keys = min(256, ceil(key tiles / 4)), and launches min(by_keys,
    ceil(1024 / rowtiles)) splits (fewer only where the tiles do not divide).  Valid while the first term is the minimum."""
    rowtiles, tiles = -(-nq // 32), -(-nk // 64)
    by_keys = min(256, -(-tiles // 4))
    assert rowtiles * by_keys <= 1023 + rowtiles and by_keys <= -(-1024 // rowtiles)
    assert search.lib().madtp_topk_workspace(nq, nk, D, k) == 8 * k * 32 * rowtiles * by_keys
    per = -(-tiles // by_keys)
    return -(-tiles // per)


EXACT = [(1, 1, 64, 1),
         (33, 63, 64, 5),        # one row past a 32-row tile, one key short of a column tile
         (33, 65, 128, 64),      # one key past it; k = 64: the last k of the 128-word candidate buffer
         (31, 1285, 768, 256),   # k = 256 (the 512-word buffer), 21 key tiles in 6 splits, frequent ties
         (65, 257, 1024, 10),    # three row tiles, the largest D
         (7, 200, 64, 65),       # k = 65: the first k of the 256-word buffer
         (5, 300, 64, 128),      # its last
         (3, 300, 64, 129)]      # the first k of the 512-word buffer


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s)))
def test_topk_embeds_equals_float64_on_exact_inputs(search, shape):
    nq, nk, D, k = shape
    q, keys, s64 = exact_inputs(nq, nk, D, seed=nq + nk)
    values, indices = search.topk_embeds(q.cuda(), keys.cuda(), k)
    check_exact(s64, values, indices, k, shape)
    ties = sum(len(np.unique(row[np.argsort(row)[::-1][:k]])) < min(k, nk) for row in s64)
    print(f"{shape}: {ties} of {nq} rows tie inside their top {k}")


def test_topk_embeds_splits_leading_dimensions_and_fill(search):
    # at least three key splits: 33 rows are 2 row tiles, 1285 keys are 21 tiles -> 6 splits (see splits_of)
    assert splits_of(search, 33, 1285) == 6 and splits_of(search, 5, 20000) == 79
    q, keys, s64 = exact_inputs(33, 1285, 64, seed=3, lo=-1, hi=2)  # features in {-1, 0, 1}: scores in a narrow range, ties everywhere
    for k in (16, 256):
        values, indices = search.topk_embeds(q.cuda(), keys.cuda(), k)
        check_exact(s64, values, indices, k, f"6 splits, k = {k}")
    assert min(len(np.unique(row)) for row in s64) < 64  # (1285 keys on fewer than 64 distinct scores)
    # ldq, ldk > D
    q, keys, s64 = exact_inputs(33, 65, 128, seed=98)
    qb, kb = torch.full((33, 136), 7.0), torch.full((65, 132), -3.0)
    qb[:, :128], kb[:, :128] = q, keys
    qd, kd = qb.cuda()[:, :128], kb.cuda()[:, :128]
    assert qd.stride(0) == 136 and kd.stride(0) == 132
    check_exact(s64, *search.topk_embeds(qd, kd, 9), 9, "ld > D")
    # k = nk, and k > nk: the tail is index -1, value -inf
    q, keys, s64 = exact_inputs(33, 63, 64, seed=96)
    check_exact(s64, *search.topk_embeds(q.cuda(), keys.cuda(), 63), 63, "k = nk")
    values, indices = search.topk_embeds(q.cuda(), keys.cuda(), 100)
    check_exact(s64, values, indices, 100, "k > nk")
    assert (indices[:, 63:] == -1).all() and (values[:, 63:] == -np.inf).all() and (indices[:, :63] >= 0).all()
    q1, k1, s1 = exact_inputs(1, 1, 64, seed=2)
    check_exact(s1, *search.topk_embeds(q1.cuda(), k1.cuda(), 256), 256, "one key, k = 256")


def test_topk_embeds_equal_scores_and_duplicated_keys(search):
    # all scores equal: the order is the index alone, descending
    q, keys = torch.ones(33, 64), torch.ones(1285, 64)
    values, indices = search.topk_embeds(q.cuda(), keys.cuda(), 40)
    assert np.array_equal(indices.cpu().numpy(), np.tile(np.arange(1284, 1244, -1), (33, 1)))
    assert (values == 64.0).all()
    # duplicated key rows: every score appears at least 37 times
    q, base, _ = exact_inputs(33, 7, 128, seed=5)
    keys = base[torch.arange(260) % 7].contiguous()
    s64 = (q.double() @ keys.double().t()).numpy()
    for k in (37, 38, 256):
        check_exact(s64, *search.topk_embeds(q.cuda(), keys.cuda(), k), k, f"duplicates, k = {k}")


def _targets(s64, k, per_row=16, seed=11):
    """per row 16 distinct keys: 8 of the float64 top 24 (ranks below and around k) and 8 others"""
    rng = np.random.default_rng(seed)
    rows = []
    for row in s64:
        order = np.argsort(row, kind="stable")[::-1]
        rows.append(np.concatenate([rng.choice(order[:24], 8, replace=False), rng.choice(order[24:], per_row - 8, replace=False)]))
    return np.stack(rows)


@pytest.mark.parametrize("kind", ["exact", "unit-norm"])
def test_topk_embeds_agrees_with_the_ranking_kernel_bit_for_bit(search, kind):
    from madtp_amd import retrieval_eval
    nq, nk, D, k = 33, 1285, 64, 16
    q, keys, s64 = exact_inputs(nq, nk, D, seed=21) if kind == "exact" else real_inputs(nq, nk, D)
    tgt = _targets(s64, k)
    ptr = torch.arange(0, 16 * nq + 1, 16, dtype=torch.int32).cuda()
    idx = torch.from_numpy(tgt.reshape(-1).astype(np.int32)).cuda()
    qd, kd = q.cuda(), keys.cuda()
    _, rank_tgt, score_tgt = retrieval_eval.rank_embeds(qd, kd, ptr, idx)
    values, indices = search.topk_embeds(qd, kd, k)
    rank_tgt, score_bits = rank_tgt.cpu().numpy().reshape(nq, 16), score_tgt.view(torch.int32).cpu().numpy().reshape(nq, 16)
    indices, value_bits = indices.cpu().numpy(), values.view(torch.int32).cpu().numpy()
    inside = 0
    for r in range(nq):
        for j in range(16):
            rho, t = int(rank_tgt[r, j]), int(tgt[r, j])
            if rho < k:
                assert indices[r, rho] == t and value_bits[r, rho] == score_bits[r, j], (r, j, rho)
                inside += 1
            else:
                assert t not in indices[r], (r, j, rho)
    print(f"{kind}: {inside} of {nq * 16} targets rank inside the top {k}")
    assert nq * 4 <= inside < nq * 16  # both branches are exercised


REAL = [(33, 1285, 64, 16), (40, 2000, 768, 64), (33, 5000, 256, 256), (65, 5000, 512, 128)]


@pytest.mark.parametrize("shape", REAL, ids=lambda s: "x".join(map(str, s)))
def test_topk_embeds_against_float64_on_unit_norm_inputs(search, shape):
    nq, nk, D, k = shape
    q, keys, s64 = real_inputs(nq, nk, D)
    values, indices = search.topk_embeds(q.cuda(), keys.cuda(), k)
    values, indices = values.cpu().numpy(), indices.cpu().numpy()
    order = np.argsort(s64, axis=1, kind="stable")[:, ::-1][:, :k + 1]
    v = np.take_along_axis(s64, order, 1)
    gap = v[:, :-1] - v[:, 1:]  # gap[p]: between positions p and p + 1 (k of them, the last to the first key left out)
    above = np.concatenate([np.full((nq, 1), np.inf), gap[:, :-1]], 1)
    pinned = (above >= GAP) & (gap >= GAP)
    boundary = gap[:, k - 1] >= GAP
    print(f"{shape}: {100 * pinned.mean():.1f} % of positions and {100 * boundary.mean():.1f} % of set boundaries pinned")
    assert pinned.mean() >= 0.95 and boundary.mean() >= 0.90
    assert np.array_equal(indices[pinned], order[:, :k][pinned])
    for r in np.flatnonzero(boundary):
        assert set(indices[r]) == set(order[r, :k]), r
    assert (indices >= 0).all() and all(len(set(row)) == k for row in indices)
    err = np.abs(values.astype(np.float64) - np.take_along_axis(s64, indices, 1)).max()
    print(f"{shape}: max |value - float64| = {err:.3g}")
    assert err < 1e-6
    assert (np.diff(values, axis=1) <= 0).all()  # best first in the kernel's own scores


def test_topk_embeds_nan_and_infinite_scores(search):
    rng = np.random.default_rng(4)
    q = torch.from_numpy(rng.choice([-2.0, -1.0, 1.0, 2.0], (5, 64)).astype(np.float32))  # no zero: inf * q is never NaN
    keys = torch.from_numpy(rng.integers(-2, 3, (300, 64)).astype(np.float32))
    for j in (3, 77, 130, 299):
        keys[j] = float("nan")
    for j, x in ((5, np.inf), (64, -np.inf), (200, np.inf), (201, -np.inf)):
        keys[j] = 0.0
        keys[j, 0] = x
    s64 = np.zeros((5, 300))
    with np.errstate(invalid="ignore"):
        for r in range(5):
            s64[r] = (q[r].double().numpy()[None, :] * keys.double().numpy()).sum(1)
    assert np.isnan(s64).sum() == 5 * 4 and np.isinf(s64).sum() == 5 * 4
    for k in (2, 256):  # (+inf first; 300 keys: the NaN and -inf ones stay outside the top 256)
        values, indices = search.topk_embeds(q.cuda(), keys.cuda(), k)
        check_exact(s64, values, indices, k, f"k = {k}")
    # all four NaN keys close a row of 64 keys, index descending, below -inf
    values, indices = search.topk_embeds(q.cuda(), keys[:80].cuda(), 80)
    check_exact(s64[:, :80], values, indices, 80, "NaN tail")
    assert indices[:, -2:].tolist() == [[77, 3]] * 5 and torch.isnan(values[:, -2:]).all() and (values[:, -3] == -np.inf).all()


def test_identical_calls_give_identical_bits(search):
    assert splits_of(search, 5, 20000) == 79  # many splits
    for (nq, nk, D), k in (((5, 20000, 64), 256), ((33, 5000, 256), 100)):
        q, keys, _ = real_inputs(nq, nk, D)
        qd, kd = q.cuda(), keys.cuda()
        first = search.topk_embeds(qd, kd, k)
        for _ in range(3):
            again = search.topk_embeds(qd, kd, k)
            assert torch.equal(again[1], first[1]) and torch.equal(again[0].view(torch.int32), first[0].view(torch.int32))
    q, keys, s64 = exact_inputs(5, 20000, 64, seed=8)
    check_exact(s64, *search.topk_embeds(q.cuda(), keys.cuda(), 256), 256, "79 splits")


def _scores_check(search, m, k, what):
    """m: a CPU f32 matrix (or view); the device result equals the restatement, values with the matrix's bits"""
    values, indices = search.topk_scores(m.cuda(), k)
    check_exact(m.double().numpy(), values, indices, k, what)


def test_topk_scores_blip_like_dense_ties_and_views(search):
    rng = np.random.default_rng(12)
    # BLIP's re-ranked matrices: -100 everywhere but 8 entries per row
    m = torch.full((37, 185), -100.0)
    for r in range(37):
        cols = rng.choice(185, 8, replace=False)
        m[r, cols] = torch.from_numpy(rng.standard_normal(8).astype(np.float32))
    for k in (8, 16):
        _scores_check(search, m, k, f"BLIP-like, k = {k}")
    values, indices = search.topk_scores(m.cuda(), 16)
    assert (values[:, 8:] == -100.0).all() and (values[:, :8] > -100.0).all()
    # the -100 entries tie: the largest free indices, descending
    free = [[c for c in range(184, -1, -1) if m[r, c] == -100.0][:8] for r in range(37)]
    assert indices[:, 8:].tolist() == free
    # dense matrices with ties (a few distinct values, -0 and +0 among them), sizes around the 256- and 1024-entry chunks
    for (nq, nk), k in (((3, 1), 1), ((4, 255), 255), ((4, 257), 256), ((5, 1023), 100), ((5, 1025), 256), ((3, 3000), 256),
                        ((2, 9), 20)):
        m = torch.from_numpy(rng.choice(np.array([-3.5, -0.0, 0.0, 1.0, 2.0, 7.25], dtype=np.float32), (nq, nk)))
        _scores_check(search, m, k, f"ties {nq} x {nk}, k = {k}")
    m = torch.from_numpy(rng.standard_normal((6, 2500)).astype(np.float32))
    m[1, 17], m[1, 2400], m[2, 0], m[3, 5], m[3, 6] = float("nan"), float("nan"), float("inf"), float("-inf"), float("nan")
    for k in (1, 50, 256):
        _scores_check(search, m, k, f"random with NaN and inf, k = {k}")
    # the values are the matrix's own bits (-0 stays -0)
    z = torch.tensor([[-0.0, 0.0, -0.0, -1.0]])
    values, indices = search.topk_scores(z.cuda(), 3)
    assert indices.tolist() == [[2, 1, 0]] and values.view(torch.int32).tolist() == [[-2 ** 31, 0, -2 ** 31]]
    # a leading dimension above nk, and a transposed view (ranked from a row-major copy)
    big = torch.from_numpy(rng.integers(-5, 6, (40, 300)).astype(np.float32)).cuda()
    view = big[:, :185]
    assert view.stride(0) == 300
    check_exact(view.cpu().double().numpy(), *search.topk_scores(view, 30), 30, "ld > nk")
    tv = big.t()
    assert tv.stride(1) == 300
    check_exact(tv.cpu().double().numpy(), *search.topk_scores(tv, 12), 12, "transposed view")


def test_embedding_index_and_clip_eval_search(search):
    from madtp_amd import retrieval_eval
    q, keys, s64 = real_inputs(33, 1285, 64)
    qd, kd = q.cuda(), keys.cuda()
    want = search.topk_embeds(qd, kd, 16)
    index = search.EmbeddingIndex(kd[:40])
    assert len(index) == 40
    index.add(kd[40:70]).add(kd[70:])
    assert len(index) == 1285 and torch.equal(index.keys, kd)
    for _ in range(2):  # the second call reuses the workspace
        got = index.search(qd, 16)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    part = search.EmbeddingIndex(kd[:40]).search(qd, 16)
    check = search.topk_embeds(qd, kd[:40], 16)
    assert torch.equal(part[1], check[1]) and torch.equal(part[0], check[0])
    ev = retrieval_eval.ClipEval(qd, kd, 0.0, [], [])
    for direction, (a, b) in (("i2t", (qd, kd)), ("t2i", (kd, qd))):
        got, want = ev.search(10, direction), search.topk_embeds(a, b, 10)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    with pytest.raises(ValueError, match="direction"):
        ev.search(10, "t2t")
    with pytest.raises(RuntimeError):
        search.topk_embeds(q, kd, 4)  # a CPU tensor
