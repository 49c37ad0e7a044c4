"""The certified bf16 shortlist of the retrieval search on a real MI355X (include/madtp_csearch.h, csrc/search_coarse.hip):
search.topk_embeds(q, keys, k, coarse="bf16") against search.topk_embeds(q, keys, k).

"Equal" always means torch.equal on the indices and on the int32 bit patterns of the values.  The shares of certified rows
asserted below are no tolerances: they keep the fallback (which IS the exact route) from carrying a test."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def search():
    from madtp_amd import build, hip, search as s
    build.build(verbose=False)
    hip.load()
    assert torch.cuda.is_available()
    return s


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def gaussian(nq, nk, D, seed=11):
    rng = np.random.default_rng(seed)
    q, keys = unit(rng.standard_normal((nq, D))), unit(rng.standard_normal((nk, D)))
    return torch.from_numpy(q.astype(np.float32)), torch.from_numpy(keys.astype(np.float32))


@functools.lru_cache(maxsize=None)
def clip_like(nq, nk, D, seed=12, mean=0.8):
    """unit rows that share a mean direction: x = mean * mu + sqrt(1 - mean^2) * (unit noise), as the embeddings of one tower do"""
    rng = np.random.default_rng(seed)
    mu = unit(rng.standard_normal((1, D)))
    q = unit(mean * mu + np.sqrt(1 - mean * mean) * unit(rng.standard_normal((nq, D))))
    keys = unit(mean * mu + np.sqrt(1 - mean * mean) * unit(rng.standard_normal((nk, D))))
    return torch.from_numpy(q.astype(np.float32)), torch.from_numpy(keys.astype(np.float32))


@functools.lru_cache(maxsize=None)
def cluster(nk, D, seed=13, radius=1e-4):
    """(direction [D], nk unit keys within `radius` of it)"""
    rng = np.random.default_rng(seed)
    d = unit(rng.standard_normal((1, D)))
    keys = unit(d + radius * rng.uniform(0, 1, (nk, 1)) * unit(rng.standard_normal((nk, D))))
    return d[0], torch.from_numpy(keys.astype(np.float32))


def both(search, q, keys, k, m=None):
    """the exact and the coarse answer for GPU tensors, asserted equal -> the SearchInfo"""
    ev, ei = search.topk_embeds(q, keys, k)
    cv, ci, info = search.topk_embeds(q, keys, k, coarse="bf16", shortlist=m, return_info=True)
    assert ci.dtype == torch.int64 and cv.dtype == torch.float32 and ci.shape == ei.shape == cv.shape
    assert torch.equal(ci, ei)
    assert torch.equal(cv.view(torch.int32), ev.view(torch.int32))
    n_un = int((~info.certified).sum())
    assert info.n_fallback == n_un
    rows = info.fallback_rows
    assert torch.equal(rows, torch.nonzero(~info.certified).flatten())  # the list is ascending and complete
    assert torch.equal(info.fallback_position[rows], torch.arange(n_un, device=rows.device, dtype=torch.int32))
    return info


# ---- 1. equality on seeded inputs -------------------------------------------------------------------------------------------------
CASES = [(70, 3000, 256, 10, 64), (33, 700, 64, 1, 64), (45, 5000, 512, 100, 256), (45, 5000, 1024, 128, 256), (1, 130, 64, 10, 64)]


@pytest.mark.parametrize("family", ["gaussian", "clip_like"])
@pytest.mark.parametrize("nq,nk,D,k,m", CASES)
def test_equal_to_the_exact_route(search, family, nq, nk, D, k, m):
    """Equal on every case, and at least 90 % of the rows certified wherever the float64 restatement of the certificate
    (restate(), computed before the device runs) certifies that many: nine of the ten cases, all of them at 100 %.  The tenth,
    clip_like at D 1024 / k 128 / m 256, is an input whose gaps ARE the bound: with 36 % of a score in the row's own direction
    the scores of 5000 keys spread by sigma = 0.36 / 32 = 0.011, the 128th and the 256th best lie 0.32 sigma = 3.6e-3 apart, and
    E is 3.7e-3 to 3.9e-3 - the restatement certifies 27 of the 45 rows, and so does the device (0.600 measured).  There, as
    everywhere, the device's flags must be the restatement's wherever its margin exceeds 10 % of E."""
    q, keys = (gaussian if family == "gaussian" else clip_like)(nq, nk, D)
    margin, E = restate(search, q, keys, k, m) if nk > m else (np.ones(nq), np.ones(nq))
    info = both(search, q.cuda(), keys.cuda(), k, m)
    share, restated = float(info.certified.float().mean()), float((margin > 0).mean())
    print(f"{family} {(nq, nk, D, k, m)}: certified {share:.3f}, restated {restated:.3f}")
    assert restated >= 0.9 or (family, D, k) == ("clip_like", 1024, 128)
    if restated >= 0.9:
        assert share >= 0.9
    clear = np.abs(margin) > 0.1 * E
    assert np.array_equal(info.certified.cpu().numpy()[clear], margin[clear] > 0)
    assert info.shortlist_indices.shape == (nq, m) and info.shortlist_coarse.shape == (nq, m)


def test_equal_on_strided_rows(search):
    q, keys = gaussian(70, 3000, 256)
    qb = torch.zeros(70, 256 + 8, device="cuda")
    qb[:, :256] = q.cuda()
    kb = torch.zeros(6000, 256, device="cuda")
    kb[::2] = keys.cuda()
    qv, kv = qb[:, :256], kb[::2]
    assert qv.stride(0) == 264 and kv.stride(0) == 512
    info = both(search, qv, kv, 10, 64)
    assert float(info.certified.float().mean()) >= 0.9
    ref = search.topk_embeds(q.cuda(), keys.cuda(), 10, coarse="bf16")
    got = search.topk_embeds(qv, kv, 10, coarse="bf16")
    assert torch.equal(ref[1], got[1]) and torch.equal(ref[0].view(torch.int32), got[0].view(torch.int32))
    # the default shortlist is the smallest that holds 2 k
    for k, m in ((1, 64), (32, 64), (33, 128), (64, 128), (65, 256), (128, 256)):
        assert search.check_coarse("bf16", k, "test") == m


# ---- 2. adversarial gaps ----------------------------------------------------------------------------------------------------------
def restate(search, q, keys, k, m):
    """float64 restatement of the certificate on the host -> (margin s_k - c_m - E [nq], E [nq])"""
    s = (q.double() @ keys.double().t()).numpy()
    c = (q.bfloat16().double() @ keys.bfloat16().double().t()).numpy()
    E = search.coarse_bound(q, keys).numpy()
    margin = np.empty(len(s))
    for r in range(len(s)):
        short = np.argsort(c[r], kind="stable")[::-1][:m]
        margin[r] = np.sort(s[r, short])[::-1][k - 1] - c[r, short[-1]] - E[r]
    return margin, E


def test_a_cluster_of_near_duplicates_certifies_nothing(search):
    d, keys = cluster(700, 256)
    q = torch.from_numpy(unit(d[None] + 0.3 * unit(np.random.default_rng(5).standard_normal((40, 256)))).astype(np.float32))
    margin, _ = restate(search, q, keys, 10, 64)
    assert (margin < 0).all()
    info = both(search, q.cuda(), keys.cuda(), 10, 64)
    assert not bool(info.certified.any()) and info.n_fallback == 40


def test_a_mixed_batch_certifies_the_rows_the_restatement_certifies(search):
    D, k, m = 256, 10, 64
    d, near = cluster(700, D)
    _, rand = gaussian(100, 3000, D)
    keys = torch.cat([rand, near], 0)
    rng = np.random.default_rng(6)
    g = unit(rng.standard_normal((100, D)))
    g[1::2] = unit(d[None] + 0.3 * g[1::2])                       # odd rows: near the cluster's direction
    g[0::2] = unit(g[0::2] - (g[0::2] @ d)[:, None] * d[None])    # even rows: that direction projected out
    q = torch.from_numpy(g.astype(np.float32))
    margin, E = restate(search, q, keys, k, m)
    share = float((margin > 0).mean())
    print(f"restated certified share {share:.2f}")
    assert 0.3 <= share <= 0.7
    info = both(search, q.cuda(), keys.cuda(), k, m)
    cert = info.certified.cpu().numpy()
    clear = np.abs(margin) > 0.1 * E
    assert clear.sum() >= 60
    assert np.array_equal(cert[clear], margin[clear] > 0)
    rows = info.fallback_rows.cpu().numpy()
    assert (np.diff(rows) > 0).all() and len(rows) == (~cert).sum()


# ---- 3. ties ----------------------------------------------------------------------------------------------------------------------
def ints(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float32))


@pytest.mark.parametrize("case", ["all_equal", "duplicates", "k_is_nk", "k_above_nk", "nk_is_m", "nk_below_m", "nk_above_m"])
def test_ties_resolve_as_the_exact_route_resolves_them(search, case):
    """entries in {-2 .. 2}: exact in bf16 and in every partial sum, so the scores tie in both routes"""
    D = 64
    q = ints((37, D), 1)
    nk, k, m = {"all_equal": (500, 10, 64), "duplicates": (900, 20, 64), "k_is_nk": (30, 30, 64), "k_above_nk": (5, 10, 64),
                "nk_is_m": (64, 10, 64), "nk_below_m": (100, 40, 128), "nk_above_m": (65, 10, 64)}[case]
    keys = ints((nk, D), 2)
    if case == "all_equal":
        keys = keys[:1].repeat(nk, 1)
    if case == "duplicates":
        keys = keys[:90].repeat(10, 1)
    info = both(search, q.cuda(), keys.cuda(), k, m)
    if nk <= m:
        assert bool(info.certified.all())  # every key is shortlisted
        if nk < m:
            assert bool((info.shortlist_indices[:, nk:] == -1).all()) and bool(torch.isinf(info.threshold).all())
    if case == "all_equal":
        assert not bool(info.certified.any())  # ties across the shortlist's boundary


# ---- 4. NaN / inf -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["key", "query", "both"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_elements(search, where, value):
    q, keys = gaussian(33, 700, 64)
    q, keys = q.clone(), keys.clone()
    if where in ("key", "both"):
        keys[123, 5] = value
    if where in ("query", "both"):
        q[7, 9] = value
    info = both(search, q.cuda(), keys.cuda(), 10, 64)
    cert = info.certified.cpu()
    if where == "query":
        assert not bool(cert[7]) and float(cert.float().mean()) >= 0.9
    else:
        assert not bool(cert.any())  # a gallery with a non-finite row certifies nothing


# ---- 5. EmbeddingIndex ------------------------------------------------------------------------------------------------------------
def test_embedding_index_keeps_the_gallery_across_adds(search):
    q, keys = gaussian(50, 900, 128)
    q, keys = q.cuda(), keys.cuda()
    index = search.EmbeddingIndex(keys[:300], coarse="bf16")
    v0, i0 = index.search(q, 10)
    e0 = search.topk_embeds(q, keys[:300], 10)
    assert torch.equal(i0, e0[1]) and torch.equal(v0.view(torch.int32), e0[0].view(torch.int32))
    index.add(keys[300:500])   # 300 -> 600 rows of storage
    index.add(keys[500:900])   # 600 -> 1200
    assert len(index) == 900 and index._store.shape[0] == 1200 and index._store16.shape[0] == 1200
    v, i, info = index.search(q, 10, return_info=True)
    fresh = search.EmbeddingIndex(keys, coarse="bf16")
    fv, fi = fresh.search(q, 10)
    ev, ei = search.topk_embeds(q, keys, 10)
    for ov, oi in ((fv, fi), (ev, ei)):
        assert torch.equal(i, oi) and torch.equal(v.view(torch.int32), ov.view(torch.int32))
    assert float(info.certified.float().mean()) >= 0.9
    k16, stats = search.prepare(keys)
    assert torch.equal(index.coarse_summary.view(torch.int32), search.summary(stats).view(torch.int32))
    assert torch.equal(index._store16[:900].view(torch.int16), k16.view(torch.int16))
    assert torch.equal(k16.view(torch.int16).cpu(), keys.cpu().bfloat16().view(torch.int16))  # round to nearest even
    # the statistics are upper bounds of the float64 norms, and close ones
    k64, k16d = keys.double().cpu(), k16.double().cpu()
    want = torch.stack([k64.norm(dim=1), (k64 - k16d).norm(dim=1), k16d.norm(dim=1)], 1)
    got = stats[:, :3].double().cpu()
    assert bool((got >= want).all()) and bool((got <= want * (1 + 2.0 ** -9)).all()) and bool((stats[:, 3] == 0).all())


# ---- 6. the bound, on the device --------------------------------------------------------------------------------------------------
def families():
    q, keys = gaussian(40, 2000, 256, seed=21)
    yield "unit", q, keys, False
    rng = np.random.default_rng(22)
    def heavy(n):
        return torch.from_numpy((rng.choice([-1.0, 1.0], (n, 1024)) * rng.uniform(1, 2, (n, 1024))).astype(np.float32))
    yield "cancellation", heavy(24), heavy(1500), False
    yield "x 1e4", q * 1e4, keys * 1e4, False
    yield "x 1e-30", q * 1e-30, keys * 1e-30, True
    yield "q x 1e-30", q * 1e-30, keys, True


def test_the_bound_holds_for_every_shortlisted_pair(search):
    """For every row r and shortlisted key j: |float64 <q, y> - coarse| <= E_r as the device reports it, and
    |float64 <q16, y16> - coarse| <= the third term alone, A D 2^-24 |q16_r| max|y16|.  Where the scores leave the normal range of
    f32 (the rows scaled by 1e-30) the coarse score is rounded absolutely, not relatively, and the 2 D 2^-126 that the header's U
    holds for the coarse stage is added to the third term.  The largest ratio to the third term is printed; README.md records
    it."""
    worst3 = 0.0
    for name, q, keys, tiny in families():
        D = q.shape[1]
        _, _, info = search.topk_embeds(q.cuda(), keys.cuda(), 10, coarse="bf16", shortlist=64, return_info=True)
        idx, coarse = info.shortlist_indices.cpu(), info.shortlist_coarse.double().cpu()
        assert bool((idx >= 0).all())
        q64, k64 = q.double(), keys.double()
        q16, k16 = q.bfloat16().double(), keys.bfloat16().double()
        real = torch.einsum("rd,rmd->rm", q64, k64[idx])
        real16 = torch.einsum("rd,rmd->rm", q16, k16[idx])
        E = info.bound.double().cpu()
        ratio = float(((real - coarse).abs() / E[:, None]).max())
        third = search.COARSE_ACC_FACTOR * D * U24 * q16.norm(dim=1) * k16.norm(dim=1).max()
        err3 = (real16 - coarse).abs()
        allow3 = third + (2 * D * 2.0 ** -126 if tiny else 0.0)
        ratio3 = float((err3 / allow3[:, None]).max())
        print(f"{name}: max |<q,y> - coarse| / E = {ratio:.3g}; max |<q16,y16> - coarse| / third term = {ratio3:.3g}")
        assert ratio <= 1.0, name
        assert ratio3 <= 1.0, name
        # the device's bound is the restated one from statistics rounded up (and evaluated in f32: 2^-20 for its roundings)
        assert bool((E >= search.coarse_bound(q, keys) * (1 - 2.0 ** -20)).all()), name
        assert bool((E <= search.coarse_bound(q, keys) * (1 + 2.0 ** -8)).all()), name
        if not tiny:
            worst3 = max(worst3, ratio3)
    print(f"largest ratio to the third term (A = {search.COARSE_ACC_FACTOR}): {worst3:.3g}")
    assert worst3 <= 0.5  # the factor of two the header promises on top of what was measured


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------
def test_identical_calls_give_identical_bits(search):
    d, near = cluster(300, 256)
    _, rand = gaussian(70, 3000, 256)
    q, _ = clip_like(70, 10, 256)
    q, keys = q.cuda(), torch.cat([rand, near], 0).cuda()
    outs = [search.topk_embeds(q, keys, 10, coarse="bf16", return_info=True) for _ in range(3)]
    for v, i, info in outs[1:]:
        assert torch.equal(i, outs[0][1]) and torch.equal(v.view(torch.int32), outs[0][0].view(torch.int32))
        for name in ("certified", "fallback_position", "shortlist_indices"):
            assert torch.equal(getattr(info, name), getattr(outs[0][2], name)), name
        for name in ("threshold", "bound", "shortlist_coarse"):
            assert torch.equal(getattr(info, name).view(torch.int32), getattr(outs[0][2], name).view(torch.int32)), name
        assert info.n_fallback == outs[0][2].n_fallback


# ---- 8. BLIP evaluate -------------------------------------------------------------------------------------------------------------
def test_blip_evaluate_takes_the_coarse_route(search):
    from madtp_amd import blip_retrieval as br, harness, retrieval_eval
    g = np.load(os.path.join(ROOT, "tests", "golden", "retr_i6_t12.npz"))
    n_img, img_bs, n_txt, size = int(g["n_img"]), int(g["img_bs"]), int(g["n_txt"]), int(g["size"])
    T, k_test, seed = float(g["temperature"]), int(g["k_test"]), int(g["seed"])
    model = harness.build_retrieval(size, seed)
    batches, ids, att = harness.retrieval_inputs(n_img, img_bs, n_txt, size, 35, seed, device="cuda")
    loader = harness.RetrievalLoader(batches, ids, att)
    cfg = {"k_test": k_test}
    want = br.evaluate(model, loader, torch.device("cuda"), cfg, T, candidates="device")
    got = br.evaluate(model, loader, torch.device("cuda"), cfg, T, candidates="device", coarse="bf16")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="k = 129"):
        br.evaluate(model, loader, torch.device("cuda"), {"k_test": 129}, T, candidates="device", coarse="bf16")
    # ClipEval.search passes the keyword through
    q, keys = clip_like(40, 600, 64)
    ev = retrieval_eval.ClipEval.__new__(retrieval_eval.ClipEval)
    ev.image_embeds, ev.text_embeds = q.cuda(), keys.cuda()
    for direction in ("i2t", "t2i"):
        a, b = ev.search(10, direction), ev.search(10, direction, coarse="bf16")
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
