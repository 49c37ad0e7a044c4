"""Retrieval evaluation on a real MI355X (csrc/eval.hip, madtp_amd/retrieval_eval.py): madtp_rank_embeds / madtp_rank_scores
against the float64 restatement of the rank rule in tests/rank_ref.py, and clip_evaluate() on the mirror model against its own
towers and the same restatement.

Tolerances.  Exact inputs (rank_ref.exact_features): every dot product is a multiple of 1/64 below 2^8, exact in f32 in any
order - ranks and scores must EQUAL the float64 ones.  Realistic inputs: scores within 1e-5 relative (test_itc_wide_gpu.py);
a target whose float64 score is >= GAP = 2e-6 from every other score of its row must rank exactly - GAP is 10x the largest
f32-vs-float64 score error of a CPU f32 matmul on these inputs (re-measured and asserted < 2e-7 in the test); the others may
differ by at most the number of competitors inside the gap, and are at most 3 % of a case's targets."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GAP = 2e-6

# (n_img, captions per image, D)
EXACT = [(1, 5, 512),     # one row, under one tile
         (3, 5, 64),      # the smallest D
         (16, 5, 512),    # a full 16-row MFMA block
         (17, 5, 512),    # one row past it
         (33, 5, 768),    # one row past a 32-row tile; 165 keys = two full column tiles + 37
         (13, 5, 576),    # 65 keys: one past a column tile
         (65, 4, 256),
         (40, 3, 1024),
         (257, 5, 768),   # the largest exact case
         (6, 16, 512),    # 16 targets per row
         (7, 1, 512)]     # one target per row
REAL = [(17, 5, 512), (33, 5, 768), (65, 4, 256), (40, 3, 1024), (130, 5, 576), (257, 5, 768)]


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


def _dev(*arrays):
    return [torch.as_tensor(a).cuda() for a in arrays]


def _directions(n_img, cap):
    """[(name, target lists, transpose?)] for image -> text and text -> image"""
    txt2img, img2txt = rank_ref.pairing(n_img, cap)
    return [("i2t", img2txt, False), ("t2i", [[t] for t in txt2img], True)]


@functools.lru_cache(maxsize=None)
def _exact(n_img, cap, D):
    img, txt = rank_ref.exact_features(n_img, cap, D, seed=n_img + D)
    s64 = (img.double() @ txt.double().t()).numpy()
    assert np.array_equal((img @ txt.t()).numpy().astype(np.float64), s64)  # the recipe: f32 is exact here
    out = {}
    for name, lists, tr in _directions(n_img, cap):
        s = s64.T if tr else s64
        rr, rt = rank_ref.ranks(s, lists)
        out[name] = (lists, rr, rt, np.array([s[r, t] for r in range(len(lists)) for t in lists[r]]))
    return img, txt, out


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s)))
def test_rank_embeds_equals_float64_on_exact_inputs(hip, shape):
    img, txt, ref = _exact(*shape)
    ties = 0
    for name, (lists, rr, rt, st) in ref.items():
        q, k = (txt, img) if name == "t2i" else (img, txt)
        ptr, idx = rank_ref.csr(lists)
        rank_row, rank_tgt, score_tgt = hip.rank_embeds(*_dev(q, k, ptr, idx))
        assert np.array_equal(score_tgt.cpu().numpy().astype(np.float64), st), name
        assert np.array_equal(rank_tgt.cpu().numpy(), rt), name
        assert np.array_equal(rank_row.cpu().numpy(), rr), name
        s = (q.double() @ k.double().t()).numpy()
        ties += sum(int((s[r] == s[r, t]).sum()) > 1 for r in range(len(lists)) for t in lists[r])
    print(f"{shape}: {ties} targets tie with another key, ranks up to {max(int(v[2].max()) for v in ref.values())}")


def test_rank_embeds_leading_dimensions_empty_rows_and_bad_targets(hip):
    img, txt, ref = _exact(17, 5, 512)
    lists, rr, rt, st = ref["i2t"]
    # ldq, ldk > D
    qb, kb = torch.full((17, 520), 7.0), torch.full((85, 516), -3.0)
    qb[:, :512], kb[:, :512] = img, txt
    qd, kd = qb.cuda()[:, :512], kb.cuda()[:, :512]
    assert qd.stride(0) == 520 and kd.stride(0) == 516
    ptr, idx = rank_ref.csr(lists)
    rank_row, rank_tgt, score_tgt = hip.rank_embeds(qd, kd, *_dev(ptr, idx))
    assert np.array_equal(rank_tgt.cpu().numpy(), rt) and np.array_equal(rank_row.cpu().numpy(), rr)
    assert np.array_equal(score_tgt.cpu().numpy().astype(np.float64), st)
    # rows 0 and 9 without a target
    some = [[] if r in (0, 9) else l for r, l in enumerate(lists)]
    s64 = (img.double() @ txt.double().t()).numpy()
    rr2, rt2 = rank_ref.ranks(s64, some)
    rank_row, rank_tgt, _ = hip.rank_embeds(*_dev(img, txt, *rank_ref.csr(some)))
    assert rr2[0] == 85 and rr2[9] == 85
    assert np.array_equal(rank_row.cpu().numpy(), rr2) and np.array_equal(rank_tgt.cpu().numpy(), rt2)
    # targets outside [0, nk) in the raw call: skipped (rank nk, NaN score, not in the row minimum), the rest unchanged
    bad = idx.copy()
    bad[2], bad[5 * 4 + 1], bad[5 * 16] = 85, -1, 2 ** 30   # row 0 (its third target), row 4, row 16
    rank_row, rank_tgt, score_tgt = hip.rank_embeds(*_dev(img, txt, ptr, bad))
    torch.cuda.synchronize()
    got, sc = rank_tgt.cpu().numpy(), score_tgt.cpu().numpy()
    skipped = np.isin(np.arange(len(idx)), [2, 21, 80])
    assert (got[skipped] == 85).all() and np.isnan(sc[skipped]).all()
    assert np.array_equal(got[~skipped], rt[~skipped]) and np.array_equal(sc[~skipped].astype(np.float64), st[~skipped])
    want_row = np.array([min([85] + [int(rt[5 * r + k]) for k in range(5) if not skipped[5 * r + k]]) for r in range(17)])
    assert np.array_equal(rank_row.cpu().numpy(), want_row)


def test_duplicate_keys_rank_by_index_with_identical_scores(hip):
    """Key rows 3, 70 and 140 are byte copies of key 100, a target of image 20 - three other column tiles, each a split of its
    own at this size.  The four scores must be the same bits and rank G+3, G+2, G+1, G (larger index first)."""
    img, txt = rank_ref.realistic_features(33, 5, 768)
    txt = txt.clone()
    for j in (3, 70, 140):
        txt[j] = txt[100]
    lists = [list(range(5 * i, 5 * i + 5)) for i in range(33)]
    lists[20] = [3, 70, 100, 140, 101]
    ptr, idx = rank_ref.csr(lists)
    rank_row, rank_tgt, score_tgt = hip.rank_embeds(*_dev(img, txt, ptr, idx))
    lo = int(ptr[20])
    sc = score_tgt.cpu().numpy()[lo:lo + 4]
    rk = rank_tgt.cpu().numpy()[lo:lo + 4]
    assert len(set(sc.view(np.int32).tolist())) == 1, sc
    assert rk.tolist() == [rk[3] + 3, rk[3] + 2, rk[3] + 1, rk[3]], rk
    s64 = (img[20].double() @ txt.double().t()).numpy()
    others = np.delete(s64, [3, 70, 100, 140])
    near = int((np.abs(others - s64[100]) < GAP).sum())
    assert abs(int(rk[3]) - int((others > s64[100]).sum())) <= near
    # as queries: the four identical caption rows score the same bits against their image
    t_ptr, t_idx = rank_ref.csr([[20] if j in (3, 70, 100, 140) else [j // 5] for j in range(165)])
    _, _, st = hip.rank_embeds(*_dev(txt, img, t_ptr, t_idx))
    st = st.cpu().numpy()
    assert len({int(st[j:j + 1].view(np.int32)[0]) for j in (3, 70, 100, 140)}) == 1


@functools.lru_cache(maxsize=None)
def _real(n_img, cap, D):
    img, txt = rank_ref.realistic_features(n_img, cap, D, seed=7)
    s64 = (img.double() @ txt.double().t()).numpy()
    err = float(np.abs((img @ txt.t()).numpy().astype(np.float64) - s64).max())
    out = {}
    for name, lists, tr in _directions(n_img, cap):
        s = s64.T if tr else s64
        rows = np.repeat(np.arange(len(lists)), [len(l) for l in lists])
        cols = np.array([t for l in lists for t in l])
        st = s[rows, cols]
        near, rank = np.empty(len(cols), dtype=np.int64), np.empty(len(cols), dtype=np.int64)
        col_id = np.arange(s.shape[1])[None, :]
        for a in range(0, len(cols), 512):
            r, c, v = rows[a:a + 512], cols[a:a + 512, None], st[a:a + 512, None]
            near[a:a + 512] = ((np.abs(s[r] - v) < GAP) & (col_id != c)).sum(1)   # competitors inside the gap
            rank[a:a + 512] = ((s[r] > v) | ((s[r] == v) & (col_id > c))).sum(1)
        out[name] = (lists, rank, st, near)
    return img, txt, err, out


def _check_realistic(hip, n_img, cap, D):
    img, txt, err, ref = _real(n_img, cap, D)
    assert err < 2e-7, err  # the error scale the 2e-6 gap is ten times of
    undecided = total = 0
    for name, (lists, rank, st, near) in ref.items():
        q, k = (txt, img) if name == "t2i" else (img, txt)
        rank_row, rank_tgt, score_tgt = hip.rank_embeds(*_dev(q, k, *rank_ref.csr(lists)))
        got, sc = rank_tgt.cpu().numpy().astype(np.int64), score_tgt.cpu().numpy().astype(np.float64)
        rel = np.abs(sc - st).max() / np.abs(st).max()
        assert rel < 1e-5, (name, rel)
        decided = near == 0
        assert np.array_equal(got[decided], rank[decided]), name
        assert (np.abs(got - rank)[~decided] <= near[~decided]).all(), name
        ptr, _ = rank_ref.csr(lists)
        assert np.array_equal(rank_row.cpu().numpy(), np.minimum.reduceat(got, ptr[:-1])), name
        undecided += int((~decided).sum())
        total += len(rank)
    r1 = float((ref["i2t"][1].reshape(n_img, cap).min(1) < 1).mean())
    print(f"({n_img}, {cap}, {D}): cpu f32 score error {err:.2e}, undecided {undecided} / {total}, R@1 {r1:.2f}, "
          f"ranks up to {int(ref['i2t'][1].max())}")
    assert undecided <= 0.03 * total, (undecided, total)


@pytest.mark.parametrize("shape", REAL, ids=lambda s: "x".join(map(str, s)))
def test_rank_embeds_realistic_inputs_against_float64(hip, shape):
    _check_realistic(hip, *shape)


def test_rank_embeds_large_case(hip):
    """The Flickr test set is 1000 images x 5000 captions at D 512.  With this recipe its undecided share - a property of the
    float64 scores alone - is 541 / 10000 = 5.4 % (and the CPU f32 error 2.2e-7), over the 3 % cap; 800 images give 4.6 %, 600
    3.4 %, 500 2.96 %, 400 2.3 %.  The image count is lowered to 400 (2000 captions, 63 key tiles, 13 row tiles), not the cap."""
    _check_realistic(hip, 400, 5, 512)


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "x".join(map(str, s)))
def test_rank_scores_equals_float64_on_dense_matrices(hip, shape):
    img, txt, ref = _exact(*shape)
    s = (img @ txt.t())
    for name, (lists, rr, rt, _) in ref.items():
        m = s.t().contiguous() if name == "t2i" else s
        ptr, idx = rank_ref.csr(lists)
        rank_row, rank_tgt = hip.rank_scores(*_dev(m, ptr, idx))
        assert np.array_equal(rank_tgt.cpu().numpy(), rt) and np.array_equal(rank_row.cpu().numpy(), rr), name
        # ld > nk with rows that start off a 16-byte boundary
        wide = torch.full((m.shape[0], m.shape[1] + 3), 1e9)
        wide[:, :m.shape[1]] = m
        view = wide.cuda()[:, :m.shape[1]]
        assert view.stride(0) == m.shape[1] + 3
        rank_row, rank_tgt = hip.rank_scores(view, *_dev(ptr, idx))
        assert np.array_equal(rank_tgt.cpu().numpy(), rt) and np.array_equal(rank_row.cpu().numpy(), rr), name


def _blip_like(nq, nk, k_test, g):
    m = torch.full((nq, nk), -100.0)
    for r in range(nq):
        cols = torch.randperm(nk, generator=g)[:k_test]
        m[r, cols] = torch.randn(k_test, generator=g) + 3
    return m


def test_rank_scores_blip_like_matrices_and_itm_eval(hip):
    """-100 everywhere except k_test = 8 re-ranked entries per row: ties with the fill are the common case"""
    from madtp_amd import retrieval_eval as re
    n_img, cap, k_test = 37, 5, 8
    n_txt = n_img * cap
    g = torch.Generator().manual_seed(3)
    txt2img, img2txt = rank_ref.pairing(n_img, cap)
    i2t, t2i = _blip_like(n_img, n_txt, k_test, g), _blip_like(n_txt, n_img, k_test, g)
    for i in range(0, n_img, 2):   # every other image: two of its captions among the re-ranked
        i2t[i, img2txt[i][0]] = 4.5
        i2t[i, img2txt[i][3]] = 2.5
    for j in range(0, n_txt, 3):
        t2i[j, txt2img[j]] = 4.0
    lists = img2txt
    ptr, idx = rank_ref.csr(lists)
    rank_row, rank_tgt = hip.rank_scores(*_dev(i2t, ptr, idx))
    rr, rt = rank_ref.ranks(i2t.double().numpy(), lists)
    got = rank_tgt.cpu().numpy()
    assert np.array_equal(got, rt) and np.array_equal(rank_row.cpu().numpy(), rr)
    filled = (i2t.numpy()[np.repeat(np.arange(n_img), cap), idx] != -100.0)
    assert filled.any() and (~filled).any() and (got[~filled] >= k_test).all()
    want = rank_ref.itm_eval(i2t.double().numpy(), t2i.double().numpy(), txt2img, img2txt)
    assert re.itm_eval(i2t.cuda(), t2i.cuda(), txt2img, img2txt) == want
    assert re.itm_eval(i2t.numpy(), t2i.numpy(), dict(enumerate(txt2img)), dict(enumerate(img2txt))) == want
    assert 0 < want["txt_r1"] < 100 and 0 < want["img_r10"] < 100


def test_identical_calls_are_bit_identical_across_a_large_call(hip):
    rimg, rtxt = rank_ref.realistic_features(33, 5, 768)
    _, img2txt = rank_ref.pairing(33, 5)
    ptr, idx = _dev(*rank_ref.csr(img2txt))
    small = _dev(rimg, rtxt)
    a = [t.clone() for t in hip.rank_embeds(*small, ptr, idx)]
    b = [t.clone() for t in hip.rank_embeds(*small, ptr, idx)]
    big_q, big_k = _dev(*rank_ref.realistic_features(1000, 5, 512))
    _, big_lists = rank_ref.pairing(1000, 5)
    big = hip.rank_embeds(big_q, big_k, *_dev(*rank_ref.csr(big_lists)))
    del big
    c = hip.rank_embeds(*small, ptr, idx)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))


# ---- clip_evaluate(): compress_retrieval_clip_dtp.py:78-124 on the mirror model --------------------------------------------------
@pytest.mark.parametrize("mode,tokenised", [("fp32", True), ("f16x3", False)])
def test_clip_evaluate_embeds_ranks_and_gflops(hip, mode, tokenised):
    """6 images in batches of 4 + 2, 3 captions each in text batches of 8 + 8 + 2, T = 4 on the ViT-B/16 mirror at 96^2: the
    embeddings are the normalised tower outputs of the same batches (same kernels, same batch shapes: equal bits), the lengths
    those of the blocks, the GFLOPs the analytic count at these lengths, the ranks those of the float64 scores of the embeddings
    under the rule of the realistic cases above, and score_matrices() their product (f32 chain over 512 features of unit
    vectors: at most 512 * 2^-24 off)."""
    from madtp_amd import clip_model as cm, harness, retrieval_eval as re, runtime, specs, synth, workloads
    n_img, img_bs, cap, size, T = 6, 4, 3, 96, 4.0
    n_txt = n_img * cap
    txt2img, img2txt = rank_ref.pairing(n_img, cap)
    model = cm.build_model(dict(specs.synth_weights(specs.clip_shapes(size), 0)), evaluate=True).eval().cuda()
    images = synth.synth_images(n_img, size, 0)
    text = synth.synth_clip_tokens(n_txt, 77, 0, 6, 40)
    if tokenised:
        texts = text                                  # pre-tokenised rows; model.tokenize stays None
    else:
        texts = [f"caption {j}" for j in range(n_txt)]
        model.tokenize = lambda caps: torch.stack([text[int(c.split()[1])] for c in caps])

    class Loader:
        dataset = types.SimpleNamespace(text=texts)
        def __iter__(self):
            for b in range(0, n_img, img_bs):
                yield images[b:b + img_bs], ["caption"] * len(images[b:b + img_bs]), torch.arange(b, min(n_img, b + img_bs))

    def lens(blocks, n0):
        return harness.token_lengths(workloads._traces(blocks), n0)

    with runtime.precision(mode), torch.no_grad():
        ev = re.clip_evaluate(model, Loader(), torch.device("cuda"), {"alpha": 0.4}, temperature=T, text_bs=8)
        metrics = ev.metrics(txt2img, img2txt)
        (_, rt_i, _), (_, rt_t, _) = ev.ranks(dict(enumerate(txt2img)), dict(enumerate(img2txt)))
        sims, sims_t, gflops = ev.score_matrices()
        want_i, want_t, vl, tl = [], [], [], []
        for b in range(0, n_img, img_bs):
            f, _ = model.encode_image(images[b:b + img_bs].cuda(), model.space_dict, T)
            want_i.append(f / f.norm(dim=1, keepdim=True))
            vl.append(lens(model.visual.transformer.resblocks, 37))
        for b in range(0, n_txt, 8):
            f, _ = model.encode_text(text[b:b + 8].cuda(), model.space_dict, T)
            want_t.append(f / f.norm(dim=1, keepdim=True))
            tl.append(lens(model.transformer.resblocks, 77))
    assert torch.equal(ev.image_embeds, torch.cat(want_i)) and torch.equal(ev.text_embeds, torch.cat(want_t))
    assert ev.image_embeds.shape == (n_img, 512) and ev.text_embeds.shape == (n_txt, 512)
    assert ev.vit_lens == vl and ev.txt_lens == tl and len(vl) == 2 and len(tl) == 3 and all(len(l) == 12 for l in vl + tl)
    assert vl[0][-1] < 37 and tl[0][-1] < 77                   # T = 4 prunes both towers
    count = (sum(b * workloads.clip_tower_flops(l, 37, 768, patch_in=768) for b, l in zip((4, 2), vl)) / 6
             + sum(b * workloads.clip_tower_flops(l, 77, 512) for b, l in zip((8, 8, 2), tl)) / 18) / 2e9
    unpruned = (workloads.clip_tower_flops([37] * 12, 37, 768, patch_in=768) + workloads.clip_tower_flops([77] * 12, 77, 512)) / 2e9
    assert abs(gflops - count) <= 1e-12 * count and 0 < gflops < unpruned
    s64 = (ev.image_embeds.double() @ ev.text_embeds.double().t()).cpu().numpy()
    assert np.abs(sims - s64).max() <= 512 * 2.0 ** -24 and np.array_equal(sims_t, sims.T) and sims.shape == (n_img, n_txt)
    got_rows = []
    for s, lists, got in ((s64, img2txt, rt_i), (s64.T, [[t] for t in txt2img], rt_t)):
        got = got.cpu().numpy().astype(np.int64)
        k = 0
        for r, l in enumerate(lists):
            for t in l:
                others = np.delete(s[r], t)
                near = int((np.abs(others - s[r, t]) < GAP).sum())
                assert abs(int(got[k]) - int((others > s[r, t]).sum())) <= near, (r, t)
                k += 1
        got_rows.append(np.minimum.reduceat(got, rank_ref.csr(lists)[0][:-1]))
    assert metrics == rank_ref.recall_dict(*got_rows)
    print(f"{mode}: {gflops:.2f} of {unpruned:.2f} GFLOPs per pair, metrics {metrics}")


# ---- the recording of the reference's own evaluate() + itm_eval() (tools/make_golden.py clip_eval_case) ---------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "clipeval_b6_T4.npz")
CLIP_TOL = 1e-3  # feature tolerance of test_model_parity_gpu.py::test_clip_both_towers


def _recorded_metrics(g):
    return dict(zip(g["metric_names"].tolist(), g["metrics"].tolist()))


def test_rank_embeds_reproduces_the_recorded_ranks_and_metrics(hip):
    """On the RECORDED embeddings: the smallest gap of the recording (1.98e-4, asserted >= 1e-4 by the recorder) is a thousand
    times the f32 rounding of these dot products, so ranks and metrics must equal the reference's exactly."""
    from madtp_amd import retrieval_eval as re
    g = np.load(FIXTURE)
    assert float(g["gap"]) >= 1e-4
    txt2img, img2txt = rank_ref.pairing(int(g["n_img"]), int(g["cap"]))
    assert txt2img == g["txt2img"].tolist()
    ev = re.ClipEval(*_dev(g["image_embeds"], g["text_embeds"]), 0.0, [], [])
    i2t, t2i = ev.ranks(txt2img, img2txt)
    assert np.array_equal(i2t[1].cpu().numpy(), g["rank_tgt_i2t"]) and np.array_equal(i2t[0].cpu().numpy(), g["rank_row_i2t"])
    assert np.array_equal(t2i[1].cpu().numpy(), g["rank_tgt_t2i"]) and np.array_equal(t2i[0].cpu().numpy(), g["rank_tgt_t2i"])
    assert ev.metrics(txt2img, img2txt) == _recorded_metrics(g)
    sims, sims_t, _ = ev.score_matrices()
    assert np.abs(sims - g["sims"]).max() <= 512 * 2.0 ** -24 and np.array_equal(sims_t, sims.T)


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
def test_clip_evaluate_matches_the_reference_recording(hip, mode):
    """clip_evaluate() on the mirror model (the recording's weights and inputs) against the reference driver's evaluate():
    embeddings and sims within the CLIP parity tolerance, the per-layer lengths of every batch equal.  Ranks: the issue wanted a
    recording whose ground-truth scores are 0.1 from all others, so that the live metrics must equal the recorded dict; no seed
    gives that (all scores of this set lie within ~0.12; tools/make_golden.py keeps the best of 16 seeds, gap 1.98e-4).  So, as in
    the realistic cases above: with e = the largest difference between the live and the recorded scores (asserted < 1e-3), a
    target whose recorded gap exceeds 2 e cannot change rank and must equal the recording; another may move by at most the
    number of competitors within 2 e; when every target is pinned, the metrics must equal the recorded dict."""
    from madtp_amd import clip_model as cm, retrieval_eval as re, runtime, specs, synth
    g = np.load(FIXTURE)
    n_img, img_bs, cap, size, seed = (int(g[k]) for k in ("n_img", "img_bs", "cap", "size", "seed"))
    T, n_txt = float(g["temperature"]), n_img * cap
    txt2img, img2txt = rank_ref.pairing(n_img, cap)
    model = cm.build_model(dict(specs.synth_weights(specs.clip_shapes(size), seed)), evaluate=True).eval().cuda()
    images = synth.synth_images(n_img, size, seed)
    text = synth.synth_clip_tokens(n_txt, 77, seed, 6, 40)
    model.tokenize = lambda t: t   # as the recorder's: dataset.text holds token rows

    class Loader:
        dataset = types.SimpleNamespace(text=text)
        def __iter__(self):
            for b in range(0, n_img, img_bs):
                yield images[b:b + img_bs], ["caption"] * len(images[b:b + img_bs]), torch.arange(b, min(n_img, b + img_bs))

    with runtime.precision(mode):
        ev = re.clip_evaluate(model, Loader(), torch.device("cuda"), {"alpha": 0.4}, temperature=T)
        metrics = ev.metrics(txt2img, img2txt)
        (rr_i, rt_i, _), (rr_t, rt_t, _) = ev.ranks(txt2img, img2txt)
        sims, sims_t, gflops = ev.score_matrices()
    e_img = float(np.abs(ev.image_embeds.cpu().numpy() - g["image_embeds"]).max())
    e_txt = float(np.abs(ev.text_embeds.cpu().numpy() - g["text_embeds"]).max())
    e = float(np.abs(sims - g["sims"]).max())
    print(f"{mode}: embeds off by {e_img:.2e} (image) {e_txt:.2e} (text), sims by {e:.2e}; {gflops:.2f} GFLOPs per pair")
    assert ev.vit_lens == g["vit_lens"].tolist() and ev.txt_lens == g["txt_lens"].tolist()
    assert e_img < CLIP_TOL and e_txt < CLIP_TOL and e < CLIP_TOL
    assert sims.shape == (n_img, n_txt) and np.array_equal(sims_t, sims.T)
    s64 = g["image_embeds"].astype(np.float64) @ g["text_embeds"].astype(np.float64).T
    pinned = 0
    for s, rows, cols, got, rec, gap in ((s64, txt2img, range(n_txt), rt_i, g["rank_tgt_i2t"], g["gap_i2t"]),
                                         (s64.T, range(n_txt), txt2img, rt_t, g["rank_tgt_t2i"], g["gap_t2i"])):
        got = got.cpu().numpy()
        for k, (r, c) in enumerate(zip(rows, cols)):   # image -> text targets are in caption order: CSR position k = caption k
            near = int((np.abs(np.delete(s[r], c) - s[r, c]) <= 2 * e).sum())
            assert (near == 0) == (gap[k] > 2 * e)
            assert abs(int(got[k]) - int(rec[k])) <= near, (mode, r, c, int(got[k]), int(rec[k]), near)
            pinned += near == 0
    print(f"{mode}: {pinned} of {2 * n_txt} targets pinned at 2 e = {2 * e:.2e}")
    assert metrics == rank_ref.recall_dict(rr_i.cpu().numpy(), rr_t.cpu().numpy())
    if pinned == 2 * n_txt:
        assert metrics == _recorded_metrics(g)


def test_no_targets_malformed_pointers_and_transposed_views(hip):
    from madtp_amd import retrieval_eval as re
    img, txt, ref = _exact(17, 5, 512)
    lists, rr, rt, _ = ref["i2t"]
    s = (img @ txt.t()).cuda()
    # no ground truth at all: every row ranks nk
    ptr0, idx0 = _dev(np.zeros(18, dtype=np.int32), np.zeros(0, dtype=np.int32))
    rank_row, rank_tgt, score_tgt = hip.rank_embeds(*_dev(img, txt), ptr0, idx0)
    assert rank_row.tolist() == [85] * 17 and rank_tgt.numel() == 0 and score_tgt.numel() == 0
    rank_row, rank_tgt = hip.rank_scores(s, ptr0, idx0)
    assert rank_row.tolist() == [85] * 17 and rank_tgt.numel() == 0
    # pointers that leave [0, tgt_ptr[nq]] or run backwards: those rows are empty, nothing outside the arrays is touched
    ptr, idx = rank_ref.csr(lists)
    bad = ptr.copy()
    bad[3], bad[9] = -7, 10 ** 6                     # rows 2, 3 and 8, 9
    empty = np.isin(np.arange(17), [2, 3, 8, 9])
    for rank_row, rank_tgt in (hip.rank_embeds(*_dev(img, txt, bad, idx))[:2], hip.rank_scores(s, *_dev(bad, idx))):
        row, tgt = rank_row.cpu().numpy(), rank_tgt.cpu().numpy()
        assert (row[empty] == 85).all() and np.array_equal(row[~empty], rr[~empty])
        assert np.array_equal(tgt[np.repeat(~empty, 5)], rt[np.repeat(~empty, 5)])
    # a driver hands itm_eval the matrix and its transposed view
    txt2img, img2txt = rank_ref.pairing(17, 5)
    assert not s.t().is_contiguous()
    assert re.itm_eval(s, s.t(), txt2img, img2txt) == re.itm_eval(s, s.t().contiguous(), txt2img, img2txt) \
        == rank_ref.itm_eval(s.double().cpu().numpy(), s.double().cpu().numpy().T, txt2img, img2txt)
