"""blip_retrieval.evaluate(scores="lists"), retrieval_eval.itm_eval on CandidateLists and blip_search.BlipSearcher on a real MI355X,
with the fixtures and the harness of tests/test_retrieval_candidates_gpu.py.  Everything here is an equality: the lists route
runs the re-ranking calls of the dense route, same batches, same order."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["retr_i6_t12", "retr_384_i4_t6"]
DEV = torch.device("cuda")


def _setup(case):
    from madtp_amd import build, hip, harness
    build.build(verbose=False)
    hip.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    n_img, img_bs, n_txt, size = int(g["n_img"]), int(g["img_bs"]), int(g["n_txt"]), int(g["size"])
    model = harness.build_retrieval(size, int(g["seed"]))
    batches, ids, att = harness.retrieval_inputs(n_img, img_bs, n_txt, size, 35, int(g["seed"]), device="cuda")
    return model, harness.RetrievalLoader(batches, ids, att), batches, ids, att, float(g["temperature"]), int(g["k_test"])


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return torch.equal(a.idx, b.idx) and torch.equal(a.val.view(torch.int32), b.val.view(torch.int32)) and (a.nk, a.fill) == (b.nk, b.fill)


def _argsort_rows(dense, r):
    """(ids, values) [n, r] of np.argsort(row, kind="stable")[::-1][:r] per dense row"""
    order = np.stack([np.argsort(row, kind="stable")[::-1][:r] for row in dense])
    return order, np.take_along_axis(dense, order, 1)


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_lists_route_and_searcher_equal_the_dense_route(case, mode):
    from madtp_amd import blip_retrieval as br, retrieval_eval, runtime
    from madtp_amd.blip_search import BlipSearcher, SearchResult
    from madtp_amd.lists import CandidateLists
    model, loader, batches, ids, att, T, k_test = _setup(case)
    cfg = {"k_test": k_test}
    n_img, n_txt = sum(b.shape[0] for b in batches), ids.shape[0]
    with runtime.precision(mode):
        d_i2t, d_t2i, _ = br.evaluate(model, loader, DEV, cfg, T, candidates="device")
        l_i2t, l_t2i, gflops = br.evaluate(model, loader, DEV, cfg, T, candidates="device", scores="lists")
        # ---- the lists are the matrices
        assert gflops == 0.0 and isinstance(l_i2t, CandidateLists) and l_i2t.idx.is_cuda and l_t2i.val.is_cuda
        assert l_i2t.shape == (n_img, k_test) and l_t2i.shape == (n_txt, k_test) and (l_i2t.nk, l_t2i.nk) == (n_txt, n_img)
        assert l_i2t.validate() is l_i2t and l_t2i.validate() is l_t2i and l_i2t.nbytes == n_img * k_test * 12
        assert np.array_equal(_np(l_i2t.to_dense()), d_i2t) and np.array_equal(_np(l_t2i.to_dense()), d_t2i)
        # ---- two rank slices, gathered by hand, are the whole; rows of the other rank are empty
        parts = [br.evaluate(model, loader, DEV, cfg, T, rank=r, world_size=2, candidates="device", scores="lists") for r in range(2)]
        for k, whole in ((0, l_i2t), (1, l_t2i)):
            n = whole.shape[0]
            (s0, e0), (s1, e1) = br.rank_rows(n, 0, 2), br.rank_rows(n, 1, 2)
            assert (s0, e0, e1) == (0, s1, n)
            assert (parts[0][k].idx[e0:] == -1).all() and (parts[1][k].idx[:s1] == -1).all()
            merged = CandidateLists(torch.cat([parts[0][k].idx[:e0], parts[1][k].idx[s1:]]),
                                    torch.cat([parts[0][k].val[:e0], parts[1][k].val[s1:]]), whole.nk)
            assert _same(merged, whole)
            assert np.array_equal(_np(parts[0][k].to_dense())[e0:], np.full((n - e0, whole.nk), -100.0, dtype=np.float32))
        # ---- itm_eval: the dict of the matrices, two captions per image
        img2txt = [[i, (i + n_img) % n_txt] for i in range(n_img)]
        txt2img = [t % n_img for t in range(n_txt)]
        want = retrieval_eval.itm_eval(d_i2t, d_t2i, txt2img, img2txt)
        assert retrieval_eval.itm_eval(l_i2t, l_t2i, txt2img, img2txt) == want and len(want) == 9
        # ---- the searcher, fed the loader's batches and texts
        s = BlipSearcher(model, temperature=T, k_test=k_test)
        for b in batches:
            s.add_images(b)
        s.add_texts(ids, att)
        assert (s.n_images, s.n_texts) == (n_img, n_txt)
        assert _same(s.lists("i2t"), l_i2t) and _same(s.lists("t2i"), l_t2i)
        some = [n_img - 1, 0]
        assert _same(s.lists("i2t", rows=some), CandidateLists(l_i2t.idx[some], l_i2t.val[some], n_txt))
        from madtp_amd import search
        for r in (1, k_test):
            for res, dense, q, keys in ((s.texts_for_images(None, r), d_i2t, s.image_embeds, s.text_embeds),
                                        (s.images_for_texts(None, r), d_t2i, s.text_embeds, s.image_embeds)):
                want_ids, want_val = _argsort_rows(dense, r)
                assert isinstance(res, SearchResult) and res.ids.dtype == torch.int64 and res.score.dtype == torch.float32
                assert np.array_equal(_np(res.ids), want_ids) and np.array_equal(_np(res.score), want_val)
                # the ITC term followed its key: it is the stage-1 score of that pair
                sim, idx = search.topk_embeds(q, keys, k_test)
                pos = (idx[:, None, :] == res.ids[:, :, None]).long().argmax(-1)
                assert torch.equal(res.itc, sim.gather(1, pos))
        whole = s.images_for_texts(None, k_test)
        again = s.query_texts(ids, att, k_test)  # the indexed texts' own ids as new queries
        assert all(torch.equal(a, b) for a, b in zip(again, whole))
        sub = s.images_for_texts(torch.tensor([2, 0]), 1)
        assert torch.equal(sub.ids, whole.ids[[2, 0], :1]) and torch.equal(sub.score, whole.score[[2, 0], :1])
        # ---- kv_cache=False changes no bit
        nc = BlipSearcher(model, temperature=T, k_test=k_test, kv_cache=False)
        for b in batches:
            nc.add_images(b)
        nc.add_texts(ids, att)
        assert _same(nc.lists("i2t"), l_i2t) and _same(nc.lists("t2i"), l_t2i)
        # ---- a query between two add_images calls sees the first batch alone; afterwards everything is re-padded
        lazy = BlipSearcher(model, temperature=T, k_test=k_test)
        lazy.add_texts(ids, att)
        lazy.add_images(batches[0])
        assert batches[0].shape[0] < k_test  # (both fixtures: the first batch alone is no gallery for k_test candidates)
        with pytest.raises(ValueError, match="k_test = .* exceeds the .* indexed images"):
            lazy.images_for_texts([0], 1)
        first = lazy.texts_for_images([0], 1)  # (builds the padded tokens and the cache of the first batch)
        assert first.ids.shape == (1, 1)
        for b in batches[1:]:
            lazy.add_images(b)
        assert _same(lazy.lists("i2t"), l_i2t) and _same(lazy.lists("t2i"), l_t2i)
        # ---- new images: a batch scored with its own tokens is the evaluation of that batch alone
        alone = BlipSearcher(model, temperature=T, k_test=k_test).add_texts(ids, att).add_images(batches[0])
        q = s.query_images(batches[0], k_test)
        assert all(torch.equal(a, b) for a, b in zip(q, alone.texts_for_images(None, k_test)))


def test_searcher_refusals():
    from madtp_amd import build, hip, harness
    from madtp_amd.blip_search import BlipSearcher
    build.build(verbose=False)
    hip.load()
    with pytest.raises(ValueError, match="coarse"):
        BlipSearcher(None, k_test=129, coarse="bf16")
    with pytest.raises(ValueError, match="coarse = 'int8'"):
        BlipSearcher(None, k_test=8, coarse="int8")
    with pytest.raises(ValueError, match="k_test = 257"):
        BlipSearcher(None, k_test=257)
    s = BlipSearcher(None, k_test=4)
    ids = torch.zeros(2, 35, dtype=torch.long)
    with pytest.raises(ValueError, match="no images are indexed"):
        s.query_texts(ids.cuda(), ids.cuda(), 1)
    with pytest.raises(ValueError, match="no texts are indexed"):
        s.query_images(torch.zeros(1, 3, 8, 8, device="cuda"), 1)
    with pytest.raises(ValueError, match="must be indexed before"):
        s.texts_for_images(None, 1)
    with pytest.raises(ValueError, match="image_batch must be a GPU tensor"):
        s.add_images(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="ids must be a GPU tensor"):
        s.add_texts(ids, ids)
    with pytest.raises(ValueError, match="direction = 'x'"):
        s.lists("x")
    # k_test above the indexed counts, and r above k_test (the fixture's model, two images)
    model = harness.build_retrieval(224, 0)
    batches, tids, tatt = harness.retrieval_inputs(2, 2, 5, 224, 35, 0, device="cuda")
    s = BlipSearcher(model, temperature=6.0, k_test=4).add_images(batches[0]).add_texts(tids, tatt)
    with pytest.raises(ValueError, match="k_test = 4 exceeds the 2 indexed images"):
        s.images_for_texts(None, 1)
    with pytest.raises(ValueError, match="r = 5 outside"):
        s.texts_for_images(None, 5)
    with pytest.raises(ValueError, match="row 2 outside"):
        s.texts_for_images([2], 1)


@pytest.mark.parametrize("case", CASES[:1])
def test_coarse_shortlist_gives_the_same_lists(case):
    from madtp_amd import blip_retrieval as br, runtime
    from madtp_amd.blip_search import BlipSearcher
    model, loader, batches, ids, att, T, k_test = _setup(case)
    with runtime.precision("fp32"):
        l_i2t, l_t2i, _ = br.evaluate(model, loader, DEV, {"k_test": k_test}, T, candidates="device", coarse="bf16", scores="lists")
        s = BlipSearcher(model, temperature=T, k_test=k_test, coarse="bf16")
        for b in batches:
            s.add_images(b)
        s.add_texts(ids, att)
        assert _same(s.lists("i2t"), l_i2t) and _same(s.lists("t2i"), l_t2i)


# ---- no [n_img, n_txt] tensor: measured where such a tensor would show -----------------------------------------------------------
class _Out:
    def __init__(self, h):
        self.last_hidden_state = h


class _TinyModel:
    """evaluate()'s model interface on four-feature tokens (plain torch, a test double): the point is what evaluate() itself
    allocates around the encoder calls, at 128 images x 384 texts, sizes the real encoders cannot reach in seconds"""
    space_dict = tokenizer = None

    def __init__(self):
        g = torch.Generator().manual_seed(0)
        self.w_img, self.w_txt = torch.randn(4, 64, generator=g).cuda(), torch.randn(4, 64, generator=g).cuda()

    def visual_encoder(self, image, space_dict=None, temperature=0):
        cls = image.reshape(image.shape[0], -1)[:, :4]
        return torch.stack([cls, 2 * cls], 1), None

    def text_encoder(self, ids, attention_mask=None, mode=None, encoder_hidden_states=None, **kw):
        h = torch.stack([ids.roll(-j, 1) for j in range(1, 5)], -1).float() * 1e-3
        if encoder_hidden_states is not None:
            h = h + encoder_hidden_states[:, :1, :]
        return _Out(h), None

    def project_image(self, cls):
        return torch.nn.functional.normalize(cls @ self.w_img, dim=-1)

    def project_text(self, cls):
        return torch.nn.functional.normalize(cls @ self.w_txt, dim=-1)

    def itm_score(self, cls):
        return cls.sum(-1)


class _OutsidePeak:
    """torch.cuda.max_memory_allocated over everything but the wrapped calls (the re-ranking's own transients, the same in both
    routes), above a baseline taken when start() is called"""

    def __init__(self):
        self.base, self.peak = None, 0

    def start(self):
        torch.cuda.synchronize()
        self.base = self.peak = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()

    def wrap(self, fn):
        def inner(*a, **kw):
            if self.base is not None:
                self.peak = max(self.peak, torch.cuda.max_memory_allocated())
            out = fn(*a, **kw)
            if self.base is not None:
                torch.cuda.reset_peak_memory_stats()
            return out
        return inner

    def above(self):
        return max(self.peak, torch.cuda.max_memory_allocated()) - self.base


def test_lists_route_allocates_no_dense_matrix(monkeypatch):
    """With scores="lists" evaluate() allocates no tensor of n_img * n_txt elements: torch.cuda.max_memory_allocated stays within
    4 * n * k_test * 16 bytes (n = n_img + n_txt rows of lists) of the baseline taken after the encoders ran, at the first
    topk_embeds call.  The bound is the one the feature was specified with; the size is chosen so that it can tell: at the fixtures' 10 and 18 rows it is 2
    and 4.6 KB, below what a dozen live tensors occupy at the allocator's 512-byte granularity, and the dense matrices there are
    288 bytes.  At 128 x 384, k_test 4, the bound is 131 072 bytes and one dense matrix 196 608: the dense return value of the same
    call must come out above the bound, the lists below it (measured: 43 008 and 424 960 bytes).  Allocations inside the encoder and ITM calls are left out of both
    figures (they are the same calls in both routes)."""
    from madtp_amd import blip_retrieval as br, build, hip, harness, search
    build.build(verbose=False)
    hip.load()
    n_img, n_txt, k_test = 128, 384, 4
    g = torch.Generator().manual_seed(1)
    batches = list(torch.randn(n_img, 3, 2, 2, generator=g).cuda().split(32))
    ids = torch.randint(1000, 30000, (n_txt, 35), generator=g).cuda()
    loader = harness.RetrievalLoader(batches, ids, torch.ones_like(ids))
    model, meter = _TinyModel(), _OutsidePeak()
    model.text_encoder, model.itm_score = meter.wrap(model.text_encoder), meter.wrap(model.itm_score)
    real = search.topk_embeds

    def first_call_starts_the_meter(q, keys, k):
        if meter.base is None:
            meter.start()
        return real(q, keys, k)
    monkeypatch.setattr(search, "topk_embeds", first_call_starts_the_meter)
    bound = 4 * (n_img + n_txt) * k_test * 16
    figures = {}
    for scores in ("lists", "dense"):
        meter.base = None
        out = br.evaluate(model, loader, DEV, {"k_test": k_test}, 0, kv_cache=False, candidates="device", scores=scores)
        figures[scores] = meter.above()
        if scores == "lists":
            kept = out
        del out
    print(f"above the baseline: lists {figures['lists']} B, dense {figures['dense']} B, bound {bound} B")
    assert figures["lists"] <= bound < figures["dense"]
    d_i2t, d_t2i, _ = br.evaluate(model, loader, DEV, {"k_test": k_test}, 0, kv_cache=False, candidates="device")
    assert np.array_equal(_np(kept[0].to_dense()), d_i2t) and np.array_equal(_np(kept[1].to_dense()), d_t2i)
