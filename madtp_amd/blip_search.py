"""Two-stage BLIP retrieval as an object: shortlist by ITC on the device, re-rank the shortlist with the ITM cross-encoder, return
ordered results.  Built only from what blip_retrieval.evaluate() uses - search.EmbeddingIndex (stage 1, exact or coarse="bf16"),
one text_encoder call per query row over its k_test pairs through EncoderKVCache.select (stage 2), madtp_lists_sort (stage 3) - so
its scores are those of evaluate(candidates="device") over the same images in the same batches and the same texts.

    s = BlipSearcher(model, temperature=0, k_test=128)
    s.add_images(image_batch);  s.add_texts(ids, att)
    res = s.texts_for_images(None, r=10)      # SearchResult(ids int64 [n,r], score f32 [n,r] = ITM + ITC, itc f32 [n,r]), best first
    res = s.query_texts(ids, att, r=10)       # new texts against the indexed images
    cl = s.lists("i2t")                       # lists.CandidateLists: what evaluate(scores="lists") returns

Reference semantics that survive here.  evaluate() pads the image tokens of all batches to the longest batch with copies of the
CLS row, and those rows take part in the cross-attention: a score depends on which other batches are indexed.  The searcher keeps
every batch's tokens as they came and builds the padded tensor and the K/V cache lazily, at the first query after an add_images();
a query between two add_images() calls sees the images indexed so far, a query after them equals evaluate() over all of them.
Texts are encoded in batches of text_bs from the start of every add_texts() call, as evaluate() does from the start of the set, so
one add_texts() call with the whole set is the evaluation.  Text-side pruning inside a k_test batch makes a pair's score depend on
its batch: a query row is always one encoder call, never merged with another row's.  An image given to query_images() is scored
with its own batch's tokens, unpadded: what evaluate() gives for a set of that one batch.

Device tensors only; refusals are ValueErrors before any GPU work."""
from collections import namedtuple

import torch

from . import lists, search
from .bert import EncoderKVCache
from .blip_nlvr import ENC_TOKEN_ID

SearchResult = namedtuple("SearchResult", "ids score itc")


def _on_gpu(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor (no CPU fallback)")
    return t


class BlipSearcher:
    def __init__(self, model, temperature=0, k_test=128, kv_cache=True, coarse=None, text_bs=256):
        k_test = int(k_test)
        if not 1 <= k_test <= lists.MAX_K:
            raise ValueError(f"BlipSearcher: k_test = {k_test} outside [1, {lists.MAX_K}]")
        if coarse is not None:
            search.check_coarse(coarse, k_test, "BlipSearcher: k_test")
        self.model, self.temperature, self.k_test, self.kv_cache, self.coarse = model, temperature, k_test, bool(kv_cache), coarse
        self.text_bs = int(text_bs)
        self._images = self._texts = None  # EmbeddingIndex of the projected CLS rows
        self._feats = []                   # the image tokens of every add_images() batch, as they came
        self._padded = self._cache = None  # what evaluate() makes of them, built at the first query after an add_images()
        self._text_ids = self._text_atts = None

    # ---- indexing --------------------------------------------------------------------------------------------------------------
    @property
    def n_images(self):
        return 0 if self._images is None else len(self._images)

    @property
    def n_texts(self):
        return 0 if self._texts is None else len(self._texts)

    def _index(self, index, embeds):
        embeds = embeds.float()
        return search.EmbeddingIndex(embeds, coarse=self.coarse) if index is None else index.add(embeds)

    @property
    def image_embeds(self):
        """f32 [n_images, D]: the projected CLS rows in the index (None before the first add_images)"""
        return None if self._images is None else self._images.keys

    @property
    def text_embeds(self):
        return None if self._texts is None else self._texts.keys

    @torch.no_grad()
    def _encode_images(self, image):
        _on_gpu(image, "image_batch")
        m = self.model
        feat, _ = m.visual_encoder(image, space_dict=m.space_dict, temperature=self.temperature)
        return feat, m.project_image(feat[:, 0, :])

    @torch.no_grad()
    def _encode_texts(self, ids, att):
        """-> (embeddings, ids with ENC_TOKEN_ID in front, masks)"""
        _on_gpu(ids, "ids"), _on_gpu(att, "att")
        m = self.model
        embeds = []
        for i in range(0, ids.shape[0], self.text_bs):
            out, _ = m.text_encoder(ids[i:i + self.text_bs], attention_mask=att[i:i + self.text_bs], mode='text',
                                    space_dict=m.space_dict, temperature=self.temperature)
            embeds.append(m.project_text(out.last_hidden_state[:, 0, :]))
        enc_ids = ids.clone()
        enc_ids[:, 0] = ENC_TOKEN_ID
        return torch.cat(embeds, 0), enc_ids, att

    def add_images(self, image_batch):
        """one loader batch: the visual encoder, project_image into the index; the batch's image tokens are kept as they came"""
        feat, embeds = self._encode_images(image_batch)
        self._images = self._index(self._images, embeds)
        self._feats.append(feat)
        self._padded = self._cache = None
        return self

    def add_texts(self, ids, att):
        """token ids and masks as the tokenizer yields them: the text-mode encoder in batches of text_bs, project_text into the
        index; the ids (with ENC_TOKEN_ID in front) and masks are kept for the re-ranking"""
        embeds, enc_ids, att = self._encode_texts(ids, att)
        self._texts = self._index(self._texts, embeds)
        self._text_ids = enc_ids if self._text_ids is None else torch.cat([self._text_ids, enc_ids], 0)
        self._text_atts = att.clone() if self._text_atts is None else torch.cat([self._text_atts, att], 0)
        return self

    # ---- the three stages ------------------------------------------------------------------------------------------------------
    def _shortlist(self, index, what, q):
        if index is None:
            raise ValueError(f"BlipSearcher: no {what} are indexed yet")
        if self.k_test > len(index):
            raise ValueError(f"BlipSearcher: k_test = {self.k_test} exceeds the {len(index)} indexed {what}")
        return index.search(q.float(), self.k_test)

    @staticmethod
    def _pad(feats):
        """blip_retrieval.evaluate(): batches pruned to different lengths, padded with their CLS row"""
        n = max(f.shape[1] for f in feats)
        return torch.cat([torch.cat([f, f[:, 0:1, :].expand(-1, n - f.shape[1], -1)], 1) if f.shape[1] < n else f for f in feats], 0)

    def _image_tokens(self):
        if self._padded is None:
            self._padded = self._pad(self._feats)
            self._cache = EncoderKVCache.build(self.model.text_encoder, self._padded) if self.kv_cache else None
        return self._padded, self._cache

    @torch.no_grad()
    def _rerank(self, ids, att, img_index, tokens):
        """the rerank closure of evaluate(): ITM scores of k_test (text, image) pairs from one text_encoder call"""
        m = self.model
        feats, cache = tokens
        if cache is not None:
            out = m.text_encoder(ids, attention_mask=att, return_dict=True, space_dict=m.space_dict, temperature=self.temperature,
                                 encoder_kv_cache=cache.select(img_index))[0]
        else:
            enc = feats[img_index].contiguous()
            enc_att = torch.ones(enc.shape[:-1], dtype=torch.long, device=enc.device)
            out = m.text_encoder(ids, attention_mask=att, encoder_hidden_states=enc, encoder_attention_mask=enc_att,
                                 return_dict=True, space_dict=m.space_dict, temperature=self.temperature)[0]
        return m.itm_score(out.last_hidden_state[:, 0, :])

    def _texts_of(self, image_rows, sim, idx, tokens):
        """stage 2, images as queries: row i of (sim, idx) is image image_rows[i] of `tokens` against the indexed texts idx[i]"""
        k, val = self.k_test, torch.empty_like(sim)
        for i, row in enumerate(image_rows):
            val[i] = self._rerank(self._text_ids[idx[i]], self._text_atts[idx[i]],
                                  torch.full((k,), row, dtype=torch.long, device=sim.device), tokens) + sim[i]
        return val

    def _images_of(self, ids, att, sim, idx):
        """stage 2, texts as queries: row i of (sim, idx) is text (ids[i], att[i]) against the indexed images idx[i]"""
        k, val, tokens = self.k_test, torch.empty_like(sim), self._image_tokens()
        for i in range(sim.shape[0]):
            val[i] = self._rerank(ids[i].repeat(k, 1), att[i].repeat(k, 1), idx[i], tokens) + sim[i]
        return val

    def _check_r(self, r):
        r = int(r)
        if not 1 <= r <= self.k_test:
            raise ValueError(f"BlipSearcher: r = {r} outside [1, k_test = {self.k_test}]")
        return r

    def _rows(self, rows, n):
        if rows is None:
            return list(range(n))
        rows = [int(r) for r in (rows.tolist() if torch.is_tensor(rows) else rows)]
        for r in rows:
            if not 0 <= r < n:
                raise ValueError(f"BlipSearcher: row {r} outside [0, {n})")
        if not rows:
            raise ValueError("BlipSearcher: no query rows")
        return rows

    def _two_stage(self, direction, rows):
        """-> (CandidateLists of the rows, their ITC scores [n, k_test])"""
        if direction not in ("i2t", "t2i"):
            raise ValueError(f"direction = {direction!r}: expected 'i2t' or 't2i'")
        if self._images is None or self._texts is None:
            raise ValueError("BlipSearcher: images and texts must be indexed before a query over indexed rows")
        if direction == "i2t":
            rows = self._rows(rows, self.n_images)
            sim, idx = self._shortlist(self._texts, "texts", self._images.keys[rows])
            return lists.CandidateLists(idx, self._texts_of(rows, sim, idx, self._image_tokens()), self.n_texts), sim
        rows = self._rows(rows, self.n_texts)
        sim, idx = self._shortlist(self._images, "images", self._texts.keys[rows])
        return lists.CandidateLists(idx, self._images_of(self._text_ids[rows], self._text_atts[rows], sim, idx), self.n_images), sim

    def _result(self, cl, sim, r):
        """stage 3: the lists in the contract order of madtp_search.h, their first r columns, and the ITC term of every result"""
        best = cl.sorted()
        # the ITC score of a key follows it: both rows hold the same keys, so their ascending orders pair the positions
        itc = torch.empty_like(sim).scatter_(1, best.idx.argsort(dim=1), sim.gather(1, cl.idx.argsort(dim=1)))
        return SearchResult(best.idx[:, :r], best.val[:, :r], itc[:, :r])

    # ---- queries ---------------------------------------------------------------------------------------------------------------
    def lists(self, direction, rows=None):
        """the re-ranked candidate lists of indexed images ("i2t") or indexed texts ("t2i") as queries; rows=None: all of them,
        which is what evaluate(candidates="device", scores="lists") returns for that direction"""
        return self._two_stage(direction, rows)[0]

    def texts_for_images(self, rows=None, r=10):
        r = self._check_r(r)
        return self._result(*self._two_stage("i2t", rows), r)

    def images_for_texts(self, rows=None, r=10):
        r = self._check_r(r)
        return self._result(*self._two_stage("t2i", rows), r)

    def query_texts(self, ids, att, r=10):
        """new texts (token ids and masks as the tokenizer yields them) against the indexed images"""
        r = self._check_r(r)
        _on_gpu(ids, "ids"), _on_gpu(att, "att")
        if self._images is None:
            raise ValueError("BlipSearcher: no images are indexed yet")
        embeds, enc_ids, att = self._encode_texts(ids, att)
        sim, idx = self._shortlist(self._images, "images", embeds)
        return self._result(lists.CandidateLists(idx, self._images_of(enc_ids, att, sim, idx), self.n_images), sim, r)

    def query_images(self, image_batch, r=10):
        """new images (one batch) against the indexed texts; the batch's own tokens, unpadded"""
        r = self._check_r(r)
        _on_gpu(image_batch, "image_batch")
        if self._texts is None:
            raise ValueError("BlipSearcher: no texts are indexed yet")
        feat, embeds = self._encode_images(image_batch)
        sim, idx = self._shortlist(self._texts, "texts", embeds)
        tokens = (feat, EncoderKVCache.build(self.model.text_encoder, feat) if self.kv_cache else None)
        val = self._texts_of(range(feat.shape[0]), sim, idx, tokens)
        return self._result(lists.CandidateLists(idx, val, self.n_texts), sim, r)
