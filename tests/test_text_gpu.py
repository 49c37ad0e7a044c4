"""The WordPiece tokenizer on the GPU (madtp_amd/text.py, csrc/text.hip) against the recorded ids of the yardstick
(tests/golden/text_wp.npz, tools/make_text_golden.py) and against the host emulation, which runs the same lane routines."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = {
    "caption40": dict(padding='longest', truncation=True, max_length=40),
    "nlvr": dict(padding='longest'),
    "retrieval35": dict(padding='max_length', truncation=True, max_length=35),
    "vqa35": dict(padding='longest', truncation=True, max_length=35),
    "short8": dict(padding='longest', truncation=True, max_length=8),
    "pad8": dict(padding='max_length', truncation=True, max_length=8),
}
FILL = -7


@pytest.fixture(scope="module")
def env():
    from madtp_amd import build, hip, text
    build.build(verbose=False)
    hip.load()
    text.lib()
    g = np.load(os.path.join(ROOT, "tests", "golden", "text_wp.npz"))
    off, raw = g["text_offsets"], g["texts"].tobytes()
    texts = [raw[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]
    out = {"text": text, "g": g}
    for name in ("traps", "big"):
        entries = g[f"vocab_{name}"].tobytes().decode().split("\n")
        out[name] = dict(tok=text.WordPiece(entries, "cuda"), use=[texts[i] for i in g[f"use_{name}"]], counts=g[f"counts_{name}"])
    return out


def selection(v, kw):
    return [t for t, c in zip(v["use"], v["counts"]) if "truncation" in kw or c <= 512]


def same(t, a):
    return torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(a)).to(torch.int64))


@pytest.mark.parametrize("key", list(KEYWORDS))
@pytest.mark.parametrize("name", ["traps", "big"])
def test_mixed_batch_equals_the_yardstick_and_the_emulation(env, name, key):
    v, kw, g = env[name], KEYWORDS[key], env["g"]
    sel = selection(v, kw)
    t = v["tok"](sel, return_tensors="pt", **kw)
    assert t.input_ids.dtype == torch.int64 and t.input_ids.is_cuda and t.to("cuda") is t and t["input_ids"] is t.input_ids
    assert same(t.input_ids, g[f"ids_{name}_{key}"]) and same(t.attention_mask, g[f"mask_{name}_{key}"])
    ids, mask = v["tok"].tables.call_host(sel, **kw)
    assert same(t.input_ids, ids) and same(t.attention_mask, mask)


def test_status_words_and_rows_equal_the_emulation(env):
    """the whole corpus without truncation at the widest row: the text of more than 512 tokens gets E_TOKENS and its count, its
    row stays unwritten; every status word and every row equals the emulation's"""
    v, text = env["big"], env["text"]
    ids, mask, status = v["tok"].encode_raw(v["use"], fill=FILL)
    hids, hmask, hstatus = v["tok"].tables.encode_host(v["use"], canary=FILL)
    assert same(status, hstatus) and same(ids, hids) and same(mask, hmask)
    bad = np.nonzero(hstatus[:, 0])[0]
    assert len(bad) == 1 and hstatus[bad[0], 0] == text.E["TOKENS"] and hstatus[bad[0], 1] == v["counts"][bad[0]] > 512
    assert (hids[bad[0]] == FILL).all() and np.array_equal(hstatus[:, 1], v["counts"])


@pytest.mark.parametrize("B", [1, 2, 65])
def test_batch_sizes(env, B):
    """batches of B from the head, the middle and the tail of the corpus (the tail holds the limit texts and the token counts around
    max_length): ids, masks and status words equal to the fixture and to the emulation of the same batch"""
    v, g = env["big"], env["g"]
    use, counts = v["use"], v["counts"]
    want, wmask = g["ids_big_retrieval35"], g["mask_big_retrieval35"]
    for start in (0, 10, 17, len(use) - B - 7, len(use) - B):
        batch = use[start:start + B]
        ids, mask, status = v["tok"].encode_raw(batch, 35, 35, True, fill=FILL)
        hids, hmask, hstatus = v["tok"].tables.encode_host(batch, 35, 35, True, canary=FILL)
        assert same(ids, hids) and same(mask, hmask) and same(status, hstatus)
        assert same(ids, want[start:start + B]) and same(mask, wmask[start:start + B])
        assert not hstatus[:, 0].any() and np.array_equal(hstatus[:, 1], counts[start:start + B])


def test_batches_of_one(env):
    """EVERY text alone, at the widest row without truncation: ids, mask and status words equal to the emulation of that text alone
    and to the fixture (the yardstick's row at padding='longest', [PAD] behind it; its token count; E_TOKENS for the one text of more
    than 512 tokens, whose row stays unwritten)"""
    v, g, text = env["big"], env["g"], env["text"]
    tok, pad = v["tok"], v["tok"].pad_token_id
    want, wmask = g["ids_big_nlvr"], g["mask_big_nlvr"]
    row = 0
    for t, count in zip(v["use"], v["counts"]):
        ids, mask, status = tok.encode_raw([t], fill=FILL)
        hids, hmask, hstatus = tok.tables.encode_host([t], canary=FILL)
        assert same(ids, hids) and same(mask, hmask) and same(status, hstatus), t[:40]
        if count > 512:
            assert hstatus.tolist() == [[text.E["TOKENS"], count]] and (hids == FILL).all() and (hmask == FILL).all()
            continue
        w = want.shape[1]
        assert hstatus.tolist() == [[0, count]], t[:40]
        assert np.array_equal(hids[0, :w], want[row]) and (hids[0, w:] == pad).all(), t[:40]
        assert np.array_equal(hmask[0, :w], wmask[row]) and not hmask[0, w:].any(), t[:40]
        row += 1
    assert row == len(want)
    # and through the call, 'longest': the row is as wide as the text's own tokens
    for b in (0, 5, 10, 11, len(want) - 1):
        t = selection(v, KEYWORDS["nlvr"])[b]
        r = tok([t], return_tensors="pt", **KEYWORDS["nlvr"])
        n = int(wmask[b].sum())
        assert r.input_ids.shape == (1, n) and same(r.input_ids, want[b:b + 1, :n]) and same(r.attention_mask, wmask[b:b + 1, :n])


def test_prompt_without_padding(env):
    for name in ("traps", "big"):
        ids = env[name]["tok"](["a picture of "] * 3, return_tensors="pt").input_ids
        assert same(ids, env["g"][f"ids_{name}_prompt"])


def test_repeats_are_bit_identical(env):
    v = env["big"]
    a = [x.clone() for x in v["tok"].encode_raw(v["use"], 40, 40, True, fill=FILL)]
    for _ in range(3):
        b = v["tok"].encode_raw(v["use"], 40, 40, True, fill=FILL)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_bad_text_raises_naming_its_index(env):
    v, text = env["big"], env["text"]
    good = v["use"][20:28]
    cases = [(b"caf\xc3", "UTF8"), (b"\xc0\xaf", "UTF8"), (b"\xed\xa0\x80", "UTF8"), (b"x" * (text.MAX_BYTES + 1), "LONG"),
             (b"a [SEP] b", "SPECIAL"), ("a \U0001d165 b".encode(), "CHAR"), (" ".join(["a"] * 511).encode(), "TOKENS")]
    for raw, code in cases:
        batch = good[:3] + [raw] + good[3:]
        with pytest.raises(ValueError, match=rf"text 3 .*\(code {text.E[code]}\)"):
            v["tok"](batch, padding='longest', return_tensors="pt")
        ids, mask, status = v["tok"].encode_raw(batch, fill=FILL)
        hids, hmask, hstatus = v["tok"].tables.encode_host(batch, canary=FILL)
        assert same(status, hstatus) and same(ids, hids) and same(mask, hmask)
        assert hstatus[3, 0] == text.E[code] and (hids[3] == FILL).all() and not hstatus[[0, 1, 2, 4, 5, 6, 7, 8], 0].any()
    with pytest.raises(ValueError, match="needs max_length"):
        v["tok"](good, padding='longest', truncation=True, return_tensors="pt")
    with pytest.raises(ValueError):
        v["tok"]([torch.zeros(3)], return_tensors="pt")


def test_cpu_device_raises(env):
    with pytest.raises(RuntimeError, match="no fallback"):
        env["text"].WordPiece(env["big"]["tok"].tables, "cpu")


def test_nlvr_forward_from_strings_equals_forward_from_ids(env):
    """model.tokenizer = text.blip_tokenizer(...) on the smoke test's BLIP_NLVR (vocabulary of 30524 with [DEC] / [ENC] appended):
    the forward from strings is the forward from the same ids, bit for bit"""
    from madtp_amd import blip_nlvr, harness, runtime
    text, v = env["text"], env["big"]
    entries = list(v["tok"].tables.entries)
    entries += [f"[unused{i}]" for i in range(30522 - len(entries))]
    tok = text.blip_tokenizer(entries, "cuda")
    assert (tok.bos_token_id, tok.enc_token_id, tok.additional_special_tokens_ids) == (30522, blip_nlvr.ENC_TOKEN_ID, [30523])
    assert (tok.pad_token_id, tok.cls_token_id, tok.sep_token_id) == (0, 2, 3)
    with pytest.raises(ValueError, match=rf"code {text.E['SPECIAL']}"):
        tok(["a [DEC] b"], padding='longest', return_tensors="pt")
    model = harness.build_nlvr(224, 0, "cuda")
    images, _, targets = harness.nlvr_inputs(2, 224, 20, seed=5)
    strings = [v["use"][60], v["use"][61]]
    t = tok(strings, padding='longest', return_tensors="pt")
    with runtime.precision("fp32"), torch.no_grad():
        from_ids = model(images, {"input_ids": t.input_ids.clone(), "attention_mask": t.attention_mask.clone()}, targets, temperature=5.0, train=False)
        model.tokenizer = tok
        from_strings = model(images, strings, targets, temperature=5.0, train=False)
    assert torch.equal(from_ids, from_strings) and torch.isfinite(from_ids).all()
