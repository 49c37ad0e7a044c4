"""CPU side of the WordPiece tokenizer (madtp_amd/text.py, csrc/madtp_text.h): the header against the binding, the character table
against a fresh recording, the restatement of tests/text_ref.py against the live yardstick, and the kernel's lane routines run on the
host (madtp_text_encode_host) against the recorded ids, with every refusal into buffers with canaries.  No GPU."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest

from tests import text_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYWORDS = {
    "caption40": dict(padding='longest', truncation=True, max_length=40),
    "nlvr": dict(padding='longest'),
    "retrieval35": dict(padding='max_length', truncation=True, max_length=35),
    "vqa35": dict(padding='longest', truncation=True, max_length=35),
    "short8": dict(padding='longest', truncation=True, max_length=8),
    "pad8": dict(padding='max_length', truncation=True, max_length=8),
}
CANARY = -7
NAMES = "abi_version strerror chartable_check vocab_bytes vocab_build encode_batch encode_host".split()


@pytest.fixture(scope="module")
def env():
    from madtp_amd import build, text
    build.build(verbose=False)
    text.lib()
    g = np.load(os.path.join(ROOT, "tests", "golden", "text_wp.npz"))
    off, raw = g["text_offsets"], g["texts"].tobytes()
    texts = [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    out = {"text": text, "g": g}
    for name in ("traps", "big"):
        entries = g[f"vocab_{name}"].tobytes().decode().split("\n")
        out[name] = dict(entries=entries, tables=text.Tables(entries), use=[texts[i] for i in g[f"use_{name}"]], counts=g[f"counts_{name}"])
    return out


def selection(v, kw):
    return [t for t, c in zip(v["use"], v["counts"]) if "truncation" in kw or c <= 512]


def yardstick(entries, tmp_path):
    transformers = pytest.importorskip("transformers")
    path = os.path.join(str(tmp_path), "vocab.txt")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(entries) + "\n")
    return transformers.BertTokenizer(path)


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
def test_header_binding_and_build_lists(env):
    from madtp_amd import abi, build
    text = env["text"]
    src = re.sub(r"/\*.*?\*/", "", open(text.HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))
    assert syms == sorted(text.SIGNATURES) == sorted("madtp_text_" + s for s in NAMES)
    raw = ctypes.CDLL(build.build(verbose=False))
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in csrc/madtp_text.h but not exported"
    assert text.lib().madtp_text_abi_version() == text.ABI_VERSION == 1
    i, p, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert text.SIGNATURES["madtp_text_encode_batch"] == (i, [p, p, p, p, p, p, p, i, i, i, i, p])
    assert text.SIGNATURES["madtp_text_encode_host"] == (i, [p, p, p, p, p, p, p, i, i, i, i])
    assert text.SIGNATURES["madtp_text_vocab_bytes"] == (i64, [p, p, i, i])
    assert (text.MAX_BYTES, text.MAX_TOKENS, text.MAX_WORD_CHARS) == (ref.MAX_BYTES, ref.MAX_TOKENS, ref.MAX_WORD) and text.MAX_BYTES >= 1024
    assert {k: text.E[k] for k in ("LONG", "UTF8", "SPECIAL", "CHAR", "TOKENS")} == \
        dict(LONG=ref.E_LONG, UTF8=ref.E_UTF8, SPECIAL=ref.E_SPECIAL, CHAR=ref.E_CHAR, TOKENS=ref.E_TOKENS)
    assert len(set(text.E.values())) == len(text.E) and all(text.lib().madtp_text_strerror(c) for c in text.E.values())
    assert not set(abi.SIGNATURES) & set(syms)
    assert "text.hip" in build.SOURCES and "text_device.h" in build.HEADERS and "madtp_text.h" in build.HEADERS
    assert not os.path.exists(os.path.join(ROOT, "include", "madtp_text.h"))


# ---- the character table -----------------------------------------------------------------------------------------------------------------
def test_committed_table_is_small_and_checked(env):
    text = env["text"]
    assert os.path.getsize(text.CHARTABLE) < 256 * 1024
    table = text.chartable()
    assert text.lib().madtp_text_chartable_check(table.ctypes.data, table.size) == 0
    f = text.read_chartable()
    assert f["max_expand"] == [1, 1, 3, 3] == table[3:7].tolist() and f["tokenizers_version"] == "0.22.2" and f["refused"] == 83
    with open(text.CHARTABLE, "rb") as raw:
        assert all(b == 10 or 32 <= b < 127 for b in raw.read()), "the table file is plain text"
    broken = table.copy()
    broken[3] = 2  # a one-byte codepoint that expands to two: the LDS arrays would not hold the text
    assert text.lib().madtp_text_chartable_check(broken.ctypes.data, broken.size) == text.E["TABLE"]
    assert text.lib().madtp_text_chartable_check(table.ctypes.data, table.size - 1) == text.E["TABLE"]


def test_committed_table_equals_a_fresh_recording(env):
    pytest.importorskip("tokenizers")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_bert_chartable
    finally:
        sys.path.pop(0)
    with open(env["text"].CHARTABLE, encoding="ascii") as have:
        assert have.read() == make_bert_chartable.render(make_bert_chartable.generate())


POOL = "abcXYZ .,-'!?éÉñüÅİıΣσςΑß़्ְּ̣́̈कא한글가中文　\u0085 ​�\x00\t\n" \
       "〮〯\U0001d165\U0001d16d\U0001f600กั€"


def test_per_codepoint_normalisation_composes(env):
    """20 000 seeded strings: the table's normalisation, one codepoint at a time, is the yardstick's normalize_str of the whole
    string; a string with a REFUSE codepoint (a kept mark that NFD moves) is refused instead"""
    tokenizers = pytest.importorskip("tokenizers")
    norm = tokenizers.normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True)
    table = ref.CharTable()
    rng = random.Random(7)
    refused = 0
    for _ in range(20000):
        s = "".join(rng.choice(POOL) for _ in range(rng.randint(1, 16)))
        if any(table.outputs(ord(c)) is None for c in s):
            refused += 1
            with pytest.raises(ref.Refused):
                table.normalize(s)
            continue
        assert table.normalize_str(s) == norm.normalize_str(s), repr(s)
    assert 1000 < refused < 15000
    assert all(table.outputs(ord(c)) is None for c in "〮〯\U0001d165\U0001d16d")


# ---- ids ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["traps", "big"])
def test_restatement_equals_the_live_yardstick(env, name, tmp_path):
    v = env[name]
    tok = yardstick(v["entries"], tmp_path)
    r = ref.Tokenizer(v["entries"])
    for raw, count in zip(v["use"], v["counts"]):
        want = tok(raw.decode()).input_ids
        assert [r.cls] + r.tokens(raw) + [r.sep] == want and len(want) == count


@pytest.mark.parametrize("key", list(KEYWORDS))
@pytest.mark.parametrize("name", ["traps", "big"])
def test_host_emulation_equals_the_recorded_ids(env, name, key):
    v, kw, g = env[name], KEYWORDS[key], env["g"]
    sel = selection(v, kw)
    ids, mask = v["tables"].call_host(sel, **kw)
    assert ids.dtype == np.int64 and np.array_equal(ids, g[f"ids_{name}_{key}"]) and np.array_equal(mask, g[f"mask_{name}_{key}"])
    rids, rmask, _ = ref.Tokenizer(v["entries"]).encode(sel, ids.shape[1], kw.get("max_length", 512), "truncation" in kw)
    assert np.array_equal(np.array(rids), ids) and np.array_equal(np.array(rmask), mask)


def test_host_emulation_status_words_and_prompt(env):
    v = env["big"]
    ids, mask, status = v["tables"].encode_host(v["use"], canary=CANARY)
    assert np.array_equal(status[:, 1], v["counts"])
    bad = np.nonzero(status[:, 0])[0]
    assert len(bad) == 1 and status[bad[0], 0] == env["text"].E["TOKENS"] and (ids[bad[0]] == CANARY).all() and (mask[bad[0]] == CANARY).all()
    for name in ("traps", "big"):
        got, _ = env[name]["tables"].call_host(["a picture of "] * 3)
        assert np.array_equal(got, env["g"][f"ids_{name}_prompt"])
    with pytest.raises(ValueError, match="do not make a tensor"):
        v["tables"].call_host(["a", "a a"])
    with pytest.raises(ValueError, match="needs max_length"):
        v["tables"].call_host(["a"], padding='longest', truncation=True)


def encode_exact(text, tables, data, begin, end, width=16, max_tokens=16, flags=0):
    """one text at data[begin:end] of a buffer that goes on behind it -> (ids row, mask row, status) with canaries around the row"""
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    off = np.array([begin, end], dtype=np.int64)
    ids = np.full((3, width), CANARY, dtype=np.int64)
    mask = np.full((3, width), CANARY, dtype=np.int64)
    status = np.full((3, 2), CANARY, dtype=np.int32)
    rc = text.lib().madtp_text_encode_host(buf.ctypes.data, off.ctypes.data, tables.chartable.ctypes.data, tables.vocab.ctypes.data,
                                          ids[1].ctypes.data, mask[1].ctypes.data, status[1].ctypes.data, 1, width, max_tokens, flags)
    assert rc == 0
    for a in (ids, mask, status):
        assert (a[0] == CANARY).all() and (a[2] == CANARY).all(), "a write outside the row"
    return ids[1], mask[1], status[1]


MALFORMED = [
    ("truncated 2-byte", b"ab\xc3", b"\xa9"), ("truncated 3-byte", b"ab\xe4\xb8", b"\xad"), ("truncated 3-byte at its lead", b"ab\xe4", b"\xb8\xad"),
    ("truncated 4-byte", b"ab\xf0\x9f\x98", b"\x80"), ("truncated 4-byte at its lead", b"\xf0", b"\x9f\x98\x80"),
    ("overlong 2-byte", b"\xc0\xaf", b""), ("overlong 3-byte", b"a\xe0\x80\xaf", b""), ("overlong 4-byte", b"\xf0\x80\x80\xaf", b""),
    ("surrogate", b"a\xed\xa0\x80b", b""), ("above U+10FFFF", b"\xf4\x90\x80\x80", b""), ("a lone continuation byte", b"a\x80b", b""),
    ("a fourth continuation byte", b"\xe4\xb8\xad\xad", b""), ("0xFF", b"a\xffb", b""), ("a lead after a lead", b"\xc3\xc3\xa9", b""),
]


@pytest.mark.parametrize("what,raw,behind", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_utf8_is_refused_and_nothing_is_written(env, what, raw, behind):
    """`behind`: bytes of the buffer past the text's extent that would complete the sequence - a decoder that read them would accept"""
    text, tables = env["text"], env["big"]["tables"]
    ids, mask, status = encode_exact(text, tables, b"xy" + raw + behind, 2, 2 + len(raw))
    assert status.tolist() == [text.E["UTF8"], 0] and (ids == CANARY).all() and (mask == CANARY).all()
    with pytest.raises(ref.Refused) as e:
        ref.Tokenizer(env["big"]["entries"]).tokens(raw)
    assert e.value.code == ref.E_UTF8


def test_every_other_code_on_its_case(env):
    """each text with b"[SEP]" behind its extent; the restatement says which code, which count and which row"""
    text, tables = env["text"], env["big"]["tables"]
    E, r = text.E, ref.Tokenizer(env["big"]["entries"])
    at_limit = b"x" * 101 + b" " + b"y" * (text.MAX_BYTES - 102)
    cases = [(at_limit, 0, 0), (at_limit + b"y", 0, E["LONG"]), (" ".join(["a"] * 510).encode(), 0, 0),
             (" ".join(["a"] * 511).encode(), 0, E["TOKENS"]), (" ".join(["a"] * 511).encode(), text.TRUNCATE, 0),
             (b"a [SEP] b", 0, E["SPECIAL"]), (b"[CLS]", 0, E["SPECIAL"]), (b"x[MASK]", 0, E["SPECIAL"]), (b"[MASK", 0, 0), (b"a [sep] b", 0, 0),
             ("a\U0001d165".encode(), 0, E["CHAR"]), ("\u302e".encode(), 0, E["CHAR"]),
             (b"\xff [SEP] \xf0\x9d\x85\xa5", 0, E["UTF8"]), (b"[SEP] \xf0\x9d\x85\xa5", 0, E["SPECIAL"])]
    for raw, flags, code in cases:
        ids, mask, status = encode_exact(text, tables, raw + b"[SEP]", 0, len(raw), 512, 512, flags)
        rids, rmask, rstatus = r.encode([raw], 512, 512, bool(flags))
        assert status.tolist() == list(rstatus[0]) and status[0] == code, (raw[:20], status, rstatus)
        if code:
            assert (ids == CANARY).all() and (mask == CANARY).all() and rids[0] is None
        else:
            assert ids.tolist() == rids[0] and mask.tolist() == rmask[0]
    lib = text.lib()
    ok = np.zeros(64, dtype=np.int64)
    p = ok.ctypes.data
    for B, width, max_tokens, flags in ((0, 8, 8, 0), (1, 513, 8, 0), (1, 8, 9, 0), (1, 8, 1, 0), (1, 8, 8, 2)):
        assert lib.madtp_text_encode_host(p, p, tables.chartable.ctypes.data, tables.vocab.ctypes.data, p, p, p, B, width, max_tokens, flags) != 0
    assert (ok == 0).all()


# ---- the vocabulary builder ------------------------------------------------------------------------------------------------------------
def test_vocabulary_refusals(env):
    text = env["text"]
    base = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "##a"]
    text.build_vocab(base)
    for entries, code in ((base + ["a"], "VOCAB_DUP"), (base + ["##a"], "VOCAB_DUP"), (base + [""], "VOCAB_EMPTY"),
                          (base[:3] + base[4:], "VOCAB_MISSING"), (base + ["x" * 257], "VOCAB_ENTRY")):
        with pytest.raises(ValueError, match=rf"code {text.E[code]}\)"):
            text.build_vocab(entries)
    with pytest.raises(ValueError, match=rf"code {text.E['VOCAB_ENTRY']}\)"):
        text.build_vocab(base, specials=[99])
    with pytest.raises(ValueError, match="not entries"):
        text.Tables(base, extra_specials=("[DEC]",))
    with pytest.raises(ValueError, match="cased"):
        text.Tables(base, lowercase=False)
    v = text.build_vocab(base + ["[DEC]"], specials=[6])
    assert [int(v[text._V[k]]) for k in ("PAD", "UNK", "CLS", "SEP", "ENTRIES", "LONGEST", "SPECIALS")] == [0, 1, 2, 3, 7, 5, 5]
    assert int(v[text._V["WORDS"]]) == v.size and int(v[text._V["SLOTS"]]) >= 14
    # "##a" and "a" are different keys, and a hit is confirmed in the pool: a table whose pool is damaged finds nothing
    t = text.Tables(base)
    ids, _, _ = t.encode_host(["aa a"], 8)
    assert ids[0].tolist() == [2, 4, 5, 4, 3, 0, 0, 0]
    t.vocab = t.vocab.copy()
    pool = int(t.vocab[text._V["OFF_POOL"]])
    t.vocab[pool:pool + int(t.vocab[text._V["POOL"]])] += 1
    ids, _, _ = t.encode_host(["aa a"], 8)
    assert ids[0].tolist() == [2, 1, 1, 3, 0, 0, 0, 0]


def test_blip_entries_and_without_a_gpu_the_object_raises(env):
    import torch
    text = env["text"]
    entries = text.blip_entries(env["traps"]["entries"])
    assert entries[-2:] == ["[DEC]", "[ENC]"] and text.blip_entries(entries) == entries
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no fallback"):
            text.WordPiece(entries, "cuda")
    with pytest.raises(RuntimeError, match="no fallback"):
        text.WordPiece(entries, "cpu")


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
def test_decode_equals_the_yardstick(env, tmp_path):
    v = env["big"]
    tok = yardstick(v["entries"], tmp_path)
    rows = [r for r in env["g"]["ids_big_nlvr"]] + [r for r in env["g"]["ids_big_short8"][:60]]
    words = "d ##o n ##o ##t , . ' s ! ? n ' t i ' m w ##e ' v ##e ' r ##e a b".split()
    ids = v["tables"].ids
    rows.append(np.array([2] + [ids[w] for w in words] + [3]))
    for row in rows:
        for skip in (True, False):
            assert v["tables"].decode(row, skip_special_tokens=skip) == tok.decode(row, skip_special_tokens=skip), row[:12]
