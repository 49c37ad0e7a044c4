"""Records tests/golden/text_wp.npz: vocabularies, texts (UTF-8 bytes) and the ids / masks the installed transformers.BertTokenizer
gives them at every keyword set the models call their tokenizer with.

    python tools/make_text_golden.py [--dump DIR]     # --dump: chartable.bin, vocab.txt (the big one) and texts.bin for
                                                      # tools/text_host_check.cpp, from the committed files; records nothing

The real vocab.txt is not at hand, so the vocabularies are synthetic: "traps" (hand-made, longest-match traps) and "big" (about
30 k entries: printable ASCII in both forms, random substrings of a seeded word list, entries only reachable after accent stripping
and lower-casing, Greek, CJK singles, a 24-character piece).  The recorder asserts what its corpus covers."""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "text_wp.npz")
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
MAX_BYTES = 2048
LONG_PIECE = "abcdefghijklmnopqrstuvwx"
# name -> the keyword set; the first five are the models' (blip.py:60, blip_nlvr.py:65, blip_retrieval.py:359, blip_vqa.py:52)
KEYWORDS = {
    "caption40": dict(padding='longest', truncation=True, max_length=40),
    "nlvr": dict(padding='longest'),
    "retrieval35": dict(padding='max_length', truncation=True, max_length=35),
    "vqa35": dict(padding='longest', truncation=True, max_length=35),
    "short8": dict(padding='longest', truncation=True, max_length=8),
    "pad8": dict(padding='max_length', truncation=True, max_length=8),
}


def word_list(rng, n):
    cons, vow = "bcdfghjklmnprstvwz", "aeiou"
    words = set()
    while len(words) < n:
        words.add("".join(rng.choice(cons) + rng.choice(vow) + (rng.choice(cons) if rng.random() < 0.3 else "") for _ in range(rng.randint(1, 5))))
    return sorted(words)


def traps_vocab():
    return SPECIALS + ["ab", "abc", "##cd", "##d", "##c", "a", "b", "c", "d", "##a", "##b", "e", "##e", ",", ".", "!", "x", "##xy", "abcx", "##ab"]


def big_vocab(rng, words):
    entries = list(SPECIALS)
    for c in range(33, 127):
        entries += [chr(c), "##" + chr(c)]
    entries += ["cafe", "uber", "istanbul", "##nbul", "resume", "angstrom", "οδοσ", "οδος", "##ς", "##σ", "σ", "ο", "##ο", "##δ", "λογ", "##οσ",
                "中", "文", "字", "日", "本", LONG_PIECE, "##" + LONG_PIECE[:20], "한", "ᄒ", "##ᅡ", "##ᆫ"]
    seen = set(entries)
    while len(entries) < 30000:
        w = rng.choice(words)
        a = rng.randrange(len(w))
        b = rng.randint(a + 1, min(len(w), a + 6))
        piece = ("##" if a or rng.random() < 0.25 else "") + w[a:b]
        if piece not in seen:
            seen.add(piece)
            entries.append(piece)
        if len(seen) > 29000 and rng.random() < 0.001:
            break
    return entries


def corpus(rng, words):
    texts = ["", "   ", " \t\n ", ".,!?;:", "...", "abcd abd abcx abcxy abab, abc. e!", "Café ÜBER İstanbul résumé Ångström", "ΟΔΟΣ οδος ΛΟΓΟΣ σ",
             "中文字 日本x 한", "tab\tnew\nline\r\x00nul ​ zero � repl \u0085  ", "a" * 100, "a" * 101, "x " + "b" * 100 + " y " + "c" * 101,
             LONG_PIECE, LONG_PIECE + "y " + LONG_PIECE[:23], "hello-world's (test) [brackets] #hash ##double", "é ạ̈ ño"]
    for w in rng.sample(words, 40):  # words that fail only at their last character, and in the middle
        texts.append(f"{w}ж {w} {w[:1]}ж{w[1:]} ж")
    for _ in range(200):  # caption-like
        n = rng.randint(3, 16)
        ws = []
        for _ in range(n):
            w = rng.choice(words)
            r = rng.random()
            if r < 0.08:
                w += rng.choice("жщю€")
            elif r < 0.2:
                w = w.capitalize()
            elif r < 0.25:
                w += rng.choice(",.!?")
            ws.append(w)
        texts.append(" ".join(ws))
    filler = " ".join(rng.choice(words) for _ in range(400))
    for n in (255, 256, 257):
        texts.append(filler[:n])
    texts.append(((LONG_PIECE + " ") * 90)[:MAX_BYTES])  # the byte limit, and the normalised limit
    texts.append(("中" * 700)[:MAX_BYTES // 3] )           # 682 three-byte characters: 2046 bytes, more than 512 tokens
    for count in (5, 6, 7, 8, 9, 32, 33, 34, 35, 36):     # token counts max_length - 3 .. max_length + 1 at 8 and 35
        texts.append(" ".join(["a"] * (count - 2)))
    return texts


def tokenizer(entries, tmp):
    import transformers
    path = os.path.join(tmp, f"vocab{len(entries)}.txt")
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(entries) + "\n")
    return transformers.BertTokenizer(path)


def coverage(tok, texts, unk):
    words = split = unks = 0
    for t in texts:
        enc = tok.backend_tokenizer.encode(t, add_special_tokens=False)
        per = {}
        for wid, i in zip(enc.word_ids, enc.ids):
            per.setdefault(wid, []).append(i)
        words += len(per)
        split += sum(len(v) > 1 for v in per.values())
        unks += sum(v == [unk] for v in per.values())
    return words, split, unks


def dump(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    g = np.load(OUT)
    sys.path.insert(0, os.path.dirname(HERE))
    from madtp_amd import text
    text.read_chartable()["table"].tofile(os.path.join(out_dir, "chartable.bin"))
    with open(os.path.join(out_dir, "vocab.txt"), "wb") as f:
        f.write(g["vocab_big"].tobytes() + b"\n")
    off = g["text_offsets"].astype(np.int64)
    with open(os.path.join(out_dir, "texts.bin"), "wb") as f:
        f.write(np.array([off.size - 1], dtype=np.int64).tobytes() + off.tobytes() + g["texts"].tobytes())
    print(out_dir, off.size - 1, "texts")
    return 0


def main():
    if "--dump" in sys.argv:
        return dump(sys.argv[sys.argv.index("--dump") + 1])
    rng = random.Random(20240611)
    words = word_list(rng, 3000)
    vocabs = {"traps": traps_vocab(), "big": big_vocab(rng, words)}
    texts = corpus(rng, words)
    out = {"texts": np.frombuffer(b"".join(t.encode() for t in texts), dtype=np.uint8),
           "text_offsets": np.cumsum([0] + [len(t.encode()) for t in texts]).astype(np.int64)}
    with tempfile.TemporaryDirectory() as tmp:
        for name, entries in vocabs.items():
            assert len(set(entries)) == len(entries)
            tok = tokenizer(entries, tmp)
            out[f"vocab_{name}"] = np.frombuffer("\n".join(entries).encode(), dtype=np.uint8)
            use = [t for t in texts if name == "big" or len(t) < 200]
            out[f"use_{name}"] = np.array([texts.index(t) for t in use], dtype=np.int32)
            counts = [len(tok(t).input_ids) for t in use]
            out[f"counts_{name}"] = np.array(counts, dtype=np.int32)
            for key, kw in KEYWORDS.items():
                sel = [t for t, c in zip(use, counts) if "truncation" in kw or c <= 512]
                r = tok(sel, return_tensors="np", **kw)
                out[f"ids_{name}_{key}"] = r["input_ids"].astype(np.int32)
                out[f"mask_{name}_{key}"] = r["attention_mask"].astype(np.int8)
            r = tok(["a picture of "] * 3, return_tensors="np")
            out[f"ids_{name}_prompt"] = r["input_ids"].astype(np.int32)
            if name == "big":
                n_words, split, unks = coverage(tok, use, entries.index("[UNK]"))
                assert split >= 0.30 * n_words, (split, n_words)
                assert unks >= 0.05 * n_words, (unks, n_words)
                w = words[0]
                assert tok.tokenize(w + "ж") == ["[UNK]"] and tok.tokenize(w) != ["[UNK]"], "a word that fails only at its last character"
                assert len(tok.tokenize("a" * 100)) == 100 and tok.tokenize("a" * 101) == ["[UNK]"]
                assert {255, 256, 257, MAX_BYTES} <= {len(t) for t in use} and "" in use and "   " in use and ".,!?;:" in use
                assert max(len(t.encode()) for t in use) == MAX_BYTES
                assert max(counts) > 512 and {5, 6, 7, 8, 9, 32, 33, 34, 35, 36} <= set(counts)
                print(f"big: {len(entries)} entries, {len(use)} texts, {n_words} words, {split} split ({split / n_words:.0%}), "
                      f"{unks} [UNK] ({unks / n_words:.0%}), token counts up to {max(counts)}")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
