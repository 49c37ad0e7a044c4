"""Records what the installed tokenizers' BertNormalizer and BertPreTokenizer do with every codepoint -> madtp_amd/data/bert_chars.txt.

    python tools/make_bert_chartable.py [--check]      # --check: compare a fresh generation with the committed file, write nothing

The table is the yardstick's behaviour, recorded - not a restatement of Unicode rules.  Per codepoint 0 .. 0x10FFFF (no surrogates):
  - normalizer.normalize_str(chr(cp)): 0 to 3 output codepoints;
  - the class of every output codepoint, read from pre_tokenizer.pre_tokenize_str("a" + c + "a"): OTHER (one word), SPACE (two
    words), PUNCT (three words: the character is a word of its own);
  - an output of the form " c " (what handle_chinese_chars makes of a CJK character) is stored as the ONE codepoint c of class
    SPACED: a word of its own like PUNCT, and three characters of the normalised string;
  - REFUSE: a codepoint that the normaliser moves past a neighbour (a kept mark with a combining class: NFD reorders it), found
    with two probes of different class, one in front and one behind.  Per-codepoint composition does not hold for these.

Layout (csrc/madtp_text.h, MADTP_TEXT_CT_*): one uint32 blob = header, page index (one word per 256 codepoints), pages of 256 entries
(identical pages shared; a single output is stored as its distance from the input, so identity pages are one page), and the pool of
the multi-codepoint outputs.

The file is text, so that it can live next to the code that reads it: comment lines, then one line per field - `tokenizers_version`,
`refused`, `max_expand`, and the blob's four sections `header`, `index`, `pages`, `pool` as hexadecimal words with runs folded:
`v*n` is v n times, `v+d*n` / `v-d*n` is n words from v in steps of d (madtp_amd/text.py read_chartable is the reader)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "madtp_amd", "data", "bert_chars.txt")

MAGIC = 0x54435442  # "BTCT"
HEADER_WORDS = 16
OTHER, SPACE, PUNCT, SPACED = 0, 1, 2, 3
KIND_REMOVED, KIND_ONE, KIND_REFUSE = 0, 1, 7  # 2, 3: that many pool words
CP_MASK, CLASS_SHIFT, KIND_SHIFT = 0x1FFFFF, 21, 24
PROBE_BEHIND, PROBE_FRONT = "\U0001d165", "〮"  # two kept marks of different combining class (216, 224)


def utf8_len(cp):
    return 1 if cp < 0x80 else 2 if cp < 0x800 else 3 if cp < 0x10000 else 4


def generate():
    import tokenizers
    from tokenizers import normalizers, pre_tokenizers
    norm = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True)
    pre = pre_tokenizers.BertPreTokenizer()
    classes = {}

    def klass(c):
        return classes[c]

    def classify(chars):
        """the classes of many characters from one call: "a" + c + "a" groups four characters apart, the words counted by offset"""
        chars = [c for c in chars if c not in classes]
        count = [0] * len(chars)
        for _, (start, _) in pre.pre_tokenize_str(" ".join("a" + c + "a" for c in chars)):
            count[start // 4] += 1
        for c, n in zip(chars, count):
            classes[c] = {1: OTHER, 2: SPACE, 3: PUNCT}[n]

    behind, front = norm.normalize_str(PROBE_BEHIND), norm.normalize_str(PROBE_FRONT)
    assert behind == PROBE_BEHIND and front == PROBE_FRONT, "the probes are not kept as they are"
    entries = np.zeros(0x110000, dtype=np.uint32)
    pool, pool_at = [], {}
    max_expand = [0, 0, 0, 0, 0]
    refused = 0
    outs = [None if 0xD800 <= cp < 0xE000 else norm.normalize_str(chr(cp)) for cp in range(0x110000)]
    for p in range(0x1100):
        classify(sorted({c for cp in range(p * 256, p * 256 + 256) if outs[cp] for c in outs[cp]}))
    for c in "a ,":  # the three classes, one character at a time, as the batches must have them
        assert klass(c) == {1: OTHER, 2: SPACE, 3: PUNCT}[len(pre.pre_tokenize_str("a" + c + "a"))]
    # the probes, a page of codepoints per call: every codepoint between the probe in front and the one behind, with a starter ("a",
    # which no mark moves past) between the two and behind the pair.  A page that is not the concatenation of what composition
    # promises is probed again one codepoint at a time.
    moved = set()
    for p in range(0x1100):
        cps = [cp for cp in range(p * 256, p * 256 + 256) if outs[cp] is not None]
        got = norm.normalize_str("".join(PROBE_FRONT + chr(cp) + "a" + chr(cp) + PROBE_BEHIND + "a" for cp in cps))
        if got == "".join(front + outs[cp] + "a" + outs[cp] + behind + "a" for cp in cps):
            continue
        for cp in cps:
            ch = chr(cp)
            if norm.normalize_str(ch + PROBE_BEHIND) != outs[cp] + behind or norm.normalize_str(PROBE_FRONT + ch) != front + outs[cp]:
                moved.add(cp)
    for cp in range(0x110000):
        if 0xD800 <= cp < 0xE000:
            entries[cp] = KIND_REFUSE << KIND_SHIFT  # never reached: the decoder refuses a surrogate first
            continue
        out = outs[cp]
        if cp in moved:
            entries[cp] = KIND_REFUSE << KIND_SHIFT
            refused += 1
            continue
        assert len(out) <= 3, (hex(cp), out)
        if len(out) == 3 and out[0] == " " and out[2] == " " and klass(out[1]) == OTHER:
            kind, word = KIND_ONE, ((ord(out[1]) - cp) & CP_MASK) | (SPACED << CLASS_SHIFT)
            expand = 3
        elif len(out) == 0:
            kind, word, expand = KIND_REMOVED, 0, 0
        elif len(out) == 1:
            kind, word, expand = KIND_ONE, ((ord(out) - cp) & CP_MASK) | (klass(out) << CLASS_SHIFT), 1
        else:
            key = tuple(ord(c) | (klass(c) << CLASS_SHIFT) for c in out)
            if key not in pool_at:
                pool_at[key] = len(pool)
                pool.extend(key)
            kind, word, expand = len(out), pool_at[key], len(out)
        entries[cp] = word | (kind << KIND_SHIFT)
        n = utf8_len(cp)
        max_expand[n] = max(max_expand[n], expand)
    pages, page_of, index = [], {}, np.zeros(0x1100, dtype=np.uint32)
    for p in range(0x1100):
        page = entries[p * 256:(p + 1) * 256]
        key = page.tobytes()
        if key not in page_of:
            page_of[key] = len(pages)
            pages.append(page)
        index[p] = page_of[key]
    header = np.zeros(HEADER_WORDS, dtype=np.uint32)
    header[0], header[1], header[2] = MAGIC, len(pages), len(pool)
    header[3:7] = max_expand[1:5]
    header[7] = HEADER_WORDS + 0x1100 + 256 * len(pages) + len(pool)
    blob = np.concatenate([header, index, np.concatenate(pages), np.asarray(pool, dtype=np.uint32)]).astype(np.uint32)
    assert blob.size == header[7]
    return {"table": blob, "tokenizers_version": np.array(tokenizers.__version__), "refused": np.array(refused),
            "max_expand": np.asarray(max_expand[1:], dtype=np.int32)}


def fold(words):
    """words -> the run-folded hexadecimal text of a section"""
    a = [int(w) for w in words]
    out, i, n = [], 0, len(a)
    while i < n:
        j = i + 1
        if j < n:
            d = a[j] - a[i]
            while j + 1 < n and a[j + 1] - a[j] == d:
                j += 1
            if j - i + 1 >= 3:
                step = "" if d == 0 else f"+{d:x}" if d > 0 else f"-{-d:x}"
                out.append(f"{a[i]:x}{step}*{j - i + 1:x}")
                i = j + 1
                continue
        out.append(f"{a[i]:x}")
        i += 1
    return " ".join(out)


def render(fresh):
    """generate()'s result -> the text of bert_chars.txt"""
    t = fresh["table"]
    pages, pool = int(t[1]), int(t[2])
    i0, p0, q0 = HEADER_WORDS, HEADER_WORDS + 0x1100, HEADER_WORDS + 0x1100 + 256 * pages
    lines = ["# What BertNormalizer(clean_text, handle_chinese_chars, strip_accents=None, lowercase=True) and BertPreTokenizer do with every",
             "# codepoint, recorded by tools/make_bert_chartable.py (layout: madtp_amd/csrc/madtp_text.h, MADTP_TEXT_CT_*).  Do not edit.",
             f"tokenizers_version {fresh['tokenizers_version']}", f"refused {int(fresh['refused'])}",
             "max_expand " + " ".join(str(int(v)) for v in fresh["max_expand"]),
             "header " + fold(t[:i0]), "index " + fold(t[i0:p0]), "pages " + fold(t[p0:q0]), "pool " + fold(t[q0:q0 + pool])]
    return "\n".join(lines) + "\n"


def main():
    text = render(generate())
    if "--check" in sys.argv:
        with open(OUT, encoding="ascii") as f:
            same = f.read() == text
        print("identical" if same else "DIFFERENT")
        return 0 if same else 1
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w", encoding="ascii") as f:
        f.write(text)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")
    for line in text.splitlines()[2:5]:
        print(" ", line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
