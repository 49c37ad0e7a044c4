"""A pure-Python restatement of the text tokenizer (madtp_amd/csrc/madtp_text.h), written from its definitions on the committed
character table: normalise per codepoint, split into words by class, longest-match-first WordPiece with "##", one [UNK] for a word
with an unmatched rest or more than 100 characters.  No library call; the tests compare it with the yardstick and with the kernel."""
import os
import re

import numpy as np

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "madtp_amd", "data", "bert_chars.txt")
OTHER, SPACE, PUNCT, SPACED = 0, 1, 2, 3
HEADER, PAGE_WORDS = 16, 0x1100
MAX_BYTES, MAX_TOKENS, MAX_WORD = 2048, 512, 100
E_LONG, E_UTF8, E_SPECIAL, E_CHAR, E_TOKENS = -401, -402, -403, -404, -405


class Refused(ValueError):
    def __init__(self, code):
        super().__init__(code)
        self.code = code


def read_table(path):
    """the table file's four sections as one list of words: hexadecimal, `v*n` a repeat, `v+d*n` / `v-d*n` a progression"""
    words = []
    with open(path, encoding="ascii") as f:
        sections = dict(line.rstrip("\n").split(" ", 1) for line in f if not line.startswith("#"))
    for name in ("header", "index", "pages", "pool"):
        for tok in sections[name].split():
            m = re.fullmatch(r"([0-9a-f]+)(?:([+-])([0-9a-f]+))?(?:\*([0-9a-f]+))?", tok)
            v, d = int(m.group(1), 16), int(m.group(3) or "0", 16) * (-1 if m.group(2) == "-" else 1)
            words += [v + d * k for k in range(int(m.group(4) or "1", 16))]
    return words


class CharTable:
    def __init__(self, path=TABLE):
        self.words = np.array(read_table(path), dtype=np.int64)
        self.pages, self.pool_words = int(self.words[1]), int(self.words[2])
        self.page0 = HEADER + PAGE_WORDS
        self.pool0 = self.page0 + 256 * self.pages

    def outputs(self, cp):
        """-> [(codepoint, class)] or None for REFUSE"""
        e = int(self.words[self.page0 + 256 * int(self.words[HEADER + (cp >> 8)]) + (cp & 255)])
        kind, value = (e >> 24) & 7, e & 0x1FFFFF
        if kind == 7:
            return None
        if kind == 0:
            return []
        if kind == 1:
            return [((cp + value) & 0x1FFFFF, (e >> 21) & 3)]
        return [(int(w) & 0x1FFFFF, (int(w) >> 21) & 3) for w in self.words[self.pool0 + value:self.pool0 + value + kind]]

    def normalize(self, text):
        """-> [(codepoint, class)] of the whole text; Refused(E_CHAR)"""
        out = []
        for ch in text:
            o = self.outputs(ord(ch))
            if o is None:
                raise Refused(E_CHAR)
            out.extend(o)
        return out

    def normalize_str(self, text):
        """the normalised string as the yardstick's normalize_str gives it: a SPACED codepoint stands for ' c '"""
        return "".join(" " + chr(c) + " " if k == SPACED else chr(c) for c, k in self.normalize(text))


def words_of(chars):
    """[(codepoint, class)] -> the words, each a str"""
    words, cur = [], []
    for c, k in chars:
        if k == OTHER:
            cur.append(chr(c))
            continue
        if cur:
            words.append("".join(cur))
            cur = []
        if k in (PUNCT, SPACED):
            words.append(chr(c))
    if cur:
        words.append("".join(cur))
    return words


def wordpiece(word, ids, unk):
    if len(word) > MAX_WORD:
        return [unk]
    out, start = [], 0
    while start < len(word):
        end = len(word)
        while end > start:
            piece = ("##" if start else "") + word[start:end]
            if piece in ids:
                break
            end -= 1
        if end == start:
            return [unk]
        out.append(ids[piece])
        start = end
    return out


class Tokenizer:
    def __init__(self, entries, specials=("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")):
        self.table = CharTable()
        self.ids = {e: i for i, e in enumerate(entries)}
        self.pad, self.unk, self.cls, self.sep = (self.ids[s] for s in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"))
        self.specials = [s.encode() for s in specials if s in self.ids]

    def tokens(self, raw):
        """UTF-8 bytes -> the ids between [CLS] and [SEP]; Refused(code) with the kernel's precedence"""
        if len(raw) > MAX_BYTES:
            raise Refused(E_LONG)
        try:
            text = raw.decode("utf-8")  # strict: refuses overlong forms, surrogates and values above U+10FFFF
        except UnicodeDecodeError:
            raise Refused(E_UTF8) from None
        if any(s in raw for s in self.specials):
            raise Refused(E_SPECIAL)
        out = []
        for w in words_of(self.table.normalize(text)):
            out.extend(wordpiece(w, self.ids, self.unk))
        return out

    def encode(self, raws, width, max_tokens, truncate):
        """-> (ids [B, width], mask [B, width], status [B, 2]) int64 lists as the kernel writes them; a refused row is None"""
        ids, mask, status = [], [], []
        for raw in raws:
            try:
                t = self.tokens(raw)
                if len(t) + 2 > max_tokens and not truncate:
                    status.append((E_TOKENS, len(t) + 2))
                    raise Refused(E_TOKENS)
            except Refused as r:
                if r.code != E_TOKENS:
                    status.append((r.code, 0))
                ids.append(None)
                mask.append(None)
                continue
            row = [self.cls] + t[:max_tokens - 2] + [self.sep]
            status.append((0, len(t) + 2))
            mask.append([1] * len(row) + [0] * (width - len(row)))
            ids.append(row + [self.pad] * (width - len(row)))
        return ids, mask, status
