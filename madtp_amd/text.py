"""Text input on the device (csrc/madtp_text.h, csrc/text.hip): a BERT WordPiece tokenizer whose ids are those of the installed
`transformers.BertTokenizer` (tokenizers 0.22.2: BertNormalizer(lowercase, strip accents, clean text, spaced CJK), BertPreTokenizer,
WordPiece with "[UNK]", "##" and 100 characters per word).  Opt-in, next to jpeg.py / png.py:

    model.tokenizer = text.blip_tokenizer("bert-base-uncased/vocab.txt", "cuda")     # the reference's init_tokenizer()
    loss = model(image, ["a sentence", ...], targets)                               # the drivers' line stays as it is

    tok = text.WordPiece(vocab, "cuda")                   # a vocab.txt path or a list of entries; tables built and uploaded once
    t = tok(texts, padding='longest', truncation=True, max_length=35, return_tensors="pt")
    t.input_ids, t.attention_mask, t["input_ids"]         # int64 [B, width] on the device; t.to(device) is t

The host only packs bytes: it encodes the strings, joins them behind an offsets array in one pinned staging buffer, copies that once
and launches one kernel (one workgroup per text); the call then waits for the two status words per text, on a side stream behind an
event.  A text the kernel refuses raises ValueError naming the text and the code: malformed UTF-8, more than MAX_BYTES bytes, more
than 512 tokens without truncation, a codepoint whose normalisation depends on its neighbours (83 of them: kept marks that NFD
reorders), or the literal of a special token ("[SEP]", "[DEC]", ...) inside the text - the yardstick matches those before it
normalises, this tokenizer does not.  Device tensors only: without a GPU WordPiece raises, there is no fallback (Tables.encode_host
runs the kernel's lane routines on the host for checking).  Not here: token_type_ids, cased models, CLIP's BPE."""
import os
import threading

import numpy as np
import torch

from . import abi, hip, staging

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "madtp_text.h")
CHARTABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "bert_chars.txt")
# the one declaration of the madtp_text_* entry points, next to the sources; lib() is hip.load()'s handle with them set on it
SIGNATURES, DEFINES, lib = abi.bind(HEADER, "madtp_text_abi_version", prefix="madtp_text_")
ABI_VERSION = DEFINES["MADTP_TEXT_ABI_VERSION"]
MAX_BYTES, MAX_TOKENS, MAX_BATCH = (DEFINES["MADTP_TEXT_" + k] for k in ("MAX_BYTES", "MAX_TOKENS", "MAX_BATCH"))
MAX_WORD_CHARS, TRUNCATE = DEFINES["MADTP_TEXT_MAX_WORD_CHARS"], DEFINES["MADTP_TEXT_TRUNCATE"]
E = {k[len("MADTP_TEXT_E_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_TEXT_E_")}
_V = {k[len("MADTP_TEXT_V_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_TEXT_V_")}
BERT_SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]")

_chartable_lock = threading.Lock()
_chartable = []


def strerror(code):
    return lib().madtp_text_strerror(int(code)).decode()


def _unfold(text):
    """a section of bert_chars.txt -> its words: hexadecimal, `v*n` is v n times, `v+d*n` / `v-d*n` n words from v in steps of d"""
    out = []
    for tok in text.split():
        head, _, run = tok.partition("*")
        sign = "+" if "+" in head else "-" if "-" in head else ""
        v, _, d = head.partition(sign) if sign else (head, "", "0")
        v, d, run = int(v, 16), int(d, 16) * (-1 if sign == "-" else 1), int(run, 16) if run else 1
        out.extend(v + d * k for k in range(run))
    return out


def read_chartable(path=CHARTABLE):
    """bert_chars.txt (tools/make_bert_chartable.py) -> dict: `table` (the uint32 blob of madtp_text.h: header, index, pages, pool),
    `tokenizers_version`, `refused`, `max_expand`"""
    fields = {}
    with open(path, encoding="ascii") as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                name, _, rest = line.partition(" ")
                fields[name] = rest.strip()
    table = np.array([w for k in ("header", "index", "pages", "pool") for w in _unfold(fields[k])], dtype=np.uint32)
    return {"table": table, "tokenizers_version": fields["tokenizers_version"], "refused": int(fields["refused"]),
            "max_expand": [int(v) for v in fields["max_expand"].split()]}


def chartable():
    """the committed character table as one uint32 array (madtp_text.h, MADTP_TEXT_CT_*), checked by the library once per process"""
    with _chartable_lock:
        if not _chartable:
            table = read_chartable()["table"]
            rc = lib().madtp_text_chartable_check(table.ctypes.data, table.size)
            if rc:
                raise RuntimeError(f"{CHARTABLE}: {strerror(rc)} (code {rc})")
            _chartable.append(table)
        return _chartable[0]


def read_vocab(path):
    """a vocab.txt -> its entries, one per line, as transformers' load_vocab reads them"""
    with open(path, encoding="utf-8") as f:
        return [line.rstrip("\n") for line in f]


def build_vocab(entries, specials=()):
    """entries (str), the ids of further special tokens -> the vocabulary table, one uint32 array (madtp_text_vocab_build).  Host
    only.  ValueError names what the builder refuses: a duplicate, an empty entry, a missing [PAD] / [UNK] / [CLS] / [SEP]."""
    raw = [e.encode("utf-8") for e in entries]
    if not raw:
        raise ValueError("vocabulary: no entries")
    blob = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    sp = np.asarray(list(specials), dtype=np.int32)
    h = lib()
    nbytes = h.madtp_text_vocab_bytes(blob.ctypes.data, off.ctypes.data, len(raw), sp.size)
    if nbytes < 0:
        raise ValueError(f"vocabulary: {strerror(nbytes)} (code {nbytes})")
    out = np.zeros(nbytes // 4, dtype=np.uint32)
    rc = h.madtp_text_vocab_build(blob.ctypes.data, off.ctypes.data, len(raw), sp.ctypes.data if sp.size else None, sp.size,
                                  out.ctypes.data, out.nbytes)
    if rc:
        raise ValueError(f"vocabulary: {strerror(rc)} (code {rc})")
    return out[:int(out[_V["WORDS"]])].copy()


def _pack(texts):
    """-> (the texts' UTF-8 bytes back to back, int64 offsets [B + 1])"""
    if isinstance(texts, str):
        texts = [texts]
    texts = list(texts)
    if not 1 <= len(texts) <= MAX_BATCH:
        raise ValueError(f"a batch of {len(texts)} texts, outside [1, {MAX_BATCH}]")
    try:
        raw = [t if isinstance(t, bytes) else t.encode("utf-8") for t in texts]
    except (UnicodeEncodeError, AttributeError) as e:
        raise ValueError(f"texts must be str (or UTF-8 bytes): {e}") from e
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return texts, b"".join(raw), off


def _plan(padding, truncation, max_length):
    """the keyword sets of the reference's drivers -> (width of the kernel's rows, max_tokens, flags)"""
    if padding is True:
        padding = 'longest'
    if padding not in (False, None, 'longest', 'max_length'):
        raise ValueError(f"padding={padding!r} is not 'longest', 'max_length' or False")
    if truncation not in (True, False):
        raise ValueError(f"truncation={truncation!r} is not True or False")
    if max_length is not None and not 2 <= int(max_length) <= MAX_TOKENS:
        raise ValueError(f"max_length={max_length} outside [2, {MAX_TOKENS}]")
    if truncation and max_length is None:
        raise ValueError("truncation=True needs max_length")
    if padding == 'max_length' and max_length is None:
        raise ValueError("padding='max_length' needs max_length")
    if truncation:
        return int(max_length), int(max_length), TRUNCATE
    return MAX_TOKENS, MAX_TOKENS, 0


def _width(padding, max_length, counts, max_tokens):
    """the width of the returned tensors from the texts' token counts: never more than the kernel's rows (max_length <= max_tokens)"""
    kept = np.minimum(counts, max_tokens)
    if padding == 'max_length':
        return max(int(max_length), int(kept.max()))
    if padding in (False, None) and int(kept.min()) != int(kept.max()):
        raise ValueError(f"texts of {int(kept.min())} to {int(kept.max())} tokens and no padding: they do not make a tensor")
    return int(kept.max())


class Encoding(dict):
    """what a call returns: .input_ids / .attention_mask and ["input_ids"] / ["attention_mask"], int64 [B, width]"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def to(self, device=None, **kw):
        return self


class Tables:
    """The host side: the entries, the two tables, the special ids and decode().  No GPU state."""

    def __init__(self, vocab, extra_specials=(), lowercase=True):
        if not lowercase:
            raise ValueError("lowercase=False: cased models are out of scope (the character table records the uncased normaliser)")
        self.entries = read_vocab(vocab) if isinstance(vocab, (str, os.PathLike)) else list(vocab)
        self.ids = {e: i for i, e in enumerate(self.entries)}
        missing = [s for s in extra_specials if s not in self.ids]
        if missing:
            raise ValueError(f"vocabulary: special tokens {missing} are not entries")
        self.special_ids = [self.ids[s] for s in BERT_SPECIALS if s in self.ids] + [self.ids[s] for s in extra_specials]
        self.vocab = build_vocab(self.entries, self.special_ids)
        self.chartable = chartable()
        for name in ("pad", "unk", "cls", "sep"):
            setattr(self, name + "_token_id", int(self.vocab[_V[name.upper()]]))
        self.mask_token_id = self.ids.get("[MASK]")
        self.vocab_size = len(self.entries)

    def __len__(self):
        return len(self.entries)

    def encode_host(self, texts, width=MAX_TOKENS, max_tokens=None, truncate=False, canary=-7):
        """madtp_text_encode_host -> (ids int64 [B, width], mask int64 [B, width], status int32 [B, 2]) numpy; a text with a code
        leaves its row at `canary`"""
        _, raw, off = _pack(texts)
        B = off.size - 1
        data = np.frombuffer(raw + b"\0", dtype=np.uint8)
        ids = np.full((B, width), canary, dtype=np.int64)
        mask = np.full((B, width), canary, dtype=np.int64)
        status = np.full((B, 2), canary, dtype=np.int32)
        hip._check(lib().madtp_text_encode_host(data.ctypes.data, off.ctypes.data, self.chartable.ctypes.data, self.vocab.ctypes.data,
                                                ids.ctypes.data, mask.ctypes.data, status.ctypes.data, B, int(width),
                                                int(width if max_tokens is None else max_tokens), TRUNCATE if truncate else 0),
                   "madtp_text_encode_host")
        return ids, mask, status

    def call_host(self, texts, padding=False, truncation=False, max_length=None):
        """the host emulation behind the keyword sets of __call__ -> (ids, mask) numpy; ValueError as __call__ raises it"""
        texts, _, _ = _pack(texts)
        width, max_tokens, flags = _plan(padding, truncation, max_length)
        ids, mask, status = self.encode_host(texts, width, max_tokens, bool(flags))
        _raise_status(texts, status)
        w = _width(padding, max_length, status[:, 1], max_tokens)
        return ids[:, :w], mask[:, :w]

    def convert_ids_to_tokens(self, ids):
        return [self.entries[int(i)] for i in ids]

    def decode(self, ids, skip_special_tokens=False, clean_up_tokenization_spaces=False):
        """ids (a tensor, an array or a list) -> the string of transformers' decode: pieces joined by spaces, "##" pieces glued on,
        the WordPiece decoder's clean-up of spaces before punctuation and contractions.  On the host."""
        ids = ids.tolist() if hasattr(ids, "tolist") else list(ids)
        special = set(self.special_ids) if skip_special_tokens else ()
        out = []
        for i in ids:
            if i in special:
                continue
            tok = self.entries[int(i)]
            if out:
                tok = tok[2:] if tok.startswith("##") else " " + tok
            out.append(_cleanup(tok, True))
        s = "".join(out)
        return _cleanup(s, False) if clean_up_tokenization_spaces else s

    def batch_decode(self, batch, **kw):
        return [self.decode(ids, **kw) for ids in batch]


def _cleanup(s, piece):
    """the WordPiece decoder's per-piece clean-up (piece=True), transformers' clean_up_tokenization of the whole string (False)"""
    s = s.replace(" .", ".").replace(" ?", "?").replace(" !", "!").replace(" ,", ",").replace(" ' ", "'").replace(" n't", "n't").replace(" 'm", "'m")
    if piece:
        s = s.replace(" do not", " don't")
    return s.replace(" 's", "'s").replace(" 've", "'ve").replace(" 're", "'re")


def _raise_status(texts, status):
    for b, (code, _) in enumerate(status):
        if code:
            t = texts[b]
            shown = t[:40] if isinstance(t, (str, bytes)) else t
            raise ValueError(f"text {b} ({shown!r}{'...' if len(t) > 40 else ''}): {strerror(code)} (code {int(code)})")


_waiter = staging.StatusWaiter()


class WordPiece:
    """The tokenizer on a device.  vocab: a vocab.txt path or a list of entries; extra_specials: entries beyond BERT's five that
    are special tokens.  Has the attributes and methods the models use of a BertTokenizer: __call__, decode, *_token_id."""

    def __init__(self, vocab, device, lowercase=True, extra_specials=()):
        self.tables = vocab if isinstance(vocab, Tables) else Tables(vocab, extra_specials, lowercase)
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"WordPiece runs on a GPU (device={device!r}): device tensors only, there is no fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self._chartable = torch.from_numpy(self.tables.chartable).pin_memory().to(self.device, non_blocking=True)
            self._vocab = torch.from_numpy(self.tables.vocab).pin_memory().to(self.device, non_blocking=True)
        self._ring = staging.StagingRing()
        self._lock = threading.Lock()
        for name in ("pad", "unk", "cls", "sep", "mask"):
            setattr(self, name + "_token_id", getattr(self.tables, name + "_token_id"))
        self.vocab_size = self.tables.vocab_size

    def __len__(self):
        return len(self.tables)

    def encode_raw(self, texts, width=MAX_TOKENS, max_tokens=None, truncate=False, fill=None):
        """One copy and one launch, no wait -> (ids int64 [B, width], mask int64 [B, width], status int32 [B, 2]) on the device.  A
        text with a code in status[:, 0] leaves its row unwritten (at `fill` where one is given)."""
        _, raw, off = _pack(texts)
        B, head = off.size - 1, off.nbytes
        with self._lock, torch.cuda.device(self.device):
            turn, stage = self._ring.acquire(head + len(raw))
            view = stage.numpy()
            view[:head] = off.view(np.uint8)
            view[head:head + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
            packed = torch.empty(head + max(len(raw), 1), dtype=torch.uint8, device=self.device)
            packed[:head + len(raw)].copy_(stage[:head + len(raw)], non_blocking=True)
            self._ring.sent(turn)
            make = torch.empty if fill is None else (lambda *shape, **kw: torch.full(shape, fill, **kw))
            ids = make(B, width, dtype=torch.int64, device=self.device)
            mask = make(B, width, dtype=torch.int64, device=self.device)
            status = torch.empty(B, 2, dtype=torch.int32, device=self.device)
            hip._check(lib().madtp_text_encode_batch(packed.data_ptr() + head, packed.data_ptr(), self._chartable.data_ptr(),
                                                     self._vocab.data_ptr(), ids.data_ptr(), mask.data_ptr(), status.data_ptr(), B,
                                                     int(width), int(width if max_tokens is None else max_tokens),
                                                     TRUNCATE if truncate else 0, hip._stream()), "madtp_text_encode_batch")
            packed.record_stream(torch.cuda.current_stream(self.device))
        return ids, mask, status

    def __call__(self, texts, padding=False, truncation=False, max_length=None, return_tensors="pt"):
        """The keyword sets of the reference's drivers -> Encoding.  'longest' takes its width from the status words and returns a
        view of the kernel's rows.  ValueError names the first text the kernel refuses."""
        if return_tensors != "pt":
            raise ValueError(f"return_tensors={return_tensors!r}: only 'pt' (device tensors)")
        texts, _, _ = _pack(texts)
        width, max_tokens, flags = _plan(padding, truncation, max_length)
        ids, mask, status = self.encode_raw(texts, width, max_tokens, bool(flags))
        words = _waiter.read(status.view(-1)).reshape(-1, 2)
        _raise_status(texts, words)
        w = _width(padding, max_length, words[:, 1], max_tokens)
        return Encoding(input_ids=ids[:, :w], attention_mask=mask[:, :w])

    def decode(self, ids, skip_special_tokens=False, clean_up_tokenization_spaces=False):
        return self.tables.decode(ids, skip_special_tokens, clean_up_tokenization_spaces)

    def batch_decode(self, batch, **kw):
        return self.tables.batch_decode(batch, **kw)

    def convert_ids_to_tokens(self, ids):
        return self.tables.convert_ids_to_tokens(ids)


BLIP_SPECIALS = ("[DEC]", "[ENC]")


def blip_entries(vocab):
    """a vocab.txt path or a list of entries -> the entries with the reference's init_tokenizer() additions: "[DEC]" (the bos token)
    and "[ENC]" appended, ids len(vocab) and len(vocab) + 1 (30522 and 30523 with bert-base-uncased's file)"""
    entries = read_vocab(vocab) if isinstance(vocab, (str, os.PathLike)) else list(vocab)
    return entries + [s for s in BLIP_SPECIALS if s not in entries]


def blip_tokenizer(vocab, device):
    """the reference's init_tokenizer() (models/blip.py): BertTokenizer + bos_token "[DEC]" + additional special token "[ENC]"."""
    tok = WordPiece(blip_entries(vocab), device, extra_specials=BLIP_SPECIALS)
    tok.bos_token_id = tok.tables.ids["[DEC]"]
    tok.enc_token_id = tok.tables.ids["[ENC]"]
    tok.additional_special_tokens_ids = [tok.enc_token_id]
    return tok
