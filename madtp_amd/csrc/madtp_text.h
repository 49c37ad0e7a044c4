/* madtp_text.h - text input: a batch of UTF-8 strings to BERT WordPiece input_ids / attention_mask on the device (csrc/text.hip,
 * linked into libmadtp_hip.so; the lane routines of csrc/text_device.h, which the host emulation below runs as well).  The ids are
 * those of BertNormalizer(clean_text, handle_chinese_chars, strip_accents=None, lowercase=True) + BertPreTokenizer +
 * WordPiece(unk "[UNK]", prefix "##", max_input_chars_per_word 100) of tokenizers 0.22.2.
 *
 * Two tables, both one blob of uint32 words made on the host and uploaded once:
 *   the CHARACTER table (madtp_amd/data/bert_chars.txt, tools/make_bert_chartable.py): what the yardstick's normaliser and
 *   pre-tokeniser do with every codepoint, recorded: 0 .. 3 output codepoints and a class for each;
 *   the VOCABULARY table (madtp_text_vocab_build): the pieces' codepoints in a pool, an open-addressing hash table over whole
 *   pieces ("##ab" and "ab" are different keys) and the literals of the special tokens.
 *
 * Conventions of madtp_hip.h: plain pointers and sizes, nothing allocates, frees or synchronises, launches go to `stream` (a
 * hipStream_t passed as void*); 0 on success, a negative code on a rejected argument before any launch, a positive hipError_t if the
 * runtime refuses a launch.  No atomics and no workgroup that waits for another; nothing a lane stored to global memory is read
 * back: identical calls give identical bits.  Every read of a text is checked against its extent, every write against the row,
 * every table index against the table's own sizes, and every loop is bounded by a count known at launch or by the text's bytes.
 * This header has its own version number; the other headers do not change with it.  It lives next to the sources that implement
 * it: the file list of include/ is pinned by a test of the candidate lists. */
#ifndef MADTP_TEXT_H
#define MADTP_TEXT_H

#include "../../include/madtp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MADTP_TEXT_ABI_VERSION 1
int madtp_text_abi_version(void);

#define MADTP_TEXT_MAX_BYTES 2048      /* UTF-8 bytes of one text                                                               */
#define MADTP_TEXT_MAX_TOKENS 512      /* tokens of one text, [CLS] and [SEP] included; and the widest row                      */
#define MADTP_TEXT_MAX_WORD_CHARS 100  /* a longer word is one [UNK]                                                            */
#define MADTP_TEXT_MAX_BATCH 65535
#define MADTP_TEXT_MAX_VOCAB 1048576   /* entries                                                                               */
#define MADTP_TEXT_MAX_PIECE_CHARS 256 /* codepoints of one entry, "##" included                                                */
#define MADTP_TEXT_MAX_SPECIALS 16     /* special tokens whose literal a text must not contain                                  */
#define MADTP_TEXT_MAX_SPECIAL_BYTES 32
#define MADTP_TEXT_LANES 256           /* of the workgroup that owns a text                                                     */

/* ---- codes: of a text (the first status word), or of a vocabulary / a table the builder and the checker refuse ----------------- */
#define MADTP_TEXT_E_LONG (-401)     /* more than MAX_BYTES bytes, or offsets that run backwards                                  */
#define MADTP_TEXT_E_UTF8 (-402)     /* a malformed sequence, an overlong form, a surrogate or a value above U+10FFFF            */
#define MADTP_TEXT_E_SPECIAL (-403)  /* the raw bytes contain the literal of a special token ("[SEP]", "[DEC]", ...)              */
#define MADTP_TEXT_E_CHAR (-404)     /* a codepoint whose normalisation depends on its neighbours (REFUSE in the table)           */
#define MADTP_TEXT_E_TOKENS (-405)   /* more tokens than max_tokens and MADTP_TEXT_TRUNCATE not set                               */
#define MADTP_TEXT_E_VOCAB_DUP (-411)     /* an entry occurs twice                                                                */
#define MADTP_TEXT_E_VOCAB_EMPTY (-412)   /* an empty entry                                                                       */
#define MADTP_TEXT_E_VOCAB_MISSING (-413) /* no [PAD], [UNK], [CLS] or [SEP]                                                      */
#define MADTP_TEXT_E_VOCAB_ENTRY (-414)   /* an entry that is not UTF-8 or longer than MAX_PIECE_CHARS, a special out of range    */
#define MADTP_TEXT_E_TABLE (-415)         /* a table blob whose header, sizes or indices do not fit together                      */
const char* madtp_text_strerror(int code);
/* a text with several faults reports the first of: E_LONG, E_UTF8, E_SPECIAL, E_CHAR, E_TOKENS */

/* ---- the character table ---------------------------------------------------------------------------------------------------------
 * words[0 .. CT_HEADER): MAGIC, pages, pool words, the largest number of output codepoints of a 1 / 2 / 3 / 4-byte codepoint, the
 * blob's words; then 0x1100 page numbers (codepoint >> 8), the pages of 256 entries, the pool.  An entry: bits 0 .. 20 a value,
 * 21 .. 22 a class, 24 .. 26 the kind: 0 removed, 1 one output codepoint (input + value mod 2^21, of the class), 2 / 3 that many
 * pool words from value on (each codepoint | class << 21), 7 REFUSE.  A SPACED codepoint stands for " c ": a word of its own. */
#define MADTP_TEXT_CT_MAGIC 1413698626
#define MADTP_TEXT_CT_HEADER 16
#define MADTP_TEXT_CT_PAGES 1
#define MADTP_TEXT_CT_POOL 2
#define MADTP_TEXT_CT_EXPAND 3
#define MADTP_TEXT_CT_WORDS 7
#define MADTP_TEXT_CLASS_OTHER 0
#define MADTP_TEXT_CLASS_SPACE 1
#define MADTP_TEXT_CLASS_PUNCT 2
#define MADTP_TEXT_CLASS_SPACED 3
/* host: 0 if the blob of `words` words is consistent (every page number, pool index and output codepoint in range) and no
 * codepoint expands to more codepoints than it has UTF-8 bytes - which is what sizes the kernel's LDS arrays; else E_TABLE */
int madtp_text_chartable_check(const uint32_t* table, int64_t words);

/* ---- the vocabulary table ----------------------------------------------------------------------------------------------------------
 * entries: the UTF-8 bytes of the n entries back to back, entry i at [entry_offsets[i], entry_offsets[i + 1]) (id = i).  specials:
 * n_special ids whose literals a text must not contain ([PAD] [UNK] [CLS] [SEP] are always among them, whether listed or not).
 * Host only, no GPU state, no allocation: _bytes says how large the blob is, _build fills it (MADTP_E_BADARG if out_bytes is less).
 * words[0 .. V_HEADER): MAGIC, entries, pool words, hash slots (a power of two, at least twice the entries), the longest entry in
 * codepoints, the ids of [PAD] [UNK] [CLS] [SEP], specials, the word offsets of the entry starts (n + 1), the pool, the hash table
 * (slots of 2 words: id + 1 or 0, the high half of the key's hash) and the specials (MAX_SPECIAL_BYTES + 2 words each: length,
 * id, bytes), the blob's words. */
#define MADTP_TEXT_V_MAGIC 1448363074
#define MADTP_TEXT_V_HEADER 16
#define MADTP_TEXT_V_ENTRIES 1
#define MADTP_TEXT_V_POOL 2
#define MADTP_TEXT_V_SLOTS 3
#define MADTP_TEXT_V_LONGEST 4
#define MADTP_TEXT_V_PAD 5
#define MADTP_TEXT_V_UNK 6
#define MADTP_TEXT_V_CLS 7
#define MADTP_TEXT_V_SEP 8
#define MADTP_TEXT_V_SPECIALS 9
#define MADTP_TEXT_V_OFF_STARTS 10
#define MADTP_TEXT_V_OFF_POOL 11
#define MADTP_TEXT_V_OFF_HASH 12
#define MADTP_TEXT_V_OFF_SPECIALS 13
#define MADTP_TEXT_V_WORDS 14
int64_t madtp_text_vocab_bytes(const void* entries, const int64_t* entry_offsets, int n, int n_special);
int madtp_text_vocab_build(const void* entries, const int64_t* entry_offsets, int n, const int32_t* specials, int n_special, void* out,
                           int64_t out_bytes);

/* ---- encode ------------------------------------------------------------------------------------------------------------------------
 * bytes: the texts back to back, text b at [offsets[b], offsets[b + 1]) (int64 [B + 1]); chartable, vocab: the blobs above;
 * ids_out, mask_out: int64 [B, width]; status: int32 [B, 2]: a code or 0, and the text's token count before truncation with [CLS]
 * and [SEP] (0 when a code came before it was known).  A text without a code gets [CLS], its first max_tokens - 2 ids, [SEP] and
 * [PAD] up to width, the mask 1 up to [SEP]; a text with a code leaves its row unwritten.  2 <= max_tokens <= width <=
 * MAX_TOKENS.  flags: MADTP_TEXT_TRUNCATE or 0 (more tokens than max_tokens is then E_TOKENS).  One workgroup owns one text.
 * All pointers are device memory.  MADTP_E_BADARG: a null pointer or a size outside these ranges. */
#define MADTP_TEXT_TRUNCATE 1
int madtp_text_encode_batch(const void* bytes, const int64_t* offsets, const uint32_t* chartable, const uint32_t* vocab, int64_t* ids_out,
                            int64_t* mask_out, int32_t* status, int B, int width, int max_tokens, int flags, void* stream);

/* the same text with the lanes (and the workgroups) in `for` loops; every pointer is host memory; no GPU call.  For checking. */
int madtp_text_encode_host(const void* bytes, const int64_t* offsets, const uint32_t* chartable, const uint32_t* vocab, int64_t* ids_out,
                           int64_t* mask_out, int32_t* status, int B, int width, int max_tokens, int flags);

#ifdef __cplusplus
}
#endif
#endif /* MADTP_TEXT_H */
