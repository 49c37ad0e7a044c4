// Text input as both sides run it (csrc/madtp_text.h): the lane routines of the kernel of text.hip, and the host-only table code
// (the vocabulary builder, the character table's checker).  The lane routines are __host__ __device__ text: the kernel runs them
// with one thread per lane, madtp_text_encode_host (and tools/text_host_check.cpp under the host compiler's sanitizers) with the
// lanes of a workgroup, and the workgroups, in `for` loops.
//
// How the 256 lanes of a workgroup work together (as in tokenmap_device.h):
//   - control is UNIFORM: every early return depends only on launch arguments, table headers and LDS words read behind a barrier;
//   - what lanes do side by side is an each_lane() body; a body keeps nothing from one each_lane() to the next except in LDS;
//   - sync_lanes() stands between a write to LDS and a read of it by another lane.
// No allocation, no mutable static, no atomics.  Two lanes write one LDS word only where both store the same value (the flags).
// Nothing a lane stored to global memory is read back.
#pragma once
#include <stdint.h>

#include "madtp_text.h"

#if defined(__HIPCC__)
#define TX_HD __host__ __device__ inline
#else
#define TX_HD inline
#endif

namespace madtp_text {

constexpr int kLanes = MADTP_TEXT_LANES, kMaxBytes = MADTP_TEXT_MAX_BYTES, kMaxTokens = MADTP_TEXT_MAX_TOKENS;
constexpr int kMaxWord = MADTP_TEXT_MAX_WORD_CHARS, kCtHeader = MADTP_TEXT_CT_HEADER, kVHeader = MADTP_TEXT_V_HEADER;
constexpr int kPageWords = 0x1100, kSpecialWords = MADTP_TEXT_MAX_SPECIAL_BYTES + 2;  // length, id, bytes
constexpr uint32_t kCpMask = 0x1FFFFF, kMaxCp = 0x10FFFF;
constexpr int kClassShift = 21, kKindShift = 24, kKindRefuse = 7;
constexpr uint64_t kMul = 0x100000001B3ull, kFold = 0x9E3779B97F4A7C15ull;  // the polynomial's base, and the multiplier that folds a hash into a slot
// a normalised text never has more codepoints than the raw one has bytes (madtp_text_chartable_check), and a word number, a
// position and a word's end fit 16 bits
static_assert(kMaxBytes <= 65535 && kMaxBytes % kLanes == 0, "positions are uint16 in LDS");
static_assert(kMaxTokens <= kMaxBytes, "a token has at least one character");

template <class F>
TX_HD void each_lane(F body) {
#if defined(__HIP_DEVICE_COMPILE__)
    body((int)threadIdx.x);
#else
    for (int lane = 0; lane < kLanes; ++lane) body(lane);
#endif
}

TX_HD void sync_lanes() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

TX_HD bool first_lane() {
#if defined(__HIP_DEVICE_COMPILE__)
    return threadIdx.x == 0;
#else
    return true;
#endif
}

inline const char* strerror_text(int code) {
    switch (code) {
        case MADTP_TEXT_E_LONG: return "the text has more bytes than MADTP_TEXT_MAX_BYTES";
        case MADTP_TEXT_E_UTF8: return "malformed UTF-8 (a broken or overlong sequence, a surrogate or a value above U+10FFFF)";
        case MADTP_TEXT_E_SPECIAL: return "the text contains the literal of a special token";
        case MADTP_TEXT_E_CHAR: return "the text contains a codepoint whose normalisation depends on its neighbours";
        case MADTP_TEXT_E_TOKENS: return "the text has more tokens than max_tokens and truncation is off";
        case MADTP_TEXT_E_VOCAB_DUP: return "the vocabulary has an entry twice";
        case MADTP_TEXT_E_VOCAB_EMPTY: return "the vocabulary has an empty entry";
        case MADTP_TEXT_E_VOCAB_MISSING: return "the vocabulary lacks [PAD], [UNK], [CLS] or [SEP]";
        case MADTP_TEXT_E_VOCAB_ENTRY: return "a vocabulary entry is not UTF-8 or too long, or a special token's id or literal is out of range";
        case MADTP_TEXT_E_TABLE: return "a table blob is inconsistent";
    }
    return nullptr;
}

// ---- UTF-8 -------------------------------------------------------------------------------------------------------------------------------
TX_HD int lead_len(uint8_t c) { return c < 0x80 ? 1 : (c & 0xE0) == 0xC0 ? 2 : (c & 0xF0) == 0xE0 ? 3 : (c & 0xF8) == 0xF0 ? 4 : 0; }

// byte i of the n bytes at t: -> the sequence's length and its codepoint if a well-formed sequence begins there, 0 if the byte is a
// continuation byte that a lead in front of it covers, -1 for anything else.  Reads t[max(i - 3, 0) .. min(i + 4, n)) only.
TX_HD int decode_at(const uint8_t* t, int n, int i, uint32_t* cp) {
    const uint8_t c = t[i];
    if ((c & 0xC0) == 0x80) {
        for (int j = i - 1; j >= 0 && j >= i - 3; --j)
            if ((t[j] & 0xC0) != 0x80) return lead_len(t[j]) > i - j ? 0 : -1;
        return -1;
    }
    const int len = lead_len(c);
    if (len == 0 || i + len > n) return -1;
    uint32_t v = len == 1 ? c : c & (0x7Fu >> len);
    for (int k = 1; k < len; ++k) {
        if ((t[i + k] & 0xC0) != 0x80) return -1;
        v = (v << 6) | (t[i + k] & 0x3Fu);
    }
    if ((len == 2 && v < 0x80) || (len == 3 && v < 0x800) || (len == 4 && v < 0x10000) || v > kMaxCp || (v >= 0xD800 && v < 0xE000)) return -1;
    *cp = v;
    return len;
}

// ---- the character table ---------------------------------------------------------------------------------------------------------------
// -> the entry of cp <= 0x10FFFF; REFUSE for an index the header does not cover
TX_HD uint32_t ct_entry(const uint32_t* ct, uint32_t cp) {
    const uint32_t page = ct[kCtHeader + (cp >> 8)];
    if (page >= ct[MADTP_TEXT_CT_PAGES]) return (uint32_t)kKindRefuse << kKindShift;
    return ct[kCtHeader + kPageWords + (size_t)page * 256 + (cp & 255)];
}

TX_HD int entry_kind(uint32_t e) { return (int)((e >> kKindShift) & 7); }
TX_HD int entry_count(uint32_t e) { return entry_kind(e) > 3 ? 0 : entry_kind(e); }  // REFUSE, or a kind there is not: none

// output k < entry_count(e) of cp: codepoint | class << 21
TX_HD uint32_t entry_out(const uint32_t* ct, uint32_t e, uint32_t cp, int k) {
    if (entry_kind(e) == 1) return ((cp + (e & kCpMask)) & kCpMask) | (e & (3u << kClassShift));
    const uint32_t at = (e & kCpMask) + (uint32_t)k;
    if (at >= ct[MADTP_TEXT_CT_POOL]) return ' ' | ((uint32_t)MADTP_TEXT_CLASS_SPACE << kClassShift);
    return ct[kCtHeader + kPageWords + (size_t)ct[MADTP_TEXT_CT_PAGES] * 256 + at] & (kCpMask | (3u << kClassShift));
}

TX_HD int klass(uint32_t w) { return (int)((w >> kClassShift) & 3); }
TX_HD bool is_word_char(uint32_t w) { return klass(w) == MADTP_TEXT_CLASS_OTHER; }

inline int chartable_check(const uint32_t* ct, int64_t words) {
    if (!ct || words < kCtHeader + kPageWords || ct[0] != (uint32_t)MADTP_TEXT_CT_MAGIC) return MADTP_TEXT_E_TABLE;
    const uint64_t pages = ct[MADTP_TEXT_CT_PAGES], pool = ct[MADTP_TEXT_CT_POOL];
    if (pages < 1 || pages > kPageWords || (uint64_t)words != kCtHeader + kPageWords + pages * 256 + pool || ct[MADTP_TEXT_CT_WORDS] != (uint64_t)words)
        return MADTP_TEXT_E_TABLE;
    for (int len = 1; len <= 4; ++len)
        if (ct[MADTP_TEXT_CT_EXPAND + len - 1] > (uint32_t)len) return MADTP_TEXT_E_TABLE;
    for (uint32_t cp = 0; cp <= kMaxCp; ++cp) {
        if (ct[kCtHeader + (cp >> 8)] >= pages) return MADTP_TEXT_E_TABLE;
        const uint32_t e = ct_entry(ct, cp);
        const int kind = entry_kind(e), len = cp < 0x80 ? 1 : cp < 0x800 ? 2 : cp < 0x10000 ? 3 : 4;
        if (kind == kKindRefuse || kind == 0) continue;
        if (kind > 3 || kind > len || (uint32_t)kind > ct[MADTP_TEXT_CT_EXPAND + len - 1]) return MADTP_TEXT_E_TABLE;
        if (kind > 1 && (uint64_t)(e & kCpMask) + kind > pool) return MADTP_TEXT_E_TABLE;
        for (int k = 0; k < kind; ++k)
            if ((entry_out(ct, e, cp, k) & kCpMask) > kMaxCp) return MADTP_TEXT_E_TABLE;
    }
    return 0;
}

// ---- the vocabulary table -------------------------------------------------------------------------------------------------------------
TX_HD uint64_t hash_step(uint64_t h, uint32_t cp) { return h * kMul + (cp + 1); }
TX_HD uint64_t hash_prefix() { return hash_step(hash_step(0, '#'), '#'); }  // of "##"
TX_HD uint32_t hash_slot(uint64_t h, uint32_t slots) { return (uint32_t)((h * kFold) >> 32) & (slots - 1); }
TX_HD uint32_t hash_tag(uint64_t h) { return (uint32_t)(h >> 32); }

// the header of a vocabulary blob, read once per workgroup: sizes a lane checks its indices against
struct Vocab {
    const uint32_t *starts, *pool, *hash, *specials;
    uint32_t entries, pool_words, slots, longest, n_special;
    int32_t pad, unk, cls, sep;
    bool ok;
};

TX_HD Vocab vocab_view(const uint32_t* v) {
    Vocab o;
    o.entries = v[MADTP_TEXT_V_ENTRIES], o.pool_words = v[MADTP_TEXT_V_POOL], o.slots = v[MADTP_TEXT_V_SLOTS];
    o.longest = v[MADTP_TEXT_V_LONGEST], o.n_special = v[MADTP_TEXT_V_SPECIALS];
    o.pad = (int32_t)v[MADTP_TEXT_V_PAD], o.unk = (int32_t)v[MADTP_TEXT_V_UNK], o.cls = (int32_t)v[MADTP_TEXT_V_CLS], o.sep = (int32_t)v[MADTP_TEXT_V_SEP];
    o.starts = v + v[MADTP_TEXT_V_OFF_STARTS], o.pool = v + v[MADTP_TEXT_V_OFF_POOL], o.hash = v + v[MADTP_TEXT_V_OFF_HASH];
    o.specials = v + v[MADTP_TEXT_V_OFF_SPECIALS];
    o.ok = v[0] == (uint32_t)MADTP_TEXT_V_MAGIC && o.entries >= 4 && o.entries <= MADTP_TEXT_MAX_VOCAB && o.slots >= 2 * o.entries &&
           (o.slots & (o.slots - 1)) == 0 && o.longest <= MADTP_TEXT_MAX_PIECE_CHARS && o.n_special <= MADTP_TEXT_MAX_SPECIALS &&
           v[MADTP_TEXT_V_OFF_STARTS] == (uint32_t)kVHeader && v[MADTP_TEXT_V_OFF_POOL] == kVHeader + o.entries + 1 &&
           v[MADTP_TEXT_V_OFF_HASH] == v[MADTP_TEXT_V_OFF_POOL] + o.pool_words &&
           v[MADTP_TEXT_V_OFF_SPECIALS] == v[MADTP_TEXT_V_OFF_HASH] + 2 * o.slots &&
           v[MADTP_TEXT_V_WORDS] == v[MADTP_TEXT_V_OFF_SPECIALS] + (uint32_t)MADTP_TEXT_MAX_SPECIALS * kSpecialWords;
    return o;
}

// the id of the piece norm[j .. e) (with "##" in front when cont), whose hash is h, or -1.  A slot's tag only spares a comparison:
// the piece's codepoints in the pool decide.
TX_HD int32_t vocab_find(const Vocab& v, uint64_t h, const uint32_t* norm, int j, int e, bool cont) {
    uint32_t at = hash_slot(h, v.slots);
    const uint32_t tag = hash_tag(h), len = (uint32_t)(e - j), skip = cont ? 2u : 0u;
    for (uint32_t probe = 0; probe < v.slots; ++probe, at = (at + 1) & (v.slots - 1)) {
        const uint32_t id1 = v.hash[2 * (size_t)at];
        if (id1 == 0) return -1;
        if (v.hash[2 * (size_t)at + 1] != tag || id1 > v.entries) continue;
        const uint32_t s = v.starts[id1 - 1], t = v.starts[id1];
        if (t < s || t > v.pool_words || t - s != len + skip) continue;
        bool same = !cont || (v.pool[s] == '#' && v.pool[s + 1] == '#');
        for (uint32_t k = 0; same && k < len; ++k) same = v.pool[s + skip + k] == (norm[j + k] & kCpMask);
        if (same) return (int32_t)(id1 - 1);
    }
    return -1;
}

// ---- the host side of the vocabulary ----------------------------------------------------------------------------------------------------
inline bool entries_ok(const void* entries, const int64_t* off, int n) {
    if (!entries || !off || n < 1 || n > MADTP_TEXT_MAX_VOCAB || off[0] < 0) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > 4 * (int64_t)MADTP_TEXT_MAX_PIECE_CHARS) return false;
    return true;
}

inline uint32_t slots_for(int n) {
    uint32_t s = 8;
    while (s < 2 * (uint32_t)n) s <<= 1;
    return s;
}

inline int64_t vocab_words(const void* entries, const int64_t* off, int n, int n_special) {
    if (!entries_ok(entries, off, n) || n_special < 0 || n_special > MADTP_TEXT_MAX_SPECIALS) return MADTP_E_BADARG;
    const uint8_t* b = (const uint8_t*)entries;
    int64_t chars = 0;
    for (int64_t i = off[0]; i < off[n]; ++i) chars += (b[i] & 0xC0) != 0x80;  // an upper bound where an entry is malformed
    return kVHeader + (int64_t)n + 1 + chars + 2 * (int64_t)slots_for(n) + (int64_t)MADTP_TEXT_MAX_SPECIALS * kSpecialWords;
}

inline bool entry_is(const uint8_t* b, int64_t len, const char* lit) {
    int64_t k = 0;
    for (; lit[k]; ++k)
        if (k >= len || b[k] != (uint8_t)lit[k]) return false;
    return k == len;
}

inline int vocab_build(const void* entries, const int64_t* off, int n, const int32_t* specials, int n_special, void* out, int64_t out_bytes) {
    const int64_t words = vocab_words(entries, off, n, n_special);
    if (words < 0) return (int)words;
    if (!out || (n_special && !specials) || out_bytes < words * 4 || words > 0x7FFFFFFF) return MADTP_E_BADARG;
    const uint8_t* b = (const uint8_t*)entries;
    uint32_t* v = (uint32_t*)out;
    for (int64_t i = 0; i < words; ++i) v[i] = 0;
    const uint32_t slots = slots_for(n);
    uint32_t* starts = v + kVHeader;
    uint32_t* pool = starts + n + 1;
    int32_t named[4] = {-1, -1, -1, -1};
    static const char* const kNames[4] = {"[PAD]", "[UNK]", "[CLS]", "[SEP]"};
    uint32_t at = 0, longest = 0;
    for (int i = 0; i < n; ++i) {
        const uint8_t* e = b + off[i];
        const int len = (int)(off[i + 1] - off[i]);
        if (len == 0) return MADTP_TEXT_E_VOCAB_EMPTY;
        starts[i] = at;
        for (int p = 0; p < len;) {
            uint32_t cp = 0;
            const int l = decode_at(e, len, p, &cp);
            if (l <= 0) return MADTP_TEXT_E_VOCAB_ENTRY;
            pool[at++] = cp;
            p += l;
        }
        if (at - starts[i] > MADTP_TEXT_MAX_PIECE_CHARS) return MADTP_TEXT_E_VOCAB_ENTRY;
        longest = at - starts[i] > longest ? at - starts[i] : longest;
        for (int k = 0; k < 4; ++k)
            if (entry_is(e, len, kNames[k])) named[k] = i;
    }
    starts[n] = at;
    uint32_t* pool_end = pool + at;  // the pool takes the codepoints there are; the hash table follows it
    uint32_t* hash = pool_end;
    for (int i = 0; i < n; ++i) {
        uint64_t h = 0;
        for (uint32_t k = starts[i]; k < starts[i + 1]; ++k) h = hash_step(h, pool[k]);
        uint32_t s = hash_slot(h, slots);
        for (;; s = (s + 1) & (slots - 1)) {  // at most n occupied slots of >= 2 n: ends
            const uint32_t id1 = hash[2 * (size_t)s];
            if (id1 == 0) break;
            const uint32_t a = starts[id1 - 1], len = starts[id1] - a;
            if (hash[2 * (size_t)s + 1] != hash_tag(h) || len != starts[i + 1] - starts[i]) continue;
            bool same = true;
            for (uint32_t k = 0; same && k < len; ++k) same = pool[a + k] == pool[starts[i] + k];
            if (same) return MADTP_TEXT_E_VOCAB_DUP;
        }
        hash[2 * (size_t)s] = (uint32_t)i + 1;
        hash[2 * (size_t)s + 1] = hash_tag(h);
    }
    for (int k = 0; k < 4; ++k)
        if (named[k] < 0) return MADTP_TEXT_E_VOCAB_MISSING;
    uint32_t* sp = hash + 2 * (size_t)slots;
    uint32_t n_sp = 0;
    for (int k = 0; k < 4 + n_special; ++k) {
        const int32_t id = k < 4 ? named[k] : specials[k - 4];
        if (id < 0 || id >= n) return MADTP_TEXT_E_VOCAB_ENTRY;
        const int len = (int)(off[id + 1] - off[id]);
        if (len > MADTP_TEXT_MAX_SPECIAL_BYTES) return MADTP_TEXT_E_VOCAB_ENTRY;
        bool seen = false;
        for (uint32_t q = 0; q < n_sp; ++q) seen = seen || sp[q * kSpecialWords + 1] == (uint32_t)id;
        if (seen) continue;
        if (n_sp == MADTP_TEXT_MAX_SPECIALS) return MADTP_TEXT_E_VOCAB_ENTRY;
        uint32_t* row = sp + n_sp++ * kSpecialWords;
        row[0] = (uint32_t)len, row[1] = (uint32_t)id;
        for (int q = 0; q < len; ++q) row[2 + q] = b[off[id] + q];
    }
    v[0] = (uint32_t)MADTP_TEXT_V_MAGIC;
    v[MADTP_TEXT_V_ENTRIES] = (uint32_t)n, v[MADTP_TEXT_V_POOL] = at, v[MADTP_TEXT_V_SLOTS] = slots, v[MADTP_TEXT_V_LONGEST] = longest;
    v[MADTP_TEXT_V_PAD] = (uint32_t)named[0], v[MADTP_TEXT_V_UNK] = (uint32_t)named[1], v[MADTP_TEXT_V_CLS] = (uint32_t)named[2], v[MADTP_TEXT_V_SEP] = (uint32_t)named[3];
    v[MADTP_TEXT_V_SPECIALS] = n_sp;
    v[MADTP_TEXT_V_OFF_STARTS] = kVHeader, v[MADTP_TEXT_V_OFF_POOL] = (uint32_t)(pool - v), v[MADTP_TEXT_V_OFF_HASH] = (uint32_t)(hash - v);
    v[MADTP_TEXT_V_OFF_SPECIALS] = (uint32_t)(sp - v);
    v[MADTP_TEXT_V_WORDS] = (uint32_t)(sp - v) + (uint32_t)MADTP_TEXT_MAX_SPECIALS * kSpecialWords;
    return 0;
}

// ---- encode ------------------------------------------------------------------------------------------------------------------------------
struct Shared {
    uint32_t norm[kMaxBytes];      // the normalised text: codepoint | class << 21
    int32_t hit_id[kMaxBytes];     // per position: the longest piece that begins there (the word-initial form at a word's start, the
    uint16_t hit_next[kMaxBytes];  // "##" form elsewhere), or -1; and where it ends
    uint16_t wnum[kMaxBytes];      // per position: its word
    uint16_t wstart[kMaxBytes], wend[kMaxBytes];  // per word
    int32_t tot[kLanes];
    int32_t flag[3];               // E_UTF8, E_SPECIAL, E_CHAR
};

TX_HD int lanes_before(const Shared& sh, int lane) {
    int s = 0;
    for (int j = 0; j < lane; ++j) s += sh.tot[j];
    return s;
}

TX_HD bool special_at(const Vocab& v, const uint8_t* t, int n, int i) {
    for (uint32_t s = 0; s < v.n_special; ++s) {
        const uint32_t* row = v.specials + s * kSpecialWords;
        const int len = (int)row[0];
        if (len < 1 || len > MADTP_TEXT_MAX_SPECIAL_BYTES || i + len > n) continue;
        bool same = true;
        for (int k = 0; same && k < len; ++k) same = row[2 + k] == t[i + k];
        if (same) return true;
    }
    return false;
}

TX_HD bool word_start(const Shared& sh, int j) {
    const int c = klass(sh.norm[j]);
    if (c == MADTP_TEXT_CLASS_SPACE) return false;
    return c != MADTP_TEXT_CLASS_OTHER || j == 0 || !is_word_char(sh.norm[j - 1]);
}

TX_HD bool word_end(const Shared& sh, int j, int n) {
    const int c = klass(sh.norm[j]);
    if (c == MADTP_TEXT_CLASS_SPACE) return false;
    return c != MADTP_TEXT_CLASS_OTHER || j == n - 1 || !is_word_char(sh.norm[j + 1]);
}

// the chain of word w from its start: -> its tokens, 0 meaning one [UNK]; kWrite puts the ids at row[at ..] below `limit`
template <bool kWrite>
TX_HD int walk_word(const Shared& sh, int w, int n, int64_t* row, int at, int limit) {
    const int ws = sh.wstart[w], we = sh.wend[w];
    if (ws >= we || we > n || we - ws > kMaxWord) return 0;
    int p = ws, count = 0;
    for (int step = 0; step < kMaxWord && p < we; ++step) {
        const int32_t id = sh.hit_id[p];
        const int nx = sh.hit_next[p];
        if (id < 0 || nx <= p || nx > we) return 0;
        if (kWrite && at + count < limit) row[at + count] = id;
        p = nx;
        ++count;
    }
    return p == we ? count : 0;
}

// text b of the batch.  Uniform; writes status[2 b], status[2 b + 1] and, without a code, row b of ids_out / mask_out.
TX_HD void encode_text(Shared& sh, const uint8_t* bytes, const int64_t* offsets, const uint32_t* ct, const uint32_t* vocab, int64_t* ids_out,
                       int64_t* mask_out, int32_t* status, int b, int width, int max_tokens, int flags) {
    const Vocab v = vocab_view(vocab);
    const int64_t begin = offsets[b], end = offsets[b + 1];
    int code = 0, tokens = 0;
    if (!v.ok || ct[0] != (uint32_t)MADTP_TEXT_CT_MAGIC) code = MADTP_TEXT_E_TABLE;
    else if (begin < 0 || end < begin || end - begin > kMaxBytes) code = MADTP_TEXT_E_LONG;
    if (code) {
        if (first_lane()) status[2 * b] = code, status[2 * b + 1] = 0;
        return;
    }
    const uint8_t* t = bytes + begin;
    const int nb = (int)(end - begin), m = (nb + kLanes - 1) / kLanes;  // a lane owns bytes [lane m, lane m + m)

    // (a) decode and validate every byte, look for special literals, count the normalised codepoints
    each_lane([&](int lane) {
        if (lane < 3) sh.flag[lane] = 0;
    });
    sync_lanes();
    each_lane([&](int lane) {
        int count = 0;
        for (int i = lane * m; i < nb && i < lane * m + m; ++i) {
            uint32_t cp = 0;
            const int len = decode_at(t, nb, i, &cp);
            if (len < 0) sh.flag[0] = 1;
            if (special_at(v, t, nb, i)) sh.flag[1] = 1;
            if (len > 0) {
                const uint32_t e = ct_entry(ct, cp);
                if (entry_kind(e) == kKindRefuse) sh.flag[2] = 1;
                count += entry_count(e) < len ? entry_count(e) : len;
            }
        }
        sh.tot[lane] = count;
    });
    sync_lanes();
    code = sh.flag[0] ? MADTP_TEXT_E_UTF8 : sh.flag[1] ? MADTP_TEXT_E_SPECIAL : sh.flag[2] ? MADTP_TEXT_E_CHAR : 0;
    if (code) {
        if (first_lane()) status[2 * b] = code, status[2 * b + 1] = 0;
        return;
    }
    int n = 0;
    for (int j = 0; j < kLanes; ++j) n += sh.tot[j];  // <= nb: a codepoint gives at most as many as it has bytes

    // (b) the normalised codepoints and their classes, compacted
    each_lane([&](int lane) {
        int at = lanes_before(sh, lane);
        for (int i = lane * m; i < nb && i < lane * m + m; ++i) {
            uint32_t cp = 0;
            const int len = decode_at(t, nb, i, &cp);
            if (len <= 0) continue;
            const uint32_t e = ct_entry(ct, cp);
            const int outs = entry_count(e) < len ? entry_count(e) : len;
            for (int k = 0; k < outs; ++k, ++at)
                if (at < kMaxBytes) sh.norm[at] = entry_out(ct, e, cp, k);
        }
    });
    sync_lanes();

    // (c) words: a run of OTHER characters, or one PUNCT / SPACED character.  The w-th start and the w-th end are one word's.
    const int mn = (n + kLanes - 1) / kLanes;
    each_lane([&](int lane) {
        int count = 0;
        for (int j = lane * mn; j < n && j < lane * mn + mn; ++j) count += word_start(sh, j);
        sh.tot[lane] = count;
    });
    sync_lanes();
    int words = 0;
    for (int j = 0; j < kLanes; ++j) words += sh.tot[j];
    each_lane([&](int lane) {
        int seen = lanes_before(sh, lane);
        for (int j = lane * mn; j < n && j < lane * mn + mn; ++j) {
            if (word_start(sh, j)) sh.wstart[seen++] = (uint16_t)j;
            sh.wnum[j] = (uint16_t)(seen > 0 ? seen - 1 : 0);
            if (word_end(sh, j, n) && seen > 0) sh.wend[seen - 1] = (uint16_t)(j + 1);
        }
    });
    sync_lanes();

    // (d) per position the longest piece that begins there: the hash grows with the piece, the last confirmed hit stays
    each_lane([&](int lane) {
        for (int j = lane; j < n; j += kLanes) {
            int32_t best = -1;
            int next = j;
            if (klass(sh.norm[j]) != MADTP_TEXT_CLASS_SPACE) {
                const int w = sh.wnum[j];
                const int ws = sh.wstart[w], we = sh.wend[w];
                if (w < words && ws <= j && j < we && we <= n && we - ws <= kMaxWord) {
                    const bool cont = j != ws;
                    const int longest = (int)v.longest - (cont ? 2 : 0);
                    uint64_t h = cont ? hash_prefix() : 0;
                    for (int e = j + 1; e <= we && e - j <= longest; ++e) {
                        h = hash_step(h, sh.norm[e - 1] & kCpMask);
                        const int32_t id = vocab_find(v, h, sh.norm, j, e, cont);
                        if (id >= 0) best = id, next = e;
                    }
                }
            }
            sh.hit_id[j] = best;
            sh.hit_next[j] = (uint16_t)next;
        }
    });
    sync_lanes();

    // (e) tokens per word, their offsets
    const int mw = (words + kLanes - 1) / kLanes;
    each_lane([&](int lane) {
        int count = 0;
        for (int w = lane * mw; w < words && w < lane * mw + mw; ++w) {
            const int c = walk_word<false>(sh, w, n, nullptr, 0, 0);
            count += c ? c : 1;
        }
        sh.tot[lane] = count;
    });
    sync_lanes();
    for (int j = 0; j < kLanes; ++j) tokens += sh.tot[j];
    tokens += 2;
    if (tokens > max_tokens && !(flags & MADTP_TEXT_TRUNCATE)) {
        if (first_lane()) status[2 * b] = MADTP_TEXT_E_TOKENS, status[2 * b + 1] = tokens;
        return;
    }

    // (f) the row: [CLS], the first max_tokens - 2 ids, [SEP], [PAD]; every cell has one writer
    const int kept = tokens < max_tokens ? tokens : max_tokens;
    int64_t* ids = ids_out + (size_t)b * width;
    int64_t* mask = mask_out + (size_t)b * width;
    each_lane([&](int lane) {
        int at = 1 + lanes_before(sh, lane);
        for (int w = lane * mw; w < words && w < lane * mw + mw; ++w) {
            const int c = walk_word<false>(sh, w, n, nullptr, 0, 0);  // first: a chain that breaks must not have written
            if (c) walk_word<true>(sh, w, n, ids, at, kept - 1);
            else if (at < kept - 1) ids[at] = v.unk;
            at += c ? c : 1;
        }
        for (int col = lane; col < width; col += kLanes) {
            mask[col] = col < kept;
            if (col == 0) ids[col] = v.cls;
            else if (col == kept - 1) ids[col] = v.sep;
            else if (col >= kept) ids[col] = v.pad;
        }
    });
    if (first_lane()) status[2 * b] = 0, status[2 * b + 1] = tokens;
}

inline int encode_args(const void* bytes, const int64_t* offsets, const uint32_t* ct, const uint32_t* vocab, const int64_t* ids, const int64_t* mask,
                       const int32_t* status, int B, int width, int max_tokens, int flags) {
    if (!bytes || !offsets || !ct || !vocab || !ids || !mask || !status || B < 1 || B > MADTP_TEXT_MAX_BATCH) return MADTP_E_BADARG;
    if (max_tokens < 2 || max_tokens > width || width > kMaxTokens || (flags & ~MADTP_TEXT_TRUNCATE)) return MADTP_E_BADARG;
    return 0;
}

inline int encode_host(const void* bytes, const int64_t* offsets, const uint32_t* ct, const uint32_t* vocab, int64_t* ids, int64_t* mask,
                       int32_t* status, int B, int width, int max_tokens, int flags) {
    if (int rc = encode_args(bytes, offsets, ct, vocab, ids, mask, status, B, width, max_tokens, flags)) return rc;
    Shared sh;
    for (int b = 0; b < B; ++b) encode_text(sh, (const uint8_t*)bytes, offsets, ct, vocab, ids, mask, status, b, width, max_tokens, flags);
    return 0;
}

}  // namespace madtp_text
