// Stand-alone check of the vocabulary builder and of the host emulation of the text kernel (madtp_amd/csrc/text_device.h) under the
// host compiler's sanitizers:
//
//     python tools/make_text_golden.py --dump DIR          (writes chartable.bin, vocab.txt, texts.bin)
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/text_host_check.cpp -o text_host_check
//     ./text_host_check DIR
//
// Every buffer is a heap block of exactly the size the interface names (a read or write past one is the sanitizer's to catch): the
// tables, each text's bytes, its row of ids and of the mask, its two status words.  The corpus is encoded whole, then every
// truncation of every text, then every text with bytes replaced at seeded positions (invalid UTF-8 included), then with a special
// token's literal or a REFUSE codepoint put in and grown past the byte limit, each of which must give its own code.  Every run is made
// twice, on workgroup memory poisoned with two different patterns: it must end in the same code both times, or in the same ids -
// which are then those of an undamaged re-encode of the same bytes.  A whole text of the corpus must encode (or have more than 512
// tokens).  CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../madtp_amd/csrc/text_device.h"

using namespace madtp_text;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> out;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
        printf("%s: cannot open\n", path.c_str());
        exit(2);
    }
    uint8_t chunk[65536];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) out.insert(out.end(), chunk, chunk + n);
    fclose(f);
    return out;
}

struct Result {
    int32_t status[2];
    std::vector<int64_t> ids, mask;
    bool operator==(const Result& o) const { return status[0] == o.status[0] && status[1] == o.status[1] && ids == o.ids && mask == o.mask; }
};

// one text in exact-size blocks, on a Shared filled with `poison`
static Result encode(const uint8_t* text, size_t n, const uint32_t* ct, const uint32_t* vocab, int width, int max_tokens, int flags, int poison) {
    std::unique_ptr<uint8_t[]> bytes(new uint8_t[n ? n : 1]);  // (n == 0: a block of one byte that is never read)
    if (n) memcpy(bytes.get(), text, n);
    std::unique_ptr<int64_t[]> off(new int64_t[2]{0, (int64_t)n}), ids(new int64_t[width]), mask(new int64_t[width]);
    std::unique_ptr<int32_t[]> status(new int32_t[2]{77, 77});
    for (int i = 0; i < width; ++i) ids[i] = mask[i] = -7;
    std::unique_ptr<Shared> sh(new Shared);
    memset(sh.get(), poison, sizeof(Shared));
    if (encode_args(bytes.get(), off.get(), ct, vocab, ids.get(), mask.get(), status.get(), 1, width, max_tokens, flags)) {
        printf("encode_args refused a good call\n");
        exit(2);
    }
    encode_text(*sh, bytes.get(), off.get(), ct, vocab, ids.get(), mask.get(), status.get(), 0, width, max_tokens, flags);
    Result r;
    r.status[0] = status[0], r.status[1] = status[1];
    r.ids.assign(ids.get(), ids.get() + width);
    r.mask.assign(mask.get(), mask.get() + width);
    return r;
}

static long g_runs = 0, g_codes = 0, g_encoded = 0;
static long g_by_code[8] = {0};

// the rule of every run -> 0 or 1 failure
static int run(const char* what, size_t index, const uint8_t* text, size_t n, const uint32_t* ct, const uint32_t* vocab, int width, int max_tokens,
               int flags) {
    const Result a = encode(text, n, ct, vocab, width, max_tokens, flags, 0xAA), b = encode(text, n, ct, vocab, width, max_tokens, flags, 0x55);
    ++g_runs;
    bool ok = a == b;
    if (a.status[0]) {
        ++g_codes;
        const int k = -a.status[0] - 401;
        ok = ok && k >= 0 && k <= 4;
        if (k >= 0 && k <= 4) ++g_by_code[k];
        for (int i = 0; i < width; ++i) ok = ok && a.ids[i] == -7 && a.mask[i] == -7;  // a row with a code stays unwritten
    } else {
        ++g_encoded;
        const int kept = a.status[1] < max_tokens ? a.status[1] : max_tokens;
        ok = ok && a.status[1] >= 2 && (a.status[1] <= max_tokens || (flags & MADTP_TEXT_TRUNCATE));
        for (int i = 0; i < width; ++i) ok = ok && a.ids[i] >= 0 && a.mask[i] == (i < kept);
    }
    if (!ok) printf("%s of text %zu (%zu bytes): status %d %d / %d %d, rows %s\n", what, index, n, a.status[0], a.status[1], b.status[0], b.status[1],
                    a.ids == b.ids ? "equal" : "DIFFER");
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: text_host_check DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    int failures = 0;
    // the character table, exact size
    const std::vector<uint8_t> ct_file = slurp(dir + "/chartable.bin");
    std::unique_ptr<uint32_t[]> ct(new uint32_t[ct_file.size() / 4]);
    memcpy(ct.get(), ct_file.data(), ct_file.size() / 4 * 4);
    if (chartable_check(ct.get(), (int64_t)(ct_file.size() / 4))) {
        printf("chartable.bin is refused\n");
        return 1;
    }
    // the vocabulary: entries back to back in an exact-size block
    const std::vector<uint8_t> vf = slurp(dir + "/vocab.txt");
    std::vector<int64_t> offs(1, 0);
    std::vector<uint8_t> joined;
    for (size_t i = 0, start = 0; i <= vf.size(); ++i)
        if (i == vf.size() || vf[i] == '\n') {
            if (i > start || i < vf.size()) {
                joined.insert(joined.end(), vf.begin() + start, vf.begin() + i);
                offs.push_back((int64_t)joined.size());
            }
            start = i + 1;
        }
    const int n = (int)offs.size() - 1;
    std::unique_ptr<uint8_t[]> entries(new uint8_t[joined.size()]);
    memcpy(entries.get(), joined.data(), joined.size());
    std::unique_ptr<int64_t[]> eoff(new int64_t[n + 1]);
    memcpy(eoff.get(), offs.data(), sizeof(int64_t) * (n + 1));
    const int32_t listed[1] = {4};  // [MASK]: a special beyond the four the builder finds by name
    const int64_t words = vocab_words(entries.get(), eoff.get(), n, 1);
    if (words < 0) {
        printf("vocab_words -> %lld\n", (long long)words);
        return 1;
    }
    std::unique_ptr<uint32_t[]> vocab(new uint32_t[words]);
    int rc = vocab_build(entries.get(), eoff.get(), n, listed, 1, vocab.get(), words * 4);
    if (rc || vocab_build(entries.get(), eoff.get(), n, listed, 1, vocab.get(), words * 4 - 1) != MADTP_E_BADARG) {
        printf("vocab_build -> %d, or a blob one byte short was accepted\n", rc);
        return 1;
    }
    long builds = 1;
    {  // the builder's refusals, each on exact-size blocks: the first entry again at the end, an empty entry, every count of entries
        // below the first four specials, an entry cut inside a sequence
        std::unique_ptr<uint8_t[]> e2(new uint8_t[joined.size() + (size_t)eoff[1]]);
        memcpy(e2.get(), joined.data(), joined.size());
        memcpy(e2.get() + joined.size(), joined.data(), (size_t)eoff[1]);
        std::unique_ptr<int64_t[]> o2(new int64_t[n + 2]);
        memcpy(o2.get(), offs.data(), sizeof(int64_t) * (n + 1));
        o2[n + 1] = o2[n] + eoff[1];
        const int64_t w2 = vocab_words(e2.get(), o2.get(), n + 1, 0);
        std::unique_ptr<uint32_t[]> v2(new uint32_t[w2]);
        if (vocab_build(e2.get(), o2.get(), n + 1, nullptr, 0, v2.get(), w2 * 4) != MADTP_TEXT_E_VOCAB_DUP) ++failures, printf("a duplicate entry was accepted\n");
        o2[n + 1] = o2[n];
        if (vocab_build(e2.get(), o2.get(), n + 1, nullptr, 0, v2.get(), w2 * 4) != MADTP_TEXT_E_VOCAB_EMPTY) ++failures, printf("an empty entry was accepted\n");
        for (int k = 1; k < 4; ++k)
            if (vocab_build(entries.get(), eoff.get(), k, nullptr, 0, v2.get(), w2 * 4) != MADTP_TEXT_E_VOCAB_MISSING) ++failures, printf("%d entries were accepted\n", k);
        builds += 5;
        for (int i = 0; i < n; ++i)
            if (entries[eoff[i]] >= 0xC0) {  // an entry that begins with a multi-byte sequence: end it after the lead
                std::unique_ptr<int64_t[]> o3(new int64_t[i + 2]);
                memcpy(o3.get(), offs.data(), sizeof(int64_t) * (i + 1));
                o3[i + 1] = o3[i] + 1;
                if (vocab_build(entries.get(), o3.get(), i + 1, nullptr, 0, v2.get(), w2 * 4) != MADTP_TEXT_E_VOCAB_ENTRY) ++failures, printf("a cut entry was accepted\n");
                ++builds;
                break;
            }
    }
    // the texts: int64 count, int64 offsets[count + 1], bytes
    const std::vector<uint8_t> tf = slurp(dir + "/texts.bin");
    int64_t count = 0;
    memcpy(&count, tf.data(), 8);
    std::vector<int64_t> toff((size_t)count + 1);
    memcpy(toff.data(), tf.data() + 8, 8 * ((size_t)count + 1));
    const uint8_t* body = tf.data() + 8 * ((size_t)count + 2);
    uint32_t seed = 12345;
    long whole = 0, truncations = 0, flips = 0, inserts = 0;
    for (int64_t t = 0; t < count; ++t) {
        const uint8_t* text = body + toff[t];
        const size_t size = (size_t)(toff[t + 1] - toff[t]);
        const Result r = encode(text, size, ct.get(), vocab.get(), 512, 512, 0, 0xAA);
        if (r.status[0] != 0 && !(r.status[0] == MADTP_TEXT_E_TOKENS && r.status[1] > 512)) {
            printf("text %lld of the corpus: code %d\n", (long long)t, r.status[0]);
            ++failures;
        }
        failures += run("whole", (size_t)t, text, size, ct.get(), vocab.get(), 512, 512, 0);
        failures += run("whole, truncated to 35 tokens", (size_t)t, text, size, ct.get(), vocab.get(), 35, 35, MADTP_TEXT_TRUNCATE);
        whole += 2;
        for (size_t len = 0; len < size; ++len, ++truncations)
            failures += run("truncation", (size_t)t, text, len, ct.get(), vocab.get(), 64, (len & 1) ? 64 : 8, (len & 2) ? MADTP_TEXT_TRUNCATE : 0);
        std::vector<uint8_t> damaged(text, text + size);
        for (int v = 0; size && v < 24; ++v, ++flips) {
            damaged.assign(text, text + size);
            const int edits = 1 + (int)(lcg(seed) >> 30);
            for (int e = 0; e < edits; ++e) {
                const size_t at = (lcg(seed) >> 8) % size;
                const uint32_t kind = lcg(seed) >> 29;  // a random byte, a flipped bit, a lead, a continuation byte, 0xF4, 0xED
                damaged[at] = kind < 3 ? (uint8_t)(lcg(seed) >> 24) : kind == 3 ? damaged[at] ^ (uint8_t)(1u << (lcg(seed) >> 29))
                              : kind == 4 ? (uint8_t)(0xC0 | (lcg(seed) >> 26)) : kind == 5 ? (uint8_t)(0x80 | (lcg(seed) >> 26)) : kind == 6 ? 0xF4 : 0xED;
            }
            failures += run("damage", (size_t)t, damaged.data(), size, ct.get(), vocab.get(), 512, 512, (v & 1) ? MADTP_TEXT_TRUNCATE : 0);
        }
        // the three codes that damage never reaches, each where it must come: a special token's literal and a REFUSE codepoint
        // (U+1D165) put in front of and behind the whole text, the literal cut at each of its bytes, and the text grown past the limit
        if (r.status[0] == 0) {
            static const char* const kInserts[3] = {"[SEP]", "[MASK]", "\xf0\x9d\x85\xa5"};
            for (int k = 0; k < 3; ++k)
                for (int back = 0; back < 2; ++back, ++inserts) {
                    const size_t len = strlen(kInserts[k]);
                    damaged.assign(text, text + size);
                    damaged.insert(back ? damaged.end() : damaged.begin(), kInserts[k], kInserts[k] + len);
                    const int want = damaged.size() > MADTP_TEXT_MAX_BYTES ? MADTP_TEXT_E_LONG : k < 2 ? MADTP_TEXT_E_SPECIAL : MADTP_TEXT_E_CHAR;
                    const Result got = encode(damaged.data(), damaged.size(), ct.get(), vocab.get(), 512, 512, MADTP_TEXT_TRUNCATE, 0xAA);
                    if (got.status[0] != want) ++failures, printf("text %lld with %s: code %d, not %d\n", (long long)t, kInserts[k], got.status[0], want);
                    failures += run("insertion", (size_t)t, damaged.data(), damaged.size(), ct.get(), vocab.get(), 512, 512, MADTP_TEXT_TRUNCATE);
                    for (size_t cut = 1; back && cut < len; ++cut, ++inserts)
                        failures += run("cut insertion", (size_t)t, damaged.data(), damaged.size() - cut, ct.get(), vocab.get(), 512, 512, MADTP_TEXT_TRUNCATE);
                }
            damaged.assign(text, text + size);
            damaged.resize(MADTP_TEXT_MAX_BYTES + 1 + (size_t)(t % 7), 'x');
            const Result got = encode(damaged.data(), damaged.size(), ct.get(), vocab.get(), 512, 512, MADTP_TEXT_TRUNCATE, 0xAA);
            if (got.status[0] != MADTP_TEXT_E_LONG) ++failures, printf("text %lld grown past the limit: code %d\n", (long long)t, got.status[0]);
            failures += run("grown", (size_t)t, damaged.data(), damaged.size(), ct.get(), vocab.get(), 512, 512, MADTP_TEXT_TRUNCATE);
            ++inserts;
        }
    }
    printf("%d vocabulary entries, %ld builds; %lld texts: %ld whole runs, %ld truncations, %ld damaged copies, %ld insertions; %ld runs (each twice): %ld encoded, "
           "%ld refused (LONG %ld, UTF8 %ld, SPECIAL %ld, CHAR %ld, TOKENS %ld); %d failures\n",
           n, builds, (long long)count, whole, truncations, flips, inserts, g_runs, g_encoded, g_codes, g_by_code[0], g_by_code[1], g_by_code[2], g_by_code[3],
           g_by_code[4], failures);
    return failures ? 1 : 0;
}
