// Stand-alone check of the lane routines and the passes of the device Huffman stage (madtp_amd/csrc/jpeg_huff_device.h) against the
// host decoder (madtp_amd/csrc/jpeg_entropy.h) under the host compiler's sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jhuff_host_check.cpp -o jhuff_host_check
//     ./jhuff_host_check DIR/*.jpg          (python tools/make_jpeg_golden.py --dump DIR writes the corpus)
//
// Every file is decoded by both, at subsequence sizes 4 and the default, into heap buffers of exactly 64 * BLOCKS elements and from
// an exact-size copy of the bytes (a read or write past either is the sanitizer's to catch): whole, truncated at every length near
// both ends and a spread in between, and with single bytes of the scan flipped at seeded positions.  Whole: code 0 and equal
// coefficients.  Truncated: the host decoder's code.  Flipped: a code on both sides, or success on both with equal coefficients;
// how often the two codes themselves differ is counted and printed.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../madtp_amd/csrc/jpeg_huff_device.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

struct Counts {
    long runs = 0, codes = 0, decoded = 0, other_code = 0, serial = 0, failures = 0;
    long passes = 0, subseqs = 0;
};

// one byte string through both decoders -> true if they agree as the kind demands (kind: 0 whole, 1 truncated, 2 flipped)
static bool both(const std::vector<uint8_t>& bytes, int subseq, int kind, Counts& c, const char* what, size_t at) {
    static madtp_jpeg::Header h;
    static madtp_jhuff::Shared sh;
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);  // no slack behind the last byte
    if (!bytes.empty()) memcpy(exact.get(), bytes.data(), bytes.size());
    const int64_t size = (int64_t)bytes.size();
    int32_t info[MADTP_JPEG_INFO_FIELDS];
    uint16_t q[3 * 64];
    ++c.runs;
    if (madtp_jpeg::inspect(exact.get(), size, info, q) != 0) {
        std::vector<int16_t> one(64);
        int32_t status[4];
        const int a = madtp_jpeg::entropy_decode(exact.get(), size, one.data(), 64);
        const int b = madtp_jhuff::decode_host(exact.get(), size, subseq, one.data(), 64, status, h, sh);
        ++c.codes;
        if (a == b) return true;
        printf("%s at %zu, subsequences of %d: header code %d against %d\n", what, at, subseq, a, b);
        return false;
    }
    const int64_t n = 64 * (int64_t)info[MADTP_JPEG_I_BLOCKS];
    std::vector<int16_t> want((size_t)n), got((size_t)n, (int16_t)0x7b7b);
    int32_t status[4];
    const int a = madtp_jpeg::entropy_decode(exact.get(), size, want.data(), n);
    const int b = madtp_jhuff::decode_host(exact.get(), size, subseq, got.data(), n, status, h, sh);
    c.serial += status[MADTP_JHUFF_S_SERIAL];
    c.passes += status[MADTP_JHUFF_S_PASSES], c.subseqs += status[MADTP_JHUFF_S_SUBSEQS];
    bool ok = status[MADTP_JHUFF_S_CODE] == b && status[MADTP_JHUFF_S_PASSES] <= status[MADTP_JHUFF_S_SUBSEQS] && status[MADTP_JHUFF_S_PASSES] >= 1;
    if (a == 0 && b == 0) {
        ++c.decoded;
        ok = ok && kind != 1 && memcmp(want.data(), got.data(), (size_t)n * 2) == 0;
    } else {
        ++c.codes;
        if (a != b) ++c.other_code;
        ok = ok && a != 0 && b != 0 && kind != 0 && (kind == 2 || a == b);
    }
    if (!ok) printf("%s at %zu, subsequences of %d: host decoder %d, lanes %d (passes %d of %d)\n", what, at, subseq, a, b,
                    status[MADTP_JHUFF_S_PASSES], status[MADTP_JHUFF_S_SUBSEQS]);
    return ok;
}

int main(int argc, char** argv) {
    Counts c;
    int flips = 2000;
    int first = 1;
    if (argc > 2 && strcmp(argv[1], "--flips") == 0) flips = atoi(argv[2]), first = 3;
    for (int a = first; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            printf("%s: cannot open\n", argv[a]);
            ++c.failures;
            continue;
        }
        std::vector<uint8_t> file;
        uint8_t chunk[4096];
        for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
        fclose(f);
        madtp_jpeg::Header h;
        if (madtp_jpeg::parse_header(file.data(), (int64_t)file.size(), h) != 0) {
            printf("%s: not a file of the corpus\n", argv[a]);
            ++c.failures;
            continue;
        }
        const size_t size = file.size();
        for (int subseq : {4, 0}) {
            if (!both(file, subseq, 0, c, argv[a], size)) ++c.failures;
            for (size_t len = 0; len < size; len += (len < 700 || len + 64 > size) ? 1 : 1 + size / 97) {
                std::vector<uint8_t> cut(file.begin(), file.begin() + len);
                if (!both(cut, subseq, 1, c, argv[a], len)) ++c.failures;
            }
            uint32_t seed = 12345u + (uint32_t)size;
            for (int i = 0; i < flips; ++i) {
                std::vector<uint8_t> bad(file);
                const size_t lo = (size_t)h.scan_begin;
                const size_t at = lo + lcg(seed) % (size - lo);
                bad[at] ^= (uint8_t)(1u << (lcg(seed) >> 29)) | (i % 3 == 0 ? 0xFF : 0);
                if (!both(bad, subseq, 2, c, argv[a], at)) ++c.failures;
            }
        }
    }
    printf("%d files, %ld decodes by both: %ld ended in a code on both sides (%ld with another code than the host decoder's), %ld decoded "
           "to equal coefficients, %ld went to the serial lane; %ld passes over %ld subsequences; %ld failures\n",
           argc - first, c.runs, c.codes, c.other_code, c.decoded, c.serial, c.passes, c.subseqs, c.failures);
    return c.failures ? 1 : 0;
}
