// Stand-alone check of the host stage of the JPEG decode (madtp_amd/csrc/jpeg_entropy.h) under the host compiler's sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//     ./jpeg_host_check DIR/*.jpg          (python tools/make_jpeg_golden.py --dump DIR writes the corpus)
//
// Every file is inspected and decoded into a heap buffer of exactly the size inspect() reports (a write past it is the sanitizer's
// to catch), then decoded again truncated at a spread of lengths and with single bytes of the scan flipped at seeded positions.  A
// whole file must decode; a damaged one must return a code or decode, and a truncated one must never decode.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madtp_amd/csrc/jpeg_entropy.h"

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

int main(int argc, char** argv) {
    int failures = 0;
    long runs = 0, refused = 0, decoded = 0;
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) {
            printf("%s: cannot open\n", argv[a]);
            ++failures;
            continue;
        }
        std::vector<uint8_t> file;
        uint8_t chunk[4096];
        for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
        fclose(f);
        int32_t info[MADTP_JPEG_INFO_FIELDS];
        uint16_t q[3 * 64];
        int rc = madtp_jpeg::inspect(file.data(), (int64_t)file.size(), info, q);
        if (rc) {
            printf("%s: inspect -> %d (%s)\n", argv[a], rc, madtp_jpeg::strerror_jpeg(rc));
            ++failures;
            continue;
        }
        const int64_t n_coef = 64 * (int64_t)info[MADTP_JPEG_I_BLOCKS];
        std::vector<int16_t> coef((size_t)n_coef);
        rc = madtp_jpeg::entropy_decode(file.data(), (int64_t)file.size(), coef.data(), n_coef);
        if (rc) {
            printf("%s: decode -> %d (%s)\n", argv[a], rc, madtp_jpeg::strerror_jpeg(rc));
            ++failures;
        }
        if (madtp_jpeg::entropy_decode(file.data(), (int64_t)file.size(), coef.data(), n_coef - 1) != MADTP_E_BADARG) {
            printf("%s: a buffer one element short was accepted\n", argv[a]);
            ++failures;
        }
        // truncations: every length near both ends, a spread in between; each in an exact-size copy, so that a read past the
        // given size is a heap overflow
        const size_t size = file.size();
        for (size_t len = 0; len < size; len += (len < 700 || len + 64 > size) ? 1 : 1 + size / 97) {
            std::vector<uint8_t> cut(file.begin(), file.begin() + len);
            rc = madtp_jpeg::entropy_decode(cut.data(), (int64_t)len, coef.data(), n_coef);
            ++runs;
            if (rc == 0) {
                printf("%s: truncated to %zu of %zu bytes, decoded as whole\n", argv[a], len, size);
                ++failures;
            } else {
                ++refused;
            }
        }
        // byte flips inside the scan (and a few in the header), one at a time
        madtp_jpeg::Header h;
        madtp_jpeg::parse_header(file.data(), (int64_t)size, h);
        uint32_t seed = 12345u + (uint32_t)size;
        for (int i = 0; i < 400; ++i) {
            std::vector<uint8_t> bad(file);
            const size_t lo = i % 8 == 0 ? 2 : (size_t)h.scan_begin;
            const size_t at = lo + lcg(seed) % (size - lo);
            bad[at] ^= (uint8_t)(1u << (lcg(seed) >> 29)) | (i % 3 == 0 ? 0xFF : 0);
            int32_t info2[MADTP_JPEG_INFO_FIELDS];
            std::vector<int16_t> out;
            if (madtp_jpeg::inspect(bad.data(), (int64_t)size, info2, q) == 0) {  // (a flipped header may change the geometry)
                out.resize((size_t)64 * info2[MADTP_JPEG_I_BLOCKS]);
                rc = madtp_jpeg::entropy_decode(bad.data(), (int64_t)size, out.data(), (int64_t)out.size());
                ++runs;
                rc == 0 ? ++decoded : ++refused;
            } else {
                ++runs, ++refused;
            }
        }
    }
    printf("%d files, %ld damaged decodes: %ld returned a code, %ld decoded; %d failures\n", argc - 1, runs, refused, decoded, failures);
    return failures ? 1 : 0;
}
