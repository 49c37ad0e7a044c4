// Stand-alone check of the host stage of the PNG decode and of the host emulation of its two kernels (madtp_amd/csrc/png_device.h)
// under the host compiler's sanitizers:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/png_host_check.cpp -o png_host_check
//     ./png_host_check DIR/*.png          (python tools/make_png_golden.py --dump DIR writes the corpus)
//
// Every file is prepared, inflated and unfiltered into heap buffers of exactly the sizes prepare() reports (a write past one is the
// sanitizer's to catch), then the file is prepared again truncated at every length near both ends and a spread between, its stream
// is inflated truncated likewise (each in an exact-size copy, so that a read past the given size is a heap overflow), and both are
// run with bits flipped at seeded positions.  A whole file must decode; a truncated one must never; a damaged one must return a
// code or decode.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../madtp_amd/csrc/png_device.h"

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
        int32_t info[MADTP_PNG_INFO_FIELDS], status[MADTP_PNG_STATUS_FIELDS];
        uint8_t palette[768];
        int rc = madtp_png::prepare(file.data(), (int64_t)file.size(), info, palette, nullptr, 0);
        if (rc) {
            printf("%s: prepare -> %d (%s)\n", argv[a], rc, madtp_png::strerror_png(rc));
            ++failures;
            continue;
        }
        const int w = info[MADTP_PNG_I_WIDTH], h = info[MADTP_PNG_I_HEIGHT], depth = info[MADTP_PNG_I_DEPTH], color = info[MADTP_PNG_I_COLOR];
        const int rowbytes = info[MADTP_PNG_I_ROWBYTES];
        const int64_t raw_bytes = info[MADTP_PNG_I_RAW_BYTES], stream_bytes = info[MADTP_PNG_I_STREAM_BYTES];
        std::vector<uint8_t> stream((size_t)stream_bytes), raw((size_t)raw_bytes), out((size_t)3 * w * h), carry((size_t)16 * h);
        rc = madtp_png::prepare(file.data(), (int64_t)file.size(), info, palette, stream.data(), stream_bytes);
        if (rc == 0 && stream_bytes > 0 && madtp_png::prepare(file.data(), (int64_t)file.size(), info, palette, stream.data(), stream_bytes - 1) != MADTP_E_BADARG) {
            printf("%s: a stream buffer one byte short was accepted\n", argv[a]);
            ++failures;
        }
        if (rc == 0) rc = madtp_png::inflate_host(stream.data(), stream_bytes, raw.data(), raw_bytes, rowbytes, status);
        if (rc == 0) rc = madtp_png::unfilter_host(raw.data(), w, h, depth, color, palette, out.data(), carry.data());
        if (rc) {
            printf("%s: decode -> %d (%s)\n", argv[a], rc, madtp_png::strerror_png(rc));
            ++failures;
            continue;
        }
        // truncations of the file and of the stream
        const size_t size = file.size();
        for (size_t len = 0; len < size; len += (len < 400 || len + 64 > size) ? 1 : 1 + size / 61) {
            std::vector<uint8_t> cut(file.begin(), file.begin() + len);
            ++runs;
            if (madtp_png::prepare(cut.data(), (int64_t)len, info, palette, nullptr, 0) == 0) {
                printf("%s: truncated to %zu of %zu bytes, prepared as whole\n", argv[a], len, size);
                ++failures;
            } else {
                ++refused;
            }
        }
        for (size_t len = 0; len < (size_t)stream_bytes; len += (len < 400 || len + 64 > (size_t)stream_bytes) ? 1 : 1 + stream_bytes / 61) {
            std::vector<uint8_t> cut(stream.begin(), stream.begin() + len);
            ++runs;
            if (madtp_png::inflate_host(len ? cut.data() : stream.data(), (int64_t)len, raw.data(), raw_bytes, rowbytes, status) == 0) {
                printf("%s: stream truncated to %zu of %ld bytes, inflated as whole\n", argv[a], len, (long)stream_bytes);
                ++failures;
            } else {
                ++refused;
            }
        }
        // bit flips: in the stream (the scanlines that come out are unfiltered too), and in the file
        uint32_t seed = 12345u + (uint32_t)size;
        for (int i = 0; i < 300 && stream_bytes > 0; ++i) {
            std::vector<uint8_t> bad(stream);
            for (int k = 0; k <= i % 3; ++k) bad[lcg(seed) % bad.size()] ^= (uint8_t)(1u << (lcg(seed) >> 29));
            rc = madtp_png::inflate_host(bad.data(), stream_bytes, raw.data(), raw_bytes, 0, status);
            ++runs;
            if (rc == 0) {  // whatever bytes came out, the unfilter must stay inside its buffers
                for (int r = 0; r < h; ++r) raw[(size_t)r * (1 + rowbytes)] %= 5;
                rc = madtp_png::unfilter_host(raw.data(), w, h, depth, color, palette, out.data(), carry.data());
            }
            rc == 0 ? ++decoded : ++refused;
        }
        for (int i = 0; i < 300; ++i) {
            std::vector<uint8_t> bad(file);
            bad[lcg(seed) % size] ^= (uint8_t)(1u << (lcg(seed) >> 29)) | (i % 3 == 0 ? 0xFF : 0);
            int32_t info2[MADTP_PNG_INFO_FIELDS];
            ++runs;
            if (madtp_png::prepare(bad.data(), (int64_t)size, info2, palette, nullptr, 0) != 0 || info2[MADTP_PNG_I_RAW_BYTES] > (64 << 20)) {
                ++refused;  // (a flipped header may claim a huge image: not decoded here)
                continue;
            }
            std::vector<uint8_t> s2((size_t)info2[MADTP_PNG_I_STREAM_BYTES]), r2((size_t)info2[MADTP_PNG_I_RAW_BYTES]);
            rc = madtp_png::prepare(bad.data(), (int64_t)size, info2, palette, s2.data(), (int64_t)s2.size());
            if (rc == 0) rc = madtp_png::inflate_host(s2.data(), (int64_t)s2.size(), r2.data(), (int64_t)r2.size(), info2[MADTP_PNG_I_ROWBYTES], status);
            if (rc == 0) {
                std::vector<uint8_t> o2((size_t)3 * info2[MADTP_PNG_I_WIDTH] * info2[MADTP_PNG_I_HEIGHT]), c2((size_t)16 * info2[MADTP_PNG_I_HEIGHT]);
                rc = madtp_png::unfilter_host(r2.data(), info2[MADTP_PNG_I_WIDTH], info2[MADTP_PNG_I_HEIGHT], info2[MADTP_PNG_I_DEPTH],
                                              info2[MADTP_PNG_I_COLOR], palette, o2.data(), c2.data());
            }
            rc == 0 ? ++decoded : ++refused;
        }
    }
    printf("%d files, %ld damaged decodes: %ld returned a code, %ld decoded; %d failures\n", argc - 1, runs, refused, decoded, failures);
    return failures ? 1 : 0;
}
