// The PNG decode as both sides run it (csrc/madtp_png.h): the chunk parser of the host stage, and the routines of the two
// kernels of png.hip - the bit reader, the canonical Huffman tables from code lengths (fixed, and dynamic through the code-length
// alphabet), the symbol loop with its window, the Adler-32 combine, the five unfilter recurrences and the sample expansion.  The
// kernel routines are __host__ __device__ text: the kernel runs them with one thread per lane, madtp_png_inflate_host /
// madtp_png_unfilter_host (and tools/png_host_check.cpp under the host compiler's sanitizers) with the lanes in a `for` loop.
//
// How the lanes of the one wave of a workgroup work together, in both routines:
//   - control is UNIFORM: every lane holds the same bit position, output position and loop counters and takes the same branches;
//     what is written to LDS from uniform code is written by the first lane only (first_lane());
//   - the cooperative parts - copying a match, storing the window, summing the checksum, the unfilter wavefront - are each_lane()
//     bodies: the kernel runs the body once with its own lane number, the host runs it for lane 0 .. 63 in turn;
//   - sync_lanes() (a barrier on the device, nothing on the host) stands between a write to LDS and a read of it by another lane.
// No allocation, no mutable static, no atomics.  Every read of a stream goes through Bits and is checked against its size; every
// write of output is checked against the image's extent before it happens.
#pragma once
#include <stdint.h>
#include <string.h>

#include "madtp_png.h"

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

namespace madtp_png {

constexpr int kLanes = MADTP_PNG_LANES, kWindow = MADTP_PNG_WINDOW, kFlush = MADTP_PNG_FLUSH, kBand = MADTP_PNG_BAND, kTile = MADTP_PNG_TILE;
constexpr int kMask = kWindow - 1;
static_assert((kWindow & kMask) == 0 && kWindow == 32768 && kFlush * 2 == kWindow, "the window of deflate, stored in halves");
static_assert(kTile % 8 == 0 && kTile % 6 == 0 && kBand == kLanes, "a tile holds whole pixels of every format; one lane per row");

#if defined(__HIP_DEVICE_COMPILE__)
constexpr int kLaneSlots = 1;  // a lane's private state is its own registers
#else
constexpr int kLaneSlots = kLanes;
#endif

template <class F>
PNG_HD void each_lane(F body) {
#if defined(__HIP_DEVICE_COMPILE__)
    body((int)threadIdx.x);
#else
    for (int lane = 0; lane < kLanes; ++lane) body(lane);
#endif
}

PNG_HD void sync_lanes() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

PNG_HD bool first_lane() {
#if defined(__HIP_DEVICE_COMPILE__)
    return threadIdx.x == 0;
#else
    return true;
#endif
}

PNG_HD int lane_slot(int lane) { return kLaneSlots == 1 ? 0 : lane; }

// ---- formats -------------------------------------------------------------------------------------------------------------------------
struct Format {
    int w, h, depth, color, channels, rowbytes, bpp;
    int64_t raw_bytes;
};

// 0, MADTP_PNG_E_HEADER (a side of 0), E_COLOR_DEPTH, E_GRAY16 or E_SIDE
PNG_HD int make_format(Format& f, int64_t w, int64_t h, int depth, int color) {
    if (w < 1 || h < 1) return MADTP_PNG_E_HEADER;
    const bool depth_ok = depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16;
    int channels = 0;
    bool pair_ok = false;
    if (color == 0) channels = 1, pair_ok = depth_ok;
    if (color == 2) channels = 3, pair_ok = depth == 8 || depth == 16;
    if (color == 3) channels = 1, pair_ok = depth_ok && depth <= 8;
    if (color == 4) channels = 2, pair_ok = depth == 8 || depth == 16;
    if (color == 6) channels = 4, pair_ok = depth == 8 || depth == 16;
    if (!pair_ok) return MADTP_PNG_E_COLOR_DEPTH;
    if ((color == 0 || color == 4) && depth == 16) return MADTP_PNG_E_GRAY16;
    if (w > MADTP_PNG_MAX_SIDE || h > MADTP_PNG_MAX_SIDE) return MADTP_PNG_E_SIDE;
    f.w = (int)w, f.h = (int)h, f.depth = depth, f.color = color, f.channels = channels;
    f.rowbytes = (int)((w * channels * depth + 7) / 8);
    f.bpp = channels * depth >= 8 ? channels * depth / 8 : 1;
    f.raw_bytes = h * (1 + (int64_t)f.rowbytes);
    return 0;
}

// ---- the bit reader -------------------------------------------------------------------------------------------------------------------
// Bits of the stream LSB first.  Bytes beyond the end read as 0 and are counted: used() > 8 * size says that the decoder went past
// the end, which every loop checks once per round (a round consumes at least one bit, so the stream's bits bound every loop).
// The stream reaches the reader through `stage`, kStage bytes of LDS that all lanes fill together from global memory whenever the
// reader leaves them (need() is called from uniform code only): a symbol then costs LDS reads, not a round trip to global memory.
constexpr int kStage = 1024;
struct Bits {
    const uint8_t* d;
    uint8_t* stage;        // bytes [staged, staged + kStage) of the stream, those beyond its end 0
    int64_t size, next;    // the next byte to load
    int64_t staged;
    uint64_t buf;
    int have;
    PNG_HD void open(const uint8_t* data, int64_t n, uint8_t* lds) { d = data, stage = lds, size = n, next = 0, staged = -kStage, buf = 0, have = 0; }
    PNG_HD void need(int n) {  // n <= 32
        if (have >= n) return;
        if (next < staged || next + 4 > staged + kStage) {
            const int64_t from = next;
            const uint8_t* src = d;
            uint8_t* dst = stage;
            const int64_t end = size;
            sync_lanes();  // (nobody still reads what is replaced)
            each_lane([&](int lane) {
                for (int i = lane; i < kStage; i += kLanes) dst[i] = from + i < end ? src[from + i] : (uint8_t)0;
            });
            sync_lanes();
            staged = from;
        }
        uint32_t v;
        memcpy(&v, stage + (next - staged), 4);
        buf |= (uint64_t)v << have;  // have <= 31 here
        next += 4, have += 32;
    }
    PNG_HD uint32_t take(int n) {  // n <= 16
        need(n);
        const uint32_t v = (uint32_t)buf & ((1u << n) - 1u);
        buf >>= n, have -= n;
        return v;
    }
    PNG_HD void to_byte() { buf >>= (have & 7), have -= (have & 7); }
    PNG_HD int64_t used() const { return 8 * next - have; }
    PNG_HD bool past_end() const { return used() > 8 * size; }
};

// ---- canonical Huffman tables ---------------------------------------------------------------------------------------------------------
struct Huff {
    uint16_t* count;   // [16]: codes of each length
    uint16_t* symbol;  // the symbols in the order of their codes
    uint16_t* fast;    // [1 << fast_bits]: the next fast_bits bits of the stream -> symbol << 4 | length, 0 for a longer code or none
    int fast_bits;
};

PNG_HD uint32_t reversed(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// lengths[0 .. n) (LDS, complete behind a sync_lanes()) -> the table: counts and symbols written by the first lane, the fast table
// by all lanes, a code each (codes are prefix-free: no two write the same entry).  Returns what is left of the code space: 0 for a
// complete code, negative for an over-subscribed one, positive for an incomplete one; only_ones: no code is longer than one bit.
// Uniform.
PNG_HD int build(const Huff& h, const uint8_t* lengths, int n, bool& only_ones) {
    int count[16], offs[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lengths[s] & 15];
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return left;
    }
    only_ones = count[1] + count[0] == n;
    if (first_lane()) {
        offs[1] = 0;
        for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l];
        for (int l = 0; l < 16; ++l) h.count[l] = (uint16_t)count[l];
        for (int s = 0; s < n; ++s)
            if (lengths[s] & 15) h.symbol[offs[lengths[s] & 15]++] = (uint16_t)s;
    }
    const int entries = 1 << h.fast_bits, codes = n - count[0];
    each_lane([&](int lane) {
        for (int i = lane; i < entries; i += kLanes) h.fast[i] = 0;
    });
    sync_lanes();
    each_lane([&](int lane) {
        for (int i = lane; i < codes; i += kLanes) {  // the i-th code in canonical order: its length, then its value
            int len = 1, start = 0;
            uint32_t first = 0;
            while (i >= start + count[len]) start += count[len], first = (first + (uint32_t)count[len]) << 1, ++len;
            if (len > h.fast_bits) break;  // (and so is every later one)
            const uint16_t entry = (uint16_t)(h.symbol[i] << 4 | len);
            for (uint32_t k = reversed(first + (uint32_t)(i - start), len); k < (uint32_t)entries; k += 1u << len) h.fast[k] = entry;
        }
    });
    sync_lanes();
    return left;
}

// one symbol, or -1 for a bit pattern that is no code (of an incomplete table).  Uniform.
PNG_HD int decode(Bits& b, const Huff& h) {
    b.need(15);
    uint32_t bits = (uint32_t)b.buf;
    const uint32_t entry = h.fast[bits & ((1u << h.fast_bits) - 1u)];
    if (entry) {
        b.buf >>= (entry & 15u), b.have -= (int)(entry & 15u);
        return (int)(entry >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int count = h.count[len];
        if (code - count < first) {
            b.buf >>= len, b.have -= len;
            return h.symbol[index + (code - first)];
        }
        index += count, first += count;
        first <<= 1, code <<= 1;
    }
    return -1;
}

// ---- Adler-32 --------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kAdlerMod = 65521u;
// (a, b) of a prefix, then a block of `len` bytes whose own sums from (0, 0) are (sa, sb): len <= 1024 keeps everything in 32 bits
PNG_HD void adler_combine(uint32_t& a, uint32_t& b, uint32_t sa, uint32_t sb, uint32_t len) {
    b = (b + len * a + sb) % kAdlerMod;
    a = (a + sa) % kAdlerMod;
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------------
constexpr int kLitFast = 10, kDistFast = 8, kCodeFast = 7;  // bits the fast tables look at (a code-length code has at most 7)
struct InflateShared {
    uint8_t win[kWindow];  // the last 32 KiB of output: byte p lives at p & kMask
    uint16_t lcount[16], lsymbol[288], dcount[16], dsymbol[32], ccount[16], csymbol[20];
    uint16_t lfast[1 << kLitFast], dfast[1 << kDistFast], cfast[1 << kCodeFast];
    uint8_t lengths[320];
    uint32_t part_a[kLanes], part_b[kLanes];
    uint8_t stage[kStage];
    int bad_filter;
};

struct Inflate {
    InflateShared* sh;
    Bits in;
    uint8_t* raw;
    int64_t expect, pos, stored;  // bytes the image takes, bytes produced, bytes of them that went to raw
    int64_t stride;               // 1 + rowbytes, 0 to leave the filter bytes unchecked
    uint32_t a, b;
    int blocks;
};

// window bytes [z.stored, z.stored + n) -> raw, with all lanes; their Adler-32 and their filter bytes.  n <= kWindow.
PNG_HD int store(Inflate& z, int n) {
    InflateShared& sh = *z.sh;
    const int64_t from = z.stored;  // a multiple of kFlush, so of 4
    uint8_t* raw = z.raw;
    int chunk = ((n + kLanes - 1) / kLanes + 3) & ~3;  // bytes of a lane's share of the checksum: whole words, an odd number of them,
    if (!(chunk & 4)) chunk += 4;                      // so that the lanes' reads fall into different LDS banks
    const int64_t stride = z.stride;
    sync_lanes();
    each_lane([&](int lane) {
        const int words = n >> 2;
        for (int i = lane; i < words; i += kLanes) {
            uint32_t v;
            memcpy(&v, &sh.win[(from + 4 * (int64_t)i) & kMask], 4);
            memcpy(raw + from + 4 * (int64_t)i, &v, 4);
        }
        for (int i = 4 * words + lane; i < n; i += kLanes) raw[from + i] = sh.win[(from + i) & kMask];
        uint32_t sa = 0, sb = 0;
        const int begin = lane * chunk, end = begin + chunk < n ? begin + chunk : n;
        for (int i = begin; i < end; ++i) {
            sa += sh.win[(from + i) & kMask];
            sb += sa;
        }
        sh.part_a[lane] = sa, sh.part_b[lane] = sb;
        if (stride > 0)
            for (int64_t r = (from + stride - 1) / stride + lane; r * stride < from + n; r += kLanes)
                if (sh.win[(r * stride) & kMask] > 4) sh.bad_filter = 1;  // (every writer writes the same value)
    });
    sync_lanes();
    for (int lane = 0; lane < kLanes; ++lane) {
        const int begin = lane * chunk;
        if (begin >= n) break;
        adler_combine(z.a, z.b, sh.part_a[lane], sh.part_b[lane], (uint32_t)(begin + chunk < n ? chunk : n - begin));
    }
    const int bad = sh.bad_filter;
    sync_lanes();  // (the partial sums are read before the next store writes them)
    z.stored += n;
    return bad ? MADTP_PNG_E_FILTER : 0;
}

PNG_HD int store_full_halves(Inflate& z) {
    while (z.pos - z.stored >= kFlush) {
        const int rc = store(z, kFlush);
        if (rc) return rc;
    }
    return 0;
}

// the base and the extra bits of length symbol s (0 .. 28) and of distance symbol d (0 .. 29), as RFC 1951 tabulates them
PNG_HD void length_of(int s, int& base, int& extra) {
    if (s < 8) base = 3 + s, extra = 0;
    else if (s == 28) base = 258, extra = 0;
    else extra = (s - 4) >> 2, base = 3 + ((4 + (s & 3)) << extra);
}
PNG_HD void distance_of(int d, int& base, int& extra) {
    if (d < 4) base = 1 + d, extra = 0;
    else extra = (d >> 1) - 1, base = 1 + ((2 + (d & 1)) << extra);
}

// the code lengths of a fixed block / of a dynamic block's header -> the two tables.  Uniform.
PNG_HD int fixed_tables(Inflate& z, const Huff& lit, const Huff& dist) {
    InflateShared& sh = *z.sh;
    each_lane([&](int lane) {
        for (int s = lane; s < 320; s += kLanes) sh.lengths[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
    });
    sync_lanes();
    bool ones;
    build(lit, sh.lengths, 288, ones);
    build(dist, sh.lengths + 288, 32, ones);  // (32 codes of 5 bits: symbols 30 and 31 are codes that stand for nothing)
    return 0;
}

PNG_HD int dynamic_tables(Inflate& z, const Huff& lit, const Huff& dist) {
    InflateShared& sh = *z.sh;
    Bits& in = z.in;
    const int nlen = (int)in.take(5) + 257, ndist = (int)in.take(5) + 1, ncode = (int)in.take(4) + 4;
    if (in.past_end()) return MADTP_PNG_E_TRUNCATED;
    if (nlen > 286 || ndist > 30) return MADTP_PNG_E_LENGTHS;
    const char* order = "\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f";
    sync_lanes();  // (the lanes have left the tables of the block before)
    each_lane([&](int lane) {
        if (lane < 19) sh.lengths[lane] = 0;
    });
    sync_lanes();
    for (int i = 0; i < ncode; ++i) {
        const uint32_t len = in.take(3);
        if (first_lane()) sh.lengths[(int)order[i]] = (uint8_t)len;
    }
    if (in.past_end()) return MADTP_PNG_E_TRUNCATED;
    sync_lanes();
    const Huff code = {sh.ccount, sh.csymbol, sh.cfast, kCodeFast};
    bool ones;
    if (build(code, sh.lengths, 19, ones) != 0) return MADTP_PNG_E_LENGTHS;  // zlib wants this one complete
    int index = 0, prev = 0;
    while (index < nlen + ndist) {
        if (in.past_end()) return MADTP_PNG_E_TRUNCATED;
        const int sym = decode(in, code);
        if (sym < 0) return MADTP_PNG_E_SYMBOL;
        int repeat = 1, len = sym;
        if (sym == 16) {
            if (index == 0) return MADTP_PNG_E_LENGTHS;
            len = prev, repeat = 3 + (int)in.take(2);
        } else if (sym == 17) {
            len = 0, repeat = 3 + (int)in.take(3);
        } else if (sym == 18) {
            len = 0, repeat = 11 + (int)in.take(7);
        }
        if (index + repeat > nlen + ndist) return MADTP_PNG_E_LENGTHS;
        // one list for both alphabets: a repeat runs across the boundary between them
        if (first_lane())
            for (int k = 0; k < repeat; ++k) sh.lengths[index + k] = (uint8_t)len;
        index += repeat, prev = len;
    }
    if (in.past_end()) return MADTP_PNG_E_TRUNCATED;
    sync_lanes();
    if (sh.lengths[256] == 0) return MADTP_PNG_E_LENGTHS;  // no end-of-block code
    // zlib's rule: an incomplete set is refused unless all it holds is codes of one bit (or, for distances, nothing)
    int left = build(lit, sh.lengths, nlen, ones);
    if (left < 0 || (left > 0 && !ones)) return MADTP_PNG_E_LENGTHS;
    left = build(dist, sh.lengths + nlen, ndist, ones);
    if (left < 0 || (left > 0 && !ones)) return MADTP_PNG_E_LENGTHS;
    return 0;
}

// len bytes from `dist` back -> the window at z.pos.  With dist < len the match overlaps its own output: byte k is byte k % dist of
// the dist bytes before z.pos, all of which exist before the copy begins.  With dist >= len a source lies less than len bytes
// ahead of its target in the ring only when dist > kWindow - len, and then at most kLanes - 1 + (kWindow - dist) targets ahead of
// the one being written: a chunk of kLanes bytes reads before it writes (one wave, one instruction after the other; lanes in
// ascending order on the host), and a later chunk's sources are never a written target.
PNG_HD void copy_match(InflateShared& sh, int64_t pos, int dist, int len) {
    sync_lanes();
    for (int base = 0; base < len; base += kLanes)
        each_lane([&](int lane) {
            const int k = base + lane;
            if (k < len) sh.win[(pos + k) & kMask] = sh.win[(pos - dist + (dist >= len ? k : k % dist)) & kMask];
        });
    sync_lanes();
}

// One zlib stream -> raw[0 .. expect): returns the code, fills status.  sh: the workgroup's LDS (the host's stack).
PNG_HD int inflate_image(InflateShared& sh, const uint8_t* stream, int64_t stream_bytes, uint8_t* raw, int64_t expect, int rowbytes,
                         int32_t* status) {
    Inflate z;
    z.sh = &sh, z.raw = raw, z.expect = expect, z.pos = 0, z.stored = 0, z.stride = rowbytes > 0 ? 1 + (int64_t)rowbytes : 0;
    z.a = 1, z.b = 0, z.blocks = 0;
    z.in.open(stream, stream_bytes, sh.stage);
    Bits& in = z.in;
    const Huff lit = {sh.lcount, sh.lsymbol, sh.lfast, kLitFast}, dist = {sh.dcount, sh.dsymbol, sh.dfast, kDistFast};
    if (first_lane()) sh.bad_filter = 0;
    sync_lanes();
    int rc = 0;
    {
        const uint32_t cmf = in.take(8), flg = in.take(8);
        if (in.past_end()) rc = MADTP_PNG_E_TRUNCATED;
        else if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u) rc = MADTP_PNG_E_ZLIB_HEADER;
        else if (flg & 0x20u) rc = MADTP_PNG_E_DICT;
    }
    bool last = false;
    while (!rc && !last) {
        last = in.take(1) != 0;
        const uint32_t type = in.take(2);
        if (in.past_end()) { rc = MADTP_PNG_E_TRUNCATED; break; }
        ++z.blocks;
        if (type == 3) { rc = MADTP_PNG_E_BLOCK_TYPE; break; }
        if (type == 0) {
            in.to_byte();
            const uint32_t len = in.take(16), nlen = in.take(16);
            if (in.past_end()) { rc = MADTP_PNG_E_TRUNCATED; break; }
            if ((len ^ 0xffffu) != nlen) { rc = MADTP_PNG_E_STORED; break; }
            const int64_t at = in.next - in.have / 8;  // the bit buffer holds whole bytes here
            if (at + len > in.size) { rc = MADTP_PNG_E_TRUNCATED; break; }
            if (z.pos + len > expect) { rc = MADTP_PNG_E_SIZE; break; }
            for (uint32_t done = 0; done < len && !rc;) {
                const int n = (int)(len - done < (uint32_t)kFlush ? len - done : (uint32_t)kFlush);
                const uint8_t* src = in.d + at + done;
                const int64_t pos = z.pos;
                sync_lanes();
                each_lane([&](int lane) {
                    for (int k = lane; k < n; k += kLanes) sh.win[(pos + k) & kMask] = src[k];
                });
                z.pos += n, done += n;
                rc = store_full_halves(z);
            }
            in.next = at + len, in.buf = 0, in.have = 0;
            continue;
        }
        rc = type == 1 ? fixed_tables(z, lit, dist) : dynamic_tables(z, lit, dist);
        while (!rc) {
            if (in.past_end()) { rc = MADTP_PNG_E_TRUNCATED; break; }
            int sym = decode(in, lit);
            if (sym < 0) { rc = MADTP_PNG_E_SYMBOL; break; }
            if (sym == 256) break;
            if (sym < 256) {
                if (z.pos >= expect) { rc = MADTP_PNG_E_SIZE; break; }
                if (first_lane()) sh.win[z.pos & kMask] = (uint8_t)sym;
                ++z.pos;
            } else {
                sym -= 257;
                if (sym >= 29) { rc = MADTP_PNG_E_SYMBOL; break; }
                int base, extra;
                length_of(sym, base, extra);
                const int len = base + (int)in.take(extra);
                const int dsym = decode(in, dist);
                if (dsym < 0 || dsym >= 30) { rc = MADTP_PNG_E_SYMBOL; break; }
                distance_of(dsym, base, extra);
                const int d = base + (int)in.take(extra);
                if (in.past_end()) { rc = MADTP_PNG_E_TRUNCATED; break; }
                if (d > z.pos) { rc = MADTP_PNG_E_DISTANCE; break; }
                if (z.pos + len > expect) { rc = MADTP_PNG_E_SIZE; break; }
                copy_match(sh, z.pos, d, len);
                z.pos += len;
            }
            if (z.pos - z.stored >= kFlush) rc = store_full_halves(z);
        }
    }
    if (!rc && z.pos > z.stored) rc = store(z, (int)(z.pos - z.stored));
    if (!rc && z.pos != expect) rc = MADTP_PNG_E_SIZE;
    if (!rc) {
        in.to_byte();
        uint32_t want = 0;
        for (int i = 0; i < 4; ++i) want = want << 8 | in.take(8);
        if (in.past_end()) rc = MADTP_PNG_E_TRUNCATED;
        else if (want != (z.b << 16 | z.a)) rc = MADTP_PNG_E_ADLER;
    }
    if (first_lane()) {
        status[MADTP_PNG_S_CODE] = rc, status[MADTP_PNG_S_BLOCKS] = z.blocks;
        status[MADTP_PNG_S_BYTES] = (int32_t)z.stored, status[MADTP_PNG_S_ADLER] = (int32_t)(z.b << 16 | z.a);
    }
    return rc;
}

// ---- unfilter and expansion -------------------------------------------------------------------------------------------------------------
// the value a filter adds to the filtered byte: a left, b above, c above left (PNG specification, 9.2 - 9.4)
PNG_HD int predict(int filter, int a, int b, int c) {
    if (filter == 1) return a;
    if (filter == 2) return b;
    if (filter == 3) return (a + b) >> 1;
    if (filter == 4) {
        const int p = a + b - c;
        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
    }
    return 0;
}

// pixel p of an unfiltered row segment that begins at a pixel boundary -> Pillow's convert('RGB') of it
PNG_HD void expand(const Format& f, const uint8_t* row, int p, const uint8_t* palette, uint8_t& r, uint8_t& g, uint8_t& b) {
    if (f.color == 2 || f.color == 6) {  // RGB(A): the high byte of a 16-bit sample
        const int step = f.depth >> 3;
        const uint8_t* s = row + p * f.channels * step;
        r = s[0], g = s[step], b = s[2 * step];
        return;
    }
    int v;
    if (f.depth == 8) {
        v = row[p * f.channels];  // gray, gray + alpha, palette
    } else {  // 1, 2, 4 bits: the leftmost pixel in the high bits
        const int per = 8 / f.depth, k = p % per;
        v = (row[p / per] >> (8 - f.depth * (k + 1))) & ((1 << f.depth) - 1);
    }
    if (f.color == 3) {
        r = palette[3 * v], g = palette[3 * v + 1], b = palette[3 * v + 2];
    } else {
        if (f.depth < 8) v *= 255 / ((1 << f.depth) - 1);  // 255, 85, 17
        r = g = b = (uint8_t)v;
    }
}

struct UnfilterShared {
    uint8_t tile[kBand][kTile + 4];
    uint8_t up[kTile];  // the unfiltered row above the band, this tile's bytes of it
    uint8_t filter[kBand];
};

// raw (f.raw_bytes, not modified) -> out (3 * w * h).  carry: 16 bytes per row, each written and read back by the lane of that row.
// Tiles of kTile bytes from left to right, in each the bands of kBand rows from top to bottom: what crosses from a band to the
// next is one row of the tile (LDS), what crosses from a tile to the next is a pixel per row (left, and above left: the lane's own).
PNG_HD void unfilter_image(UnfilterShared& sh, const Format& f, const uint8_t* raw, const uint8_t* palette, uint8_t* out, uint8_t* carry) {
    const int64_t stride = 1 + (int64_t)f.rowbytes;
    const int bits = f.depth * f.channels, bpp = f.bpp;
    uint64_t left[kLaneSlots], above_left[kLaneSlots];
    for (int x0 = 0; x0 < f.rowbytes; x0 += kTile) {
        const int tb = f.rowbytes - x0 < kTile ? f.rowbytes - x0 : kTile;
        const int units = (tb + bpp - 1) / bpp;
        const int px0 = (int)((int64_t)x0 * 8 / bits);
        const int npx = f.w - px0 < kTile * 8 / bits ? f.w - px0 : kTile * 8 / bits;
        const bool more = x0 + kTile < f.rowbytes;
        sync_lanes();
        each_lane([&](int lane) {
            for (int i = lane; i < kTile; i += kLanes) sh.up[i] = 0;
        });
        for (int y0 = 0; y0 < f.h; y0 += kBand) {
            const int rows = f.h - y0 < kBand ? f.h - y0 : kBand;
            sync_lanes();
            each_lane([&](int lane) {
                for (int r = 0; r < rows; ++r) {
                    const uint8_t* src = raw + (y0 + r) * stride + 1 + x0;
                    for (int i = lane; i < tb; i += kLanes) sh.tile[r][i] = src[i];
                }
                const int s = lane_slot(lane);
                left[s] = above_left[s] = 0;
                if (lane < rows) {
                    const uint8_t ft = raw[(y0 + lane) * stride];
                    sh.filter[lane] = ft > 4 ? 0 : ft;
                    if (x0 > 0) {
                        memcpy(&left[s], carry + 16 * (int64_t)(y0 + lane), 8);
                        memcpy(&above_left[s], carry + 16 * (int64_t)(y0 + lane) + 8, 8);
                    }
                }
            });
            sync_lanes();
            // the skewed wavefront: at step t lane r is at unit t - r, one behind the lane above, whose byte above it is in LDS
            for (int t = 0; t < units + rows - 1; ++t) {
                each_lane([&](int lane) {
                    const int u = t - lane;
                    if (lane >= rows || u < 0 || u >= units) return;
                    const int s = lane_slot(lane), ft = sh.filter[lane];
                    const uint8_t* upper = lane ? sh.tile[lane - 1] : sh.up;
                    uint64_t a = left[s], c = above_left[s], na = 0, nc = 0;
                    for (int j = 0; j < bpp; ++j) {
                        const int at = u * bpp + j;
                        if (at >= tb) break;
                        const int b = upper[at];
                        const int v = (sh.tile[lane][at] + predict(ft, (int)(a >> (8 * j)) & 255, b, (int)(c >> (8 * j)) & 255)) & 255;
                        sh.tile[lane][at] = (uint8_t)v;
                        na |= (uint64_t)v << (8 * j), nc |= (uint64_t)b << (8 * j);
                    }
                    left[s] = na, above_left[s] = nc;
                });
                sync_lanes();
            }
            each_lane([&](int lane) {
                const int s = lane_slot(lane);
                if (more && lane < rows) {
                    memcpy(carry + 16 * (int64_t)(y0 + lane), &left[s], 8);
                    memcpy(carry + 16 * (int64_t)(y0 + lane) + 8, &above_left[s], 8);
                }
                for (int i = lane; i < tb; i += kLanes) sh.up[i] = sh.tile[rows - 1][i];
                for (int r = 0; r < rows; ++r) {
                    uint8_t* dst = out + ((int64_t)(y0 + r) * f.w + px0) * 3;
                    for (int p = lane; p < npx; p += kLanes) expand(f, sh.tile[r], p, palette, dst[3 * p], dst[3 * p + 1], dst[3 * p + 2]);
                }
            });
        }
    }
}

// ---- the host stage: chunks ------------------------------------------------------------------------------------------------------------
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

inline const char* strerror_png(int code) {
    switch (code) {
        case MADTP_PNG_E_INTERLACE: return "Adam7 interlace";
        case MADTP_PNG_E_GRAY16: return "16-bit gray or gray + alpha";
        case MADTP_PNG_E_APNG: return "an animation (APNG frames beyond the default image)";
        case MADTP_PNG_E_SIDE: return "a side over 8192";
        case MADTP_PNG_E_COLOR_DEPTH: return "a colour type / bit depth pair the PNG specification forbids";
        case MADTP_PNG_E_SIGNATURE: return "not a PNG signature";
        case MADTP_PNG_E_NO_IHDR: return "the first chunk is not IHDR";
        case MADTP_PNG_E_NO_PLTE: return "a palette image without PLTE";
        case MADTP_PNG_E_NO_IDAT: return "no IDAT chunk";
        case MADTP_PNG_E_CHUNK: return "a chunk runs past the end of the data, or IEND is missing";
        case MADTP_PNG_E_HEADER: return "IHDR or PLTE with impossible content";
        case MADTP_PNG_E_IDAT_ORDER: return "IDAT chunks that are not consecutive";
        case MADTP_PNG_E_ZLIB_HEADER: return "a zlib header that is not deflate with a window of at most 32 KiB";
        case MADTP_PNG_E_DICT: return "a zlib preset dictionary";
        case MADTP_PNG_E_BLOCK_TYPE: return "an invalid deflate block type";
        case MADTP_PNG_E_STORED: return "a stored block whose LEN and NLEN disagree";
        case MADTP_PNG_E_LENGTHS: return "an invalid set of code lengths";
        case MADTP_PNG_E_SYMBOL: return "a bit pattern that is no code";
        case MADTP_PNG_E_DISTANCE: return "a distance beyond the bytes produced so far";
        case MADTP_PNG_E_SIZE: return "the stream does not hold exactly the image's scanlines";
        case MADTP_PNG_E_TRUNCATED: return "the stream ends before its final block and checksum";
        case MADTP_PNG_E_ADLER: return "an Adler-32 mismatch";
        case MADTP_PNG_E_FILTER: return "a filter byte above 4";
    }
    return nullptr;
}

inline int prepare(const uint8_t* d, int64_t size, int32_t* info, uint8_t* palette, uint8_t* stream, int64_t capacity) {
    static const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < MADTP_PNG_INFO_FIELDS; ++i) info[i] = 0;
    memset(palette, 0, 768);
    if (size < 8 || memcmp(d, kSignature, 8) != 0) return MADTP_PNG_E_SIGNATURE;
    Format f = {};
    bool have_ihdr = false, have_plte = false, in_idat = false, idat_over = false, ended = false;
    int64_t total = 0, first_idat = 0;
    int entries = 0;
    for (int64_t at = 8; !ended;) {
        if (size - at < 12) return MADTP_PNG_E_CHUNK;
        const int64_t len = be32(d + at);
        if (len > 0x7fffffff || len > size - at - 12) return MADTP_PNG_E_CHUNK;
        const uint8_t* type = d + at + 4;
        const uint8_t* body = d + at + 8;
        const bool idat = memcmp(type, "IDAT", 4) == 0;
        if (!have_ihdr) {
            if (memcmp(type, "IHDR", 4) != 0 || len != 13) return MADTP_PNG_E_NO_IHDR;
            if (body[10] != 0 || body[11] != 0 || body[12] > 1) return MADTP_PNG_E_HEADER;
            const int rc = make_format(f, be32(body), be32(body + 4), body[8], body[9]);
            if (rc) return rc;
            if (body[12] == 1) return MADTP_PNG_E_INTERLACE;
            have_ihdr = true;
        } else if (memcmp(type, "IHDR", 4) == 0) {
            return MADTP_PNG_E_HEADER;
        } else if (memcmp(type, "PLTE", 4) == 0) {
            if (len == 0 || len % 3 || len > 768 || have_plte || in_idat) return MADTP_PNG_E_HEADER;
            have_plte = true;
            if (f.color == 3) {
                entries = (int)(len / 3);
                memcpy(palette, body, (size_t)len);
            }
        } else if (idat) {
            if (f.color == 3 && !have_plte) return MADTP_PNG_E_NO_PLTE;
            if (idat_over) return MADTP_PNG_E_IDAT_ORDER;
            if (!in_idat) first_idat = at;
            in_idat = true;
            total += len;
        } else if (memcmp(type, "acTL", 4) == 0) {
            if (len >= 4 && be32(body) > 1) return MADTP_PNG_E_APNG;
        } else if (memcmp(type, "fdAT", 4) == 0) {
            return MADTP_PNG_E_APNG;
        } else if (memcmp(type, "IEND", 4) == 0) {
            ended = true;
        }
        if (in_idat && !idat) idat_over = true;
        at += 12 + len;
    }
    if (f.color == 3 && !have_plte) return MADTP_PNG_E_NO_PLTE;
    if (!in_idat) return MADTP_PNG_E_NO_IDAT;
    if (total > 0x7fffffff) return MADTP_PNG_E_CHUNK;
    info[MADTP_PNG_I_WIDTH] = f.w, info[MADTP_PNG_I_HEIGHT] = f.h, info[MADTP_PNG_I_DEPTH] = f.depth, info[MADTP_PNG_I_COLOR] = f.color;
    info[MADTP_PNG_I_CHANNELS] = f.channels, info[MADTP_PNG_I_ROWBYTES] = f.rowbytes, info[MADTP_PNG_I_BPP] = f.bpp;
    info[MADTP_PNG_I_RAW_BYTES] = (int32_t)f.raw_bytes, info[MADTP_PNG_I_STREAM_BYTES] = (int32_t)total, info[MADTP_PNG_I_PALETTE] = entries;
    if (!stream) return 0;
    if (capacity < total) return MADTP_E_BADARG;
    int64_t to = 0;
    for (int64_t at = first_idat; to < total;) {  // the IDAT chunks stand one behind the other from first_idat on
        const int64_t len = be32(d + at);
        memcpy(stream + to, d + at + 8, (size_t)len);
        to += len, at += 12 + len;
    }
    return 0;
}

inline int inflate_host(const uint8_t* stream, int64_t stream_bytes, uint8_t* raw, int64_t raw_bytes, int rowbytes, int32_t* status) {
    if (!stream || !raw || !status || stream_bytes < 0 || stream_bytes > 0x7fffffff || raw_bytes < 1 || raw_bytes > 0x7fffffff) return MADTP_E_BADARG;
    InflateShared sh;
    return inflate_image(sh, stream, stream_bytes, raw, raw_bytes, rowbytes, status);
}

// carry: 16 * h bytes of scratch
inline int unfilter_host(const uint8_t* raw, int w, int h, int depth, int color, const uint8_t* palette, uint8_t* out, uint8_t* carry) {
    Format f;
    if (!raw || !palette || !out || !carry || make_format(f, w, h, depth, color) != 0) return MADTP_E_BADARG;
    for (int r = 0; r < h; ++r)
        if (raw[r * (1 + (int64_t)f.rowbytes)] > 4) return MADTP_PNG_E_FILTER;
    UnfilterShared sh;
    unfilter_image(sh, f, raw, palette, out, carry);
    return 0;
}

}  // namespace madtp_png
