// The Huffman entropy stage of the JPEG decode as one lane runs it (include/madtp_jhuff.h): the bit reader, one symbol, one block
// step, the state compare, and the phases of an image written per lane.  Everything a lane does is a __host__ __device__ function,
// so the text the kernel of jpeg_huff.hip runs with one thread per lane is the text decode_image_host runs with the lanes in a
// `for` loop (madtp_jhuff_decode_host, tools/jhuff_host_check.cpp under the host compiler's sanitizers).  No allocation, no mutable
// static.  Every read of the file goes through Reader and is checked against the file's size, every write of a coefficient through
// block_of and is checked against the image's blocks.
//
// A lane's state between two symbols is (bit position, block of the MCU, zigzag index): pos = 8 * byte + bit, where `byte` is the
// file offset of the byte that holds the next unread bit - never the 00 of a stuffed FF 00 pair - and with bit = 0 the next byte to
// load, which may be a marker.  A state with block 0 and index 0 stands BEHIND whatever marker the MCU boundary held: the lane that
// completes a MCU's last block deals with the marker, the lane that starts there does not look again.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/madtp_jhuff.h"
#include "jpeg_entropy.h"

#if defined(__HIPCC__)
#define JH_HD __host__ __device__ inline
#else
#define JH_HD inline
#endif

namespace madtp_jhuff {

constexpr int kLookBits = 9;
constexpr int kLanes = MADTP_JHUFF_LANES;
constexpr uint32_t kNoBoundary = 0xffffffffu;
constexpr uint16_t kTerminal = 0xffffu;  // in place of 64 * block + index: the lane ended in a code, no state follows it

struct Table {
    uint16_t look[1 << kLookBits];
    int32_t maxcode[18];
    int32_t valoffset[18];
    uint8_t vals[256];
};
static_assert(sizeof(Table) == MADTP_JHUFF_TABLE_BYTES && 6 * sizeof(Table) == MADTP_JHUFF_RECORD_BYTES, "the record of the header");

// what a table row says of an image, checked
struct Image {
    const uint8_t* d;
    const uint8_t* zz;  // madtp_jpeg::kZigzagToColumnMajor where the lane can read it
    int64_t size, scan;
    int components, hs, vs, bx, by, restart;
    int bpm, mcus_x, chroma_x;  // blocks per MCU
    int64_t mcus, luma, chroma, blocks;
    int subseq, lanes;  // bytes per subsequence, subsequences
};

JH_HD int default_subseq(int64_t scan_bytes) {
    if (scan_bytes < 0) return 0;
    const int64_t per = (scan_bytes + kLanes - 1) / kLanes;
    const int64_t s = (per + 3) / 4 * 4;
    return (int)(s < 32 ? 32 : s);
}

// -> false for fields that contradict each other or the limits of the header
JH_HD bool make_image(Image& im, const uint8_t* d, int64_t size, int64_t scan, int components, int hs, int vs, int bx, int by, int restart,
                      int subseq_bytes) {
    if (size < 0 || size > MADTP_JHUFF_MAX_BYTES || scan < 0 || scan > size) return false;
    if (components != 1 && components != 3) return false;
    if (!((hs == 1 && vs == 1) || (components == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
    const int most = MADTP_JPEG_MAX_SIDE / 8 + 1;
    if (bx < 1 || by < 1 || bx > most || by > most || bx % hs || by % vs || restart < 0 || restart > 65535) return false;
    if (subseq_bytes < 0 || (subseq_bytes & 3)) return false;
    im.d = d, im.zz = nullptr, im.size = size, im.scan = scan;
    im.components = components, im.hs = hs, im.vs = vs, im.bx = bx, im.by = by, im.restart = restart;
    im.bpm = components == 1 ? 1 : hs * vs + 2;
    im.mcus_x = bx / hs, im.chroma_x = bx / hs;
    im.mcus = (int64_t)(bx / hs) * (by / vs);
    im.luma = (int64_t)bx * by;
    im.chroma = components == 1 ? 0 : im.luma / (hs * vs);
    im.blocks = im.luma + 2 * im.chroma;
    im.subseq = subseq_bytes ? subseq_bytes : default_subseq(size - scan);
    const int64_t n = (size - scan + im.subseq - 1) / im.subseq;
    im.lanes = (int)(n < 1 ? 1 : n);
    return true;
}

// element offset of block n (in scan order) within the image's coefficients, -1 beyond the image
JH_HD int64_t block_of(const Image& im, int64_t n) {
    if (n < 0 || n >= im.blocks) return -1;
    const int64_t mcu = n / im.bpm;
    const int j = (int)(n - mcu * im.bpm);
    const int64_t my = mcu / im.mcus_x, mx = mcu - my * im.mcus_x;
    int64_t k;
    if (j < im.hs * im.vs) {
        const int v = j / im.hs, u = j - v * im.hs;
        k = (my * im.vs + v) * im.bx + (mx * im.hs + u);
    } else {
        k = im.luma + (j - im.hs * im.vs) * im.chroma + my * im.chroma_x + mx;
    }
    return k < im.blocks ? 64 * k : -1;
}

// ---- the bit reader: madtp_jpeg::BitReader's semantics over file offsets ----------------------------------------------------------
// acc holds n bits, the next one highest.  At a marker or the end of the data it goes on with zero bits and counts them in pad.
struct Reader {
    const uint8_t* d;
    int64_t end, p, lo;  // file size; next byte to load; first byte loaded since the start or the last marker
    uint64_t acc;
    int n, pad;

    JH_HD void start(const uint8_t* data, int64_t size, uint32_t pos) {
        d = data, end = size, p = lo = (int64_t)(pos >> 3), acc = 0, n = 0, pad = 0;
        fill();
        n -= (int)(pos & 7);
    }
    JH_HD void fill() {
        while (n <= 56) {
            unsigned b = 0;
            if (p < end && d[p] != 0xFF) {
                b = d[p++];
            } else if (p + 1 < end && d[p + 1] == 0x00) {  // (here d[p] is FF) a stuffed FF
                b = 0xFF;
                p += 2;
            } else {  // a marker, or the end: stay in front of it
                pad += 8;
            }
            acc = acc << 8 | b;
            n += 8;
        }
    }
    JH_HD unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    JH_HD void restart_at(int64_t byte) { acc = 0, n = 0, pad = 0, p = lo = byte; }
    // the state's position; the caller has made sure of n >= pad
    JH_HD uint32_t position() const {
        const int r = n - pad;  // real bits loaded and not read
        const int steps = (r + 7) >> 3;
        int64_t q = p;
        for (int i = 0; i < steps && q > lo; ++i) {
            --q;
            if (q > lo && d[q] == 0x00 && d[q - 1] == 0xFF) --q;  // the reader only ever passed an FF together with its 00
        }
        return (uint32_t)(q * 8 + (steps * 8 - r));
    }
};

// one symbol; the caller has made sure of 16 bits.  -> symbol, or -1 for a pattern that is no code
JH_HD int decode_symbol(Reader& br, const Table& t) {
    const unsigned e = t.look[br.peek(kLookBits)];
    if (e) {
        br.n -= (int)(e >> 8);
        return (int)(e & 255);
    }
    const int32_t code16 = (int32_t)br.peek(16);
    for (int len = kLookBits + 1; len <= 16; ++len) {
        const int32_t code = code16 >> (16 - len);
        if (code <= t.maxcode[len]) {
            br.n -= len;
            return t.vals[(code + t.valoffset[len]) & 255];
        }
    }
    return -1;
}

JH_HD int receive_extend(Reader& br, int s) {  // s in 1 .. 15
    const int v = (int)br.peek(s);
    br.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// madtp_jpeg::next_marker: the marker that must stand at the reader's position once the buffered bits are dropped
JH_HD int next_marker(Reader& br, int extra_code) {
    if (br.n < br.pad) return MADTP_JPEG_E_TRUNCATED;
    if (br.n - br.pad >= 8) return extra_code;
    int64_t q = br.p;
    br.restart_at(q);
    if (q >= br.end) return MADTP_JPEG_E_TRUNCATED;
    if (br.d[q] != 0xFF) return extra_code;
    while (q < br.end && br.d[q] == 0xFF) ++q;
    if (q >= br.end) {
        br.restart_at(q);
        return MADTP_JPEG_E_TRUNCATED;
    }
    const int m = br.d[q];
    br.restart_at(q + 1);
    return m;
}

// a lane that does not know its MCU number takes a restart marker wherever one stands behind a whole MCU
JH_HD void take_restart_marker(Reader& br) {
    const int r = br.n - br.pad;
    if (r < 0 || r >= 8) return;
    int64_t q = br.p;
    if (q >= br.end || br.d[q] != 0xFF) return;
    while (q < br.end && br.d[q] == 0xFF) ++q;
    if (q < br.end && br.d[q] >= 0xD0 && br.d[q] <= 0xD7) br.restart_at(q + 1);
}

struct LaneEnd {
    uint32_t pos;   // the end state, if bk != kTerminal
    uint16_t bk;    // 64 * block of the MCU + zigzag index, or kTerminal
    uint32_t count; // blocks completed
    int code;       // of a terminal lane: 0 (the scan ended as it must) or a MADTP_JPEG_E_*
};

// One lane: decode from the state (pos, bk) up to the first symbol that begins at or beyond `boundary`, or to a code.
//   first_block < 0   the lane does not know where in the image it is: it takes restart markers where it finds them, writes nothing
//                     and its codes mean only "no state follows"
//   first_block >= 0  number of blocks completed in front of the state: the host decoder's rules, coefficients written to coef (DC
//                     values as differences)
// The loop is bounded by the bits between the state and the boundary: every symbol takes at least one bit, and a reader that has
// run into padding ends with the block it is in.
JH_HD LaneEnd lane_run(const Image& im, const Table* tab, uint32_t pos, uint16_t bk, int64_t first_block, uint32_t boundary, int16_t* coef) {
    LaneEnd out;
    out.pos = pos, out.bk = kTerminal, out.count = 0, out.code = MADTP_JPEG_E_TRUNCATED;
    const bool exact = first_block >= 0;
    int b = bk >> 6, k = bk & 63;
    if (b >= im.bpm) return out;
    const int64_t last_bit = 8 * im.size;
    const int64_t stop = (int64_t)boundary < last_bit ? (int64_t)boundary : last_bit;
    const int64_t limit = (stop > (int64_t)pos ? stop - (int64_t)pos : 0) + 160;
    Reader br;
    br.start(im.d, im.size, pos);
    int64_t at = exact && k > 0 ? block_of(im, first_block) : -1;  // the block being written
    for (int64_t it = 0; it < limit; ++it) {
        if ((uint64_t)br.p * 8 >= boundary && br.n >= br.pad) {
            const uint32_t here = br.position();
            if (here >= boundary) {
                out.pos = here, out.bk = (uint16_t)(b << 6 | k), out.code = 0;
                return out;
            }
        }
        if (br.n < 32) br.fill();
        const int comp = b < im.hs * im.vs ? 0 : b - im.hs * im.vs + 1;
        bool done = false;
        if (k == 0) {
            const int s = decode_symbol(br, tab[2 * comp]);
            if (s < 0 || s > 15) {
                out.code = MADTP_JPEG_E_CODE;
                return out;
            }
            const int diff = s ? receive_extend(br, s) : 0;
            if (exact) {
                at = block_of(im, first_block + out.count);
                if (at >= 0 && coef) coef[at] = (int16_t)diff;
            }
            k = 1;
        } else {
            const int rs = decode_symbol(br, tab[2 * comp + 1]);
            if (rs < 0) {
                out.code = MADTP_JPEG_E_CODE;
                return out;
            }
            const int r = rs >> 4, s = rs & 15;
            if (s) {
                k += r;
                if (k > 63) {
                    out.code = MADTP_JPEG_E_INDEX;
                    return out;
                }
                const int v = receive_extend(br, s);
                if (at >= 0 && coef) coef[at + im.zz[k]] = (int16_t)v;
                ++k;
                done = k > 63;
            } else if (r == 15) {
                k += 16;
                if (k > 63) {
                    out.code = MADTP_JPEG_E_INDEX;
                    return out;
                }
            } else if (r == 0) {
                done = true;
            } else {
                out.code = MADTP_JPEG_E_CODE;
                return out;
            }
        }
        if (!done) continue;
        if (br.n < br.pad) {
            out.code = MADTP_JPEG_E_TRUNCATED;
            return out;
        }
        ++out.count, k = 0, at = -1;
        if (++b < im.bpm) continue;
        b = 0;  // a whole MCU: the marker that may stand here is this lane's
        if (!exact) {
            if (im.restart) take_restart_marker(br);
            continue;
        }
        const int64_t n = first_block + out.count;
        if (n >= im.blocks) {
            const int m = next_marker(br, MADTP_JPEG_E_MARKER);
            out.code = m < 0 ? m : m == 0xD9 ? 0 : (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD) ? MADTP_JPEG_E_SCANS
                       : m == 0xDC ? MADTP_JPEG_E_DNL : MADTP_JPEG_E_MARKER;
            return out;
        }
        const int64_t mcu = n / im.bpm;
        if (im.restart && mcu % im.restart == 0) {
            const int m = next_marker(br, MADTP_JPEG_E_RESTART);
            if (m < 0 || m != 0xD0 + (int)((mcu / im.restart - 1) & 7)) {
                out.code = m < 0 ? m : MADTP_JPEG_E_RESTART;
                return out;
            }
        }
    }
    return out;  // (not reached by the bound's argument; a code, not a state, if it were)
}

// ---- an image, phase by phase; every phase is one call per lane with all lanes of the phase before finished -----------------------
struct DcSum {
    uint32_t s[3];
    uint32_t cut;  // a restart interval began inside
};

struct Shared {
    Table tab[6];
    union {
        struct {
            uint32_t spos[kLanes], epos[kLanes], tpos[kLanes], count[kLanes], xpos[kLanes], xcount[kLanes];
            uint32_t sum[2][kLanes];
            int xcode[kLanes];
            uint16_t sbk[kLanes], ebk[kLanes], tbk[kLanes], xbk[kLanes];
        } l;
        DcSum dc[2][kLanes];
    } u;
    int again[2];   // a lane has to decode again (two flags, used in turn)
    int first_bad;  // first lane of the round that ended in a code or whose successor started elsewhere
    // carried from round to round
    uint32_t carry_pos;
    uint16_t carry_bk;
    int64_t carry_blocks;
};

JH_HD uint32_t boundary_of(const Image& im, int64_t lane) {
    return lane + 1 >= im.lanes ? kNoBoundary : (uint32_t)((im.scan + (lane + 1) * im.subseq) * 8);
}

// step 1: lane j of the round that begins at subsequence g0
JH_HD void phase_first(const Image& im, Shared& sh, int64_t g0, int j) {
    uint32_t pos = sh.carry_pos;
    uint16_t bk = sh.carry_bk;
    if (j > 0) {
        int64_t q = im.scan + (g0 + j) * im.subseq;
        if (q < im.size && q > im.scan && im.d[q] == 0x00 && im.d[q - 1] == 0xFF) ++q;  // the 00 of a stuffed pair holds no bit
        pos = (uint32_t)(q * 8), bk = 0;
    }
    const LaneEnd e = lane_run(im, sh.tab, pos, bk, -1, boundary_of(im, g0 + j), nullptr);
    sh.u.l.spos[j] = pos, sh.u.l.sbk[j] = bk;
    sh.u.l.epos[j] = e.pos, sh.u.l.ebk[j] = e.bk, sh.u.l.count[j] = e.count;
}

// step 2a: does lane j have to decode again?  (the state compare)  -> true, the state to start from in tpos / tbk
JH_HD bool phase_compare(Shared& sh, int j) {
    sh.u.l.tbk[j] = kTerminal;
    if (j == 0 || sh.u.l.ebk[j - 1] == kTerminal) return false;
    if (sh.u.l.epos[j - 1] == sh.u.l.spos[j] && sh.u.l.ebk[j - 1] == sh.u.l.sbk[j]) return false;
    sh.u.l.tpos[j] = sh.u.l.epos[j - 1], sh.u.l.tbk[j] = sh.u.l.ebk[j - 1];
    return true;
}

// step 2b
JH_HD void phase_again(const Image& im, Shared& sh, int64_t g0, int j) {
    if (sh.u.l.tbk[j] == kTerminal) return;
    const LaneEnd e = lane_run(im, sh.tab, sh.u.l.tpos[j], sh.u.l.tbk[j], -1, boundary_of(im, g0 + j), nullptr);
    sh.u.l.spos[j] = sh.u.l.tpos[j], sh.u.l.sbk[j] = sh.u.l.tbk[j];
    sh.u.l.epos[j] = e.pos, sh.u.l.ebk[j] = e.bk, sh.u.l.count[j] = e.count;
}

// step 3: inclusive prefix sum of the counts, one doubling step: sum[to] from sum[1 - to] (d = 0 copies the counts in)
JH_HD void phase_sum(Shared& sh, int j, int d, int to) {
    if (d == 0) {
        sh.u.l.sum[to][j] = sh.u.l.count[j];
        return;
    }
    const uint32_t* from = sh.u.l.sum[1 - to];
    sh.u.l.sum[to][j] = from[j] + (j >= d ? from[j - d] : 0u);
}

// step 4: the exact decode with the writes
JH_HD void phase_write(const Image& im, Shared& sh, int64_t g0, int j, int from, int16_t* coef) {
    const int64_t first = sh.carry_blocks + (int64_t)(sh.u.l.sum[from][j] - sh.u.l.count[j]);
    const LaneEnd e = lane_run(im, sh.tab, sh.u.l.spos[j], sh.u.l.sbk[j], first, boundary_of(im, g0 + j), coef);
    sh.u.l.xpos[j] = e.pos, sh.u.l.xbk[j] = e.bk, sh.u.l.xcount[j] = e.count, sh.u.l.xcode[j] = e.code;
}

// step 4, the chain: is lane j one the round cannot pass?
JH_HD bool phase_chain(const Shared& sh, int j, int lanes) {
    if (sh.u.l.xbk[j] == kTerminal) return true;
    if (sh.u.l.xcount[j] != sh.u.l.count[j]) return true;
    return j + 1 < lanes && (sh.u.l.xpos[j] != sh.u.l.spos[j + 1] || sh.u.l.xbk[j] != sh.u.l.sbk[j + 1]);
}

// step 5: the MCUs of lane j, the differences of each component summed from the last restart interval's beginning
JH_HD int64_t dc_mcus_per_lane(const Image& im) { return (im.mcus + kLanes - 1) / kLanes; }

JH_HD void dc_walk(const Image& im, int j, DcSum& v, int16_t* coef, bool write) {
    const int64_t per = dc_mcus_per_lane(im);
    const int64_t m0 = j * per, m1 = m0 + per < im.mcus ? m0 + per : im.mcus;
    uint32_t p0 = v.s[0], p1 = v.s[1], p2 = v.s[2];  // (scalars: an array indexed by the component would leave the registers)
    for (int64_t m = m0; m < m1; ++m) {
        if (im.restart && m % im.restart == 0) p0 = p1 = p2 = 0, v.cut = 1;
        for (int b = 0; b < im.bpm; ++b) {
            const int64_t at = block_of(im, m * im.bpm + b);
            if (at < 0) continue;
            const int c = b < im.hs * im.vs ? 0 : b - im.hs * im.vs + 1;
            const uint32_t diff = (uint32_t)(int32_t)coef[at];
            const uint32_t now = (c == 0 ? p0 : c == 1 ? p1 : p2) + diff;
            if (c == 0) p0 = now; else if (c == 1) p1 = now; else p2 = now;
            if (write) coef[at] = (int16_t)now;
        }
    }
    v.s[0] = p0, v.s[1] = p1, v.s[2] = p2;
}

JH_HD void phase_dc_local(const Image& im, Shared& sh, int j, int16_t* coef) {
    DcSum v;
    v.s[0] = v.s[1] = v.s[2] = 0, v.cut = 0;
    dc_walk(im, j, v, coef, false);
    sh.u.dc[0][j] = v;
}

JH_HD void phase_dc_sum(Shared& sh, int j, int d, int to) {
    const DcSum* from = sh.u.dc[1 - to];
    DcSum v = from[j];
    if (j >= d && !v.cut) {
        const DcSum a = from[j - d];
        v.s[0] += a.s[0], v.s[1] += a.s[1], v.s[2] += a.s[2], v.cut = a.cut;
    }
    sh.u.dc[to][j] = v;
}

JH_HD void phase_dc_write(const Image& im, const Shared& sh, int j, int from, int16_t* coef) {
    DcSum v;
    v.s[0] = v.s[1] = v.s[2] = 0, v.cut = 0;
    if (j > 0) v = sh.u.dc[from][j - 1];
    dc_walk(im, j, v, coef, true);
}

// ---- the host stage ------------------------------------------------------------------------------------------------------------------
inline void copy_table(Table& t, const madtp_jpeg::HuffTable& h) {
    memset(&t, 0, sizeof(t));
    memcpy(t.look, h.look, sizeof(t.look));
    for (int i = 1; i <= 16; ++i) t.maxcode[i] = h.maxcode[i], t.valoffset[i] = h.valoffset[i];
    t.maxcode[0] = -1, t.maxcode[17] = h.maxcode[17];
    memcpy(t.vals, h.vals, sizeof(t.vals));
}

inline int prepare(const uint8_t* data, int64_t size, int32_t* info, uint16_t* qtables, Table* tables, int64_t* scan_begin,
                   madtp_jpeg::Header& h) {
    if (!data || !info || !qtables || !tables || !scan_begin || size < 0 || size > MADTP_JHUFF_MAX_BYTES) return MADTP_E_BADARG;
    h = madtp_jpeg::Header();
    const int rc = madtp_jpeg::parse_header(data, size, h);
    if (rc) return rc;
    memset(info, 0, MADTP_JPEG_INFO_FIELDS * sizeof(int32_t));
    info[MADTP_JPEG_I_WIDTH] = h.width;
    info[MADTP_JPEG_I_HEIGHT] = h.height;
    info[MADTP_JPEG_I_COMPONENTS] = h.components;
    info[MADTP_JPEG_I_HS] = h.hs;
    info[MADTP_JPEG_I_VS] = h.vs;
    info[MADTP_JPEG_I_BLOCKS_X] = h.blocks_x;
    info[MADTP_JPEG_I_BLOCKS_Y] = h.blocks_y;
    info[MADTP_JPEG_I_RESTART] = h.restart;
    info[MADTP_JPEG_I_BLOCKS] = (int32_t)madtp_jpeg::total_blocks(h);
    memset(qtables, 0, 3 * 64 * sizeof(uint16_t));
    memset(tables, 0, 6 * sizeof(Table));
    for (int c = 0; c < h.components; ++c) {
        memcpy(qtables + 64 * c, h.q[h.comp_tq[c]], 64 * sizeof(uint16_t));
        copy_table(tables[2 * c], h.dc[h.comp_td[c]]);
        copy_table(tables[2 * c + 1], h.ac[h.comp_ta[c]]);
    }
    *scan_begin = h.scan_begin;
    return 0;
}

// The passes of jpeg_huff.hip's kernel with the lanes in a loop: every `for (j ...)` here is one phase between two barriers there.
// sh.tab holds the image's record.  -> the code; coef is zeroed first, as the kernel does.
inline int decode_image_host(const Image& im, Shared& sh, int16_t* coef, int32_t* status) {
    memset(coef, 0, (size_t)(128 * im.blocks));
    int code = MADTP_JPEG_E_TRUNCATED, passes = 0, serial = 0;
    bool over = false;
    sh.carry_pos = (uint32_t)(im.scan * 8), sh.carry_bk = 0, sh.carry_blocks = 0;
    for (int64_t g0 = 0; g0 < im.lanes && !over; g0 += kLanes) {
        const int lanes = (int)(im.lanes - g0 < kLanes ? im.lanes - g0 : kLanes);
        for (int j = 0; j < lanes; ++j) phase_first(im, sh, g0, j);
        ++passes;
        for (int pass = 2; pass <= lanes; ++pass) {
            bool again = false;
            for (int j = 0; j < lanes; ++j) again |= phase_compare(sh, j);
            if (!again) break;
            for (int j = 0; j < lanes; ++j) phase_again(im, sh, g0, j);
            ++passes;
        }
        int to = 0;
        for (int j = 0; j < lanes; ++j) phase_sum(sh, j, 0, to);
        for (int d = 1; d < lanes; d <<= 1) {
            to ^= 1;
            for (int j = 0; j < lanes; ++j) phase_sum(sh, j, d, to);
        }
        for (int j = 0; j < lanes; ++j) phase_write(im, sh, g0, j, to, coef);
        int first_bad = lanes;
        for (int j = lanes - 1; j >= 0; --j)
            if (phase_chain(sh, j, lanes)) first_bad = j;
        if (first_bad < lanes) {
            over = true;
            if (sh.u.l.xbk[first_bad] == kTerminal) {
                code = sh.u.l.xcode[first_bad];
            } else {  // the lanes' guesses and the exact rules parted: one lane, from the beginning
                serial = 1;
                memset(coef, 0, (size_t)(128 * im.blocks));
                code = lane_run(im, sh.tab, (uint32_t)(im.scan * 8), 0, 0, kNoBoundary, coef).code;
            }
        } else {
            sh.carry_pos = sh.u.l.xpos[lanes - 1], sh.carry_bk = sh.u.l.xbk[lanes - 1];
            sh.carry_blocks += sh.u.l.sum[to][lanes - 1];
        }
    }
    if (code == 0) {
        for (int j = 0; j < kLanes; ++j) phase_dc_local(im, sh, j, coef);
        int to = 0;
        for (int d = 1; d < kLanes; d <<= 1) {
            to ^= 1;
            for (int j = 0; j < kLanes; ++j) phase_dc_sum(sh, j, d, to);
        }
        for (int j = 0; j < kLanes; ++j) phase_dc_write(im, sh, j, to, coef);
    }
    status[MADTP_JHUFF_S_CODE] = code, status[MADTP_JHUFF_S_PASSES] = passes;
    status[MADTP_JHUFF_S_SUBSEQS] = im.lanes, status[MADTP_JHUFF_S_SERIAL] = serial;
    return code;
}

inline int decode_host(const uint8_t* data, int64_t size, int subseq_bytes, int16_t* coef, int64_t coef_capacity, int32_t* status,
                       madtp_jpeg::Header& h, Shared& sh) {
    if (!data || !coef || !status || subseq_bytes < 0 || (subseq_bytes & 3)) return MADTP_E_BADARG;
    int32_t info[MADTP_JPEG_INFO_FIELDS];
    uint16_t q[3 * 64];
    int64_t scan = 0;
    status[0] = status[1] = status[2] = status[3] = 0;
    const int rc = prepare(data, size, info, q, sh.tab, &scan, h);
    if (rc) return status[MADTP_JHUFF_S_CODE] = rc;
    Image im;
    if (!make_image(im, data, size, scan, h.components, h.hs, h.vs, h.blocks_x, h.blocks_y, h.restart, subseq_bytes)) return MADTP_E_BADARG;
    if (coef_capacity < 64 * im.blocks) return MADTP_E_BADARG;
    im.zz = madtp_jpeg::kZigzagToColumnMajor;
    return decode_image_host(im, sh, coef, status);
}

}  // namespace madtp_jhuff
