// The host stage of the JPEG decode (include/madtp_jpeg.h): parse a baseline file and Huffman-decode its one interleaved scan into
// de-zigzagged int16 coefficient blocks, stored column-major for the device stage.  Host-only C++17: no HIP include, no allocation,
// no mutable static, no GPU call - it compiles with a plain C++ compiler (tools/jpeg_host_check.cpp runs it under sanitizers) and a
// DataLoader worker may call it.  Every read is bounds-checked against the given size and every write against the given capacity;
// a malformed stream ends in a negative code, never in a partial image that is reported as whole.
//
// Speed: a 64-bit bit buffer refilled bytewise (FF 00 unstuffed on the way), a 9-bit lookahead table per Huffman table that gives
// length and symbol in one read, a canonical search only for the longer codes; no per-bit work.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/madtp_jpeg.h"

namespace madtp_jpeg {

constexpr int kLookBits = 9;

// zigzag position -> element of the column-major block: natural index n = 8 r + c is stored at 8 c + r
inline constexpr uint8_t kZigzagToColumnMajor[64] = {
    0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,  13, 20, 27, 34, 41, 48, 56, 49, 42, 35,
    28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58, 51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};
inline constexpr uint8_t kZigzagToNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct HuffTable {
    bool defined = false;
    uint16_t look[1 << kLookBits];  // (length << 8) | symbol of the code that begins these 9 bits, 0 = longer than 9 bits or none
    int32_t maxcode[18];            // largest code of each length, -1 = none
    int32_t valoffset[17];          // index of a code's symbol = code + valoffset[length]
    uint8_t vals[256];
};

struct Header {
    int width = 0, height = 0, components = 0;
    int hs = 1, vs = 1;            // luma sampling
    int blocks_x = 0, blocks_y = 0;  // luma plane, MCU-padded
    int mcus_x = 0, mcus_y = 0;
    int restart = 0;
    int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0}, comp_td[3] = {0, 0, 0}, comp_ta[3] = {0, 0, 0};
    bool have_sof = false, have_q[4] = {false, false, false, false};
    int adobe_transform = -1;
    uint16_t q[4][64];  // natural order
    HuffTable dc[4], ac[4];
    int64_t scan_begin = 0;  // first byte of the entropy-coded data
};

inline int64_t total_blocks(const Header& h) {
    const int64_t luma = (int64_t)h.blocks_x * h.blocks_y;
    return h.components == 1 ? luma : luma + 2 * (luma / (h.hs * h.vs));
}

inline int build_huffman(HuffTable& t, const uint8_t* counts, const uint8_t* vals, int n_vals, bool is_dc) {
    memset(t.look, 0, sizeof(t.look));
    memcpy(t.vals, vals, (size_t)n_vals);
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = counts[len - 1];
        if (code + n > (1 << len)) return MADTP_JPEG_E_HEADER;  // more codes than the length has
        t.valoffset[len] = k - code;
        t.maxcode[len] = n ? code + n - 1 : -1;
        for (int i = 0; i < n; ++i, ++k, ++code) {
            if (is_dc && vals[k] > 15) return MADTP_JPEG_E_HEADER;
            if (len <= kLookBits) {
                const int first = code << (kLookBits - len);
                for (int j = 0; j < (1 << (kLookBits - len)); ++j) t.look[first + j] = (uint16_t)(len << 8 | vals[k]);
            }
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.defined = true;
    return 0;
}

// ---- the header: every marker segment up to the scan's first byte --------------------------------------------------------------
inline int parse_header(const uint8_t* d, int64_t size, Header& h) {
    if (size < 2 || d[0] != 0xFF || d[1] != 0xD8) return MADTP_JPEG_E_NOT_JPEG;
    int64_t p = 2;
    for (;;) {
        if (p >= size) return MADTP_JPEG_E_TRUNCATED;
        if (d[p] != 0xFF) return MADTP_JPEG_E_HEADER;  // a marker must stand here
        while (p < size && d[p] == 0xFF) ++p;          // fill bytes
        if (p >= size) return MADTP_JPEG_E_TRUNCATED;
        const int m = d[p++];
        if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return MADTP_JPEG_E_HEADER;
        if (p + 2 > size) return MADTP_JPEG_E_TRUNCATED;
        const int64_t len = (int64_t)d[p] << 8 | d[p + 1];
        if (len < 2) return MADTP_JPEG_E_SEGMENT;
        if (len > size - p) return MADTP_JPEG_E_SEGMENT;
        const uint8_t* s = d + p + 2;
        const int64_t n = len - 2;
        p += len;
        if (m == 0xC0 || m == 0xC1) {
            if (h.have_sof) return MADTP_JPEG_E_HEADER;
            if (n < 6) return MADTP_JPEG_E_SEGMENT;
            if (s[0] != 8) return MADTP_JPEG_E_PRECISION;
            h.height = s[1] << 8 | s[2];
            h.width = s[3] << 8 | s[4];
            const int nf = s[5];
            if (n != 6 + 3 * (int64_t)nf) return MADTP_JPEG_E_SEGMENT;
            if (nf != 1 && nf != 3) return MADTP_JPEG_E_COMPONENTS;
            if (h.height == 0) return MADTP_JPEG_E_DNL;
            if (h.width == 0) return MADTP_JPEG_E_HEADER;
            if (h.width > MADTP_JPEG_MAX_SIDE || h.height > MADTP_JPEG_MAX_SIDE) return MADTP_JPEG_E_SIDE;
            int sh[3], sv[3];
            for (int c = 0; c < nf; ++c) {
                h.comp_id[c] = s[6 + 3 * c];
                sh[c] = s[7 + 3 * c] >> 4;
                sv[c] = s[7 + 3 * c] & 15;
                h.comp_tq[c] = s[8 + 3 * c];
                if (sh[c] < 1 || sh[c] > 4 || sv[c] < 1 || sv[c] > 4 || h.comp_tq[c] > 3) return MADTP_JPEG_E_HEADER;
            }
            h.components = nf;
            h.hs = h.vs = 1;
            if (nf == 3) {
                if (h.comp_id[0] == 'R' && h.comp_id[1] == 'G' && h.comp_id[2] == 'B') return MADTP_JPEG_E_RGB_IDS;
                if (sh[1] != 1 || sv[1] != 1 || sh[2] != 1 || sv[2] != 1) return MADTP_JPEG_E_CHROMA;
                if (!((sh[0] == 1 && sv[0] == 1) || (sh[0] == 2 && sv[0] == 1) || (sh[0] == 2 && sv[0] == 2))) return MADTP_JPEG_E_LUMA;
                h.hs = sh[0];
                h.vs = sv[0];
            }
            h.mcus_x = (h.width + 8 * h.hs - 1) / (8 * h.hs);
            h.mcus_y = (h.height + 8 * h.vs - 1) / (8 * h.vs);
            h.blocks_x = h.mcus_x * h.hs;
            h.blocks_y = h.mcus_y * h.vs;
            h.have_sof = true;
        } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return MADTP_JPEG_E_PROGRESSIVE;  // SOF2 .. SOF15 and DAC
        } else if (m == 0xC4) {
            int64_t at = 0;
            while (at < n) {
                if (n - at < 17) return MADTP_JPEG_E_SEGMENT;
                const int tc = s[at] >> 4, th = s[at] & 15;
                if (tc > 1 || th > 3) return MADTP_JPEG_E_HEADER;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[at + 1 + i];
                if (total > 256) return MADTP_JPEG_E_HEADER;
                if (n - at - 17 < total) return MADTP_JPEG_E_SEGMENT;
                const int rc = build_huffman(tc ? h.ac[th] : h.dc[th], s + at + 1, s + at + 17, total, tc == 0);
                if (rc) return rc;
                at += 17 + total;
            }
        } else if (m == 0xDB) {
            int64_t at = 0;
            while (at < n) {
                const int pq = s[at] >> 4, tq = s[at] & 15;
                if (pq > 1 || tq > 3) return MADTP_JPEG_E_HEADER;
                const int bytes = 64 * (pq + 1);
                if (n - at - 1 < bytes) return MADTP_JPEG_E_SEGMENT;
                for (int i = 0; i < 64; ++i) {
                    const uint8_t* v = s + at + 1 + i * (pq + 1);
                    h.q[tq][kZigzagToNatural[i]] = pq ? (uint16_t)(v[0] << 8 | v[1]) : v[0];
                }
                h.have_q[tq] = true;
                at += 1 + bytes;
            }
        } else if (m == 0xDD) {
            if (n != 2) return MADTP_JPEG_E_SEGMENT;
            h.restart = s[0] << 8 | s[1];
        } else if (m == 0xDC) {
            return MADTP_JPEG_E_DNL;
        } else if (m == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) h.adobe_transform = s[11];
        } else if (m == 0xDA) {
            if (!h.have_sof) return MADTP_JPEG_E_HEADER;
            if (n < 1) return MADTP_JPEG_E_SEGMENT;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * (int64_t)ns) return MADTP_JPEG_E_SEGMENT;
            if (ns != h.components) return ns < h.components ? MADTP_JPEG_E_SCANS : MADTP_JPEG_E_HEADER;
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h.comp_id[c]) return MADTP_JPEG_E_SCANS;
                h.comp_td[c] = s[2 + 2 * c] >> 4;
                h.comp_ta[c] = s[2 + 2 * c] & 15;
                if (h.comp_td[c] > 3 || h.comp_ta[c] > 3) return MADTP_JPEG_E_HEADER;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return MADTP_JPEG_E_SCAN_PARAMS;
            if (h.components == 3 && h.adobe_transform == 0) return MADTP_JPEG_E_ADOBE_RGB;
            for (int c = 0; c < ns; ++c)
                if (!h.have_q[h.comp_tq[c]] || !h.dc[h.comp_td[c]].defined || !h.ac[h.comp_ta[c]].defined) return MADTP_JPEG_E_NO_TABLE;
            h.scan_begin = p;
            return 0;
        }
        // every other segment (APPn, COM, JPGn, ...) is skipped by its length
    }
}

// ---- the bit reader ------------------------------------------------------------------------------------------------------------
// acc holds n bits, the next one highest.  At a marker or the end of the data the reader goes on with zero bits and counts them in
// `pad`: the real bits left are n - pad, and a negative value means the decoder consumed bits the stream does not have.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0, pad = 0;

    inline void fill() {
        while (n <= 56) {
            unsigned b = 0;
            if (p < end && *p != 0xFF) {
                b = *p++;
            } else if (p + 1 < end && p[1] == 0x00) {  // (here *p is FF) a stuffed FF
                b = 0xFF;
                p += 2;
            } else {  // a marker, or the end: stay in front of it
                pad += 8;
            }
            acc = acc << 8 | b;
            n += 8;
        }
    }
    inline unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }
    inline void reset() { acc = 0, n = 0, pad = 0; }
};

// one symbol; the caller has made sure of 16 bits.  -> symbol, or -1 for a pattern that is no code
inline int decode_symbol(BitReader& br, const HuffTable& t) {
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

inline int receive_extend(BitReader& br, int s) {  // s in 1 .. 15
    const int v = (int)br.peek(s);
    br.n -= s;
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

inline int decode_block(BitReader& br, const HuffTable& dc, const HuffTable& ac, int& pred, int16_t* block) {
    memset(block, 0, 64 * sizeof(int16_t));
    if (br.n < 32) br.fill();
    int s = decode_symbol(br, dc);
    if (s < 0) return MADTP_JPEG_E_CODE;
    if (s) pred += receive_extend(br, s);
    block[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if (br.n < 32) br.fill();
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return MADTP_JPEG_E_CODE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) return MADTP_JPEG_E_INDEX;
            block[kZigzagToColumnMajor[k]] = (int16_t)receive_extend(br, s);
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 63) return MADTP_JPEG_E_INDEX;  // a run of zeros is only coded in front of a coefficient
        } else if (r == 0) {
            break;
        } else {
            return MADTP_JPEG_E_CODE;  // an end-of-band run: progressive only
        }
    }
    return br.n < br.pad ? MADTP_JPEG_E_TRUNCATED : 0;
}

// the marker that must stand at the reader's position once the buffered bits (less than a byte of padding) are dropped -> marker
// byte, or a negative code
inline int next_marker(BitReader& br, int extra_code) {
    if (br.n < br.pad) return MADTP_JPEG_E_TRUNCATED;
    if (br.n - br.pad >= 8) return extra_code;  // whole bytes of entropy data that no MCU used
    br.reset();
    if (br.p >= br.end) return MADTP_JPEG_E_TRUNCATED;
    if (*br.p != 0xFF) return extra_code;
    while (br.p < br.end && *br.p == 0xFF) ++br.p;
    if (br.p >= br.end) return MADTP_JPEG_E_TRUNCATED;
    return *br.p++;
}

inline int inspect(const uint8_t* data, int64_t size, int32_t* info, uint16_t* qtables) {
    if (!data || !info || !qtables || size < 0) return MADTP_E_BADARG;
    Header h;
    const int rc = parse_header(data, size, h);
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
    info[MADTP_JPEG_I_BLOCKS] = (int32_t)total_blocks(h);
    memset(qtables, 0, 3 * 64 * sizeof(uint16_t));
    for (int c = 0; c < h.components; ++c) memcpy(qtables + 64 * c, h.q[h.comp_tq[c]], 64 * sizeof(uint16_t));
    return 0;
}

inline int entropy_decode(const uint8_t* data, int64_t size, int16_t* coef, int64_t coef_capacity) {
    if (!data || !coef || size < 0) return MADTP_E_BADARG;
    Header h;
    int rc = parse_header(data, size, h);
    if (rc) return rc;
    if (coef_capacity < 64 * total_blocks(h)) return MADTP_E_BADARG;
    BitReader br;
    br.p = data + h.scan_begin;
    br.end = data + size;
    const int64_t luma = (int64_t)h.blocks_x * h.blocks_y, chroma = luma / (h.hs * h.vs);
    int16_t* plane[3] = {coef, coef + 64 * luma, coef + 64 * (luma + chroma)};
    const int chroma_x = h.blocks_x / h.hs;
    int pred[3] = {0, 0, 0};
    const int64_t mcus = (int64_t)h.mcus_x * h.mcus_y;
    int64_t until_restart = h.restart ? h.restart : mcus + 1;
    int expected = 0;
    int64_t mcu = 0;
    for (int my = 0; my < h.mcus_y; ++my) {
        for (int mx = 0; mx < h.mcus_x; ++mx, ++mcu) {
            if (until_restart == 0) {
                const int m = next_marker(br, MADTP_JPEG_E_RESTART);
                if (m < 0) return m;
                if (m != 0xD0 + expected) return MADTP_JPEG_E_RESTART;
                expected = (expected + 1) & 7;
                pred[0] = pred[1] = pred[2] = 0;
                until_restart = h.restart;
            }
            --until_restart;
            for (int v = 0; v < h.vs; ++v)
                for (int u = 0; u < h.hs; ++u) {
                    int16_t* b = plane[0] + 64 * ((int64_t)(my * h.vs + v) * h.blocks_x + (mx * h.hs + u));
                    if ((rc = decode_block(br, h.dc[h.comp_td[0]], h.ac[h.comp_ta[0]], pred[0], b)) != 0) return rc;
                }
            for (int c = 1; c < h.components; ++c) {
                int16_t* b = plane[c] + 64 * ((int64_t)my * chroma_x + mx);
                if ((rc = decode_block(br, h.dc[h.comp_td[c]], h.ac[h.comp_ta[c]], pred[c], b)) != 0) return rc;
            }
        }
    }
    const int m = next_marker(br, MADTP_JPEG_E_MARKER);
    if (m < 0) return m;
    if (m == 0xD9) return 0;
    if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD) return MADTP_JPEG_E_SCANS;
    if (m == 0xDC) return MADTP_JPEG_E_DNL;
    return MADTP_JPEG_E_MARKER;
}

inline const char* strerror_jpeg(int code) {
    switch (code) {
        case MADTP_JPEG_E_PROGRESSIVE: return "unsupported JPEG: progressive, lossless or arithmetic coding (SOF2 and up); only baseline Huffman files are decoded";
        case MADTP_JPEG_E_PRECISION: return "unsupported JPEG: sample precision is not 8 bits";
        case MADTP_JPEG_E_COMPONENTS: return "unsupported JPEG: component count is not 1 or 3 (CMYK / YCCK)";
        case MADTP_JPEG_E_ADOBE_RGB: return "unsupported JPEG: Adobe APP14 transform 0 (RGB, not YCbCr)";
        case MADTP_JPEG_E_RGB_IDS: return "unsupported JPEG: component ids R, G, B (RGB, not YCbCr)";
        case MADTP_JPEG_E_CHROMA: return "unsupported JPEG: chroma sampling is not 1x1";
        case MADTP_JPEG_E_LUMA: return "unsupported JPEG: luma sampling is not 1x1, 2x1 or 2x2";
        case MADTP_JPEG_E_SCANS: return "unsupported JPEG: more than one scan";
        case MADTP_JPEG_E_DNL: return "unsupported JPEG: the height comes in a DNL segment";
        case MADTP_JPEG_E_SIDE: return "unsupported JPEG: a side is over 8192 pixels";
        case MADTP_JPEG_E_SCAN_PARAMS: return "unsupported JPEG: spectral selection or successive approximation in the scan header";
        case MADTP_JPEG_E_TRUNCATED: return "corrupt JPEG: the data ends before the image does";
        case MADTP_JPEG_E_CODE: return "corrupt JPEG: a bit pattern that is no Huffman code of its table";
        case MADTP_JPEG_E_INDEX: return "corrupt JPEG: a coefficient index beyond 63";
        case MADTP_JPEG_E_NO_TABLE: return "corrupt JPEG: a quantisation or Huffman table is used but never defined";
        case MADTP_JPEG_E_RESTART: return "corrupt JPEG: a restart marker is missing or out of sequence";
        case MADTP_JPEG_E_SEGMENT: return "corrupt JPEG: a segment length beyond the data or shorter than its content";
        case MADTP_JPEG_E_NOT_JPEG: return "corrupt JPEG: the data does not begin with SOI";
        case MADTP_JPEG_E_HEADER: return "corrupt JPEG: a frame, scan or table segment with impossible content";
        case MADTP_JPEG_E_MARKER: return "corrupt JPEG: the scan is not followed by EOI";
        default: return nullptr;
    }
}

}  // namespace madtp_jpeg
