"""A numpy restatement of the whole baseline JPEG decode the way libjpeg-turbo (Pillow's JPEG library) does it by default: an own
Huffman entropy decoder, dequantisation + the `islow` integer IDCT, h2v1 / h2v2 "fancy" upsampling, the fixed-point colour conversion.
It is slow and plain on purpose: the CPU tests hold it against Pillow's pixels (recorded, and live where Pillow is installed), and
the GPU tests hold madtp_amd.jpeg against it.  Never imported by the product.

All IDCT arithmetic is numpy int32, which wraps like the device's 32-bit integers do; no Pillow-written file comes near the wrap."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


def _huffman_lut(counts, vals):
    """16 counts + symbols -> list of 65536 (length, symbol) or None, indexed by the next 16 bits"""
    lut = [None] * 65536
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            first = code << (16 - length)
            lut[first:first + (1 << (16 - length))] = [(length, vals[k])] * (1 << (16 - length))
            code += 1
            k += 1
        code <<= 1
    return lut


def parse(data):
    """bytes -> header dict (everything up to the scan's first byte)"""
    d = bytes(data)
    if d[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    h = {"q": {}, "dc": {}, "ac": {}, "restart": 0}
    p = 2
    while True:
        if d[p] != 0xFF:
            raise ValueError(f"no marker at {p}")
        while d[p] == 0xFF:
            p += 1
        m = d[p]
        p += 1
        n = d[p] << 8 | d[p + 1]
        s = d[p + 2:p + n]
        p += n
        if m in (0xC0, 0xC1):
            if s[0] != 8:
                raise ValueError("precision")
            h["height"], h["width"] = s[1] << 8 | s[2], s[3] << 8 | s[4]
            h["comps"] = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
        elif 0xC2 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise ValueError("not a baseline Huffman file")
        elif m == 0xC4:
            at = 0
            while at < len(s):
                counts = list(s[at + 1:at + 17])
                total = sum(counts)
                h["ac" if s[at] >> 4 else "dc"][s[at] & 15] = _huffman_lut(counts, list(s[at + 17:at + 17 + total]))
                at += 17 + total
        elif m == 0xDB:
            at = 0
            while at < len(s):
                pq, tq = s[at] >> 4, s[at] & 15
                raw = np.frombuffer(s[at + 1:at + 1 + 64 * (pq + 1)], dtype=">u2" if pq else np.uint8).astype(np.uint16)
                table = np.zeros(64, dtype=np.uint16)
                table[ZIGZAG] = raw
                h["q"][tq] = table
                at += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            h["restart"] = s[0] << 8 | s[1]
        elif m == 0xDA:
            ns = s[0]
            if ns != len(h["comps"]) or tuple(s[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise ValueError("not one interleaved sequential scan")
            h["tables"] = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(ns)]
            h["scan"] = p
            break
    comps = h["comps"]
    h["components"] = len(comps)
    if len(comps) == 1:
        h["hs"], h["vs"] = 1, 1
    elif len(comps) == 3 and comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1) and comps[0][1:3] in ((1, 1), (2, 1), (2, 2)):
        h["hs"], h["vs"] = comps[0][1], comps[0][2]
    else:
        raise ValueError("unsupported components / sampling")
    h["mcus_x"] = -(-h["width"] // (8 * h["hs"]))
    h["mcus_y"] = -(-h["height"] // (8 * h["vs"]))
    h["blocks_x"], h["blocks_y"] = h["mcus_x"] * h["hs"], h["mcus_y"] * h["vs"]
    h["qtables"] = np.stack([h["q"][c[3]] for c in comps] + [np.zeros(64, dtype=np.uint16)] * (3 - len(comps)))
    return h


class _Bits:
    """the bits of one restart interval, FF 00 already unstuffed"""

    def __init__(self, raw):
        self.b = raw + b"\0\0\0\0"
        self.pos = 0
        self.limit = 8 * len(raw)

    def peek16(self):
        i = self.pos >> 3
        return ((self.b[i] << 16 | self.b[i + 1] << 8 | self.b[i + 2]) >> (8 - (self.pos & 7))) & 0xFFFF

    def symbol(self, lut):
        length, sym = lut[self.peek16()]
        self.pos += length
        return sym

    def extend(self, s):
        v = self.peek16() >> (16 - s)
        self.pos += s
        if self.pos > self.limit:
            raise ValueError("out of data")
        return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def entropy(data):
    """bytes -> (header, [int16 [blocks_y, blocks_x, 8, 8] per component]): de-zigzagged coefficients in natural (row-major) order,
    not dequantised"""
    d = bytes(data)
    h = parse(d)
    # the entropy-coded segments, split at the restart markers
    segments, cur, p = [], bytearray(), h["scan"]
    while True:
        b = d[p]
        if b != 0xFF:
            cur.append(b)
            p += 1
        elif d[p + 1] == 0:
            cur.append(0xFF)
            p += 2
        elif d[p + 1] == 0xFF:
            p += 1
        elif 0xD0 <= d[p + 1] <= 0xD7:
            segments.append(bytes(cur))
            cur = bytearray()
            p += 2
        elif d[p + 1] == 0xD9:
            segments.append(bytes(cur))
            break
        else:
            raise ValueError(f"marker {d[p + 1]:02x} in the scan")
    nc, hs, vs = h["components"], h["hs"], h["vs"]
    shape = [(h["blocks_y"], h["blocks_x"])] + [(h["mcus_y"], h["mcus_x"])] * (nc - 1)
    coef = [np.zeros(s + (64,), dtype=np.int16) for s in shape]
    mcus = h["mcus_x"] * h["mcus_y"]
    per = h["restart"] or mcus
    if len(segments) != -(-mcus // per):
        raise ValueError("restart intervals")
    mcu = 0
    for raw in segments:
        bits = _Bits(raw)
        pred = [0] * nc
        for _ in range(min(per, mcus - mcu)):
            my, mx = divmod(mcu, h["mcus_x"])
            for c in range(nc):
                dc, ac = h["dc"][h["tables"][c][0]], h["ac"][h["tables"][c][1]]
                for v in range(vs if c == 0 else 1):
                    for u in range(hs if c == 0 else 1):
                        block = coef[c][my * vs + v, mx * hs + u] if c == 0 else coef[c][my, mx]
                        s = bits.symbol(dc)
                        if s:
                            pred[c] += bits.extend(s)
                        block[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = bits.symbol(ac)
                            r, s = rs >> 4, rs & 15
                            if s:
                                k += r
                                block[ZIGZAG[k]] = bits.extend(s)
                                k += 1
                            elif r == 15:
                                k += 16
                            else:
                                break
            mcu += 1
    return h, [c.reshape(c.shape[:2] + (8, 8)) for c in coef]


def _idct_pass(x, shift):
    """jpeg_idct_islow's butterfly over eight int32 arrays -> eight int32 arrays, DESCALEd by `shift`"""
    x0, x1, x2, x3, x4, x5, x6, x7 = x
    z1 = (x2 + x6) * 4433
    tmp2 = z1 + x6 * -15137
    tmp3 = z1 + x2 * 6270
    tmp0 = (x0 + x4) << 13
    tmp1 = (x0 - x4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x7, x5, x3, x1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069, z4 * -3196
    z3 = z3 + z5
    z4 = z4 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    half = np.int32(1 << (shift - 1))
    return [(v + half) >> shift for v in (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1,
                                          tmp11 - tmp2, tmp10 - tmp3)]


def idct(coef, q):
    """int16 [by, bx, 8, 8] coefficients, uint16 [64] natural-order table -> uint8 [8 by, 8 bx] samples"""
    with np.errstate(over="ignore"):
        x = coef.astype(np.int32) * q.reshape(8, 8).astype(np.int32)
        cols = np.stack(_idct_pass([x[:, :, r, :] for r in range(8)], 11), axis=2)      # over the rows of each column
        rows = np.stack(_idct_pass([cols[:, :, :, c] for c in range(8)], 18), axis=3)   # over the columns of each row
    v = ((rows + 512) & 1023) - 512 + 128  # the range-limit table at x & 1023
    by, bx = coef.shape[:2]
    return np.clip(v, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(8 * by, 8 * bx)


def upsample_h2v1(s):
    """[rows, dw] real samples -> [rows, 2 dw]"""
    s = s.astype(np.int32)
    if s.shape[1] <= 2:
        return np.repeat(s, 2, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int32)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    return out


def upsample_h2v2(s):
    """[dh, dw] real samples -> [2 dh, 2 dw]"""
    s = s.astype(np.int32)
    if s.shape[1] <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    above = np.concatenate([s[:1], s[:-1]], axis=0)
    below = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), dtype=np.int32)
    for parity, far in ((0, above), (1, below)):
        c = 3 * s + far
        left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
        right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
        out[parity::2, 0::2] = (3 * c + left + 8) >> 4
        out[parity::2, 1::2] = (3 * c + right + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def planes_to_rgb(planes, w, h, hs, vs):
    """block-padded uint8 planes (one, or Y Cb Cr) -> uint8 [h, w, 3]"""
    if len(planes) == 1:
        return np.repeat(planes[0][:h, :w, None], 3, axis=2)
    dw, dh = -(-w // hs), -(-h // vs)
    up = []
    for p in planes[1:]:
        s = p[:dh, :dw]
        up.append(s if hs == 1 else upsample_h2v1(s) if vs == 1 else upsample_h2v2(s))
    return ycc_to_rgb(planes[0][:h, :w], up[0][:h, :w], up[1][:h, :w])


def decode_coefficients(h, coef):
    planes = [idct(coef[c], h["qtables"][c]) for c in range(h["components"])]
    return planes_to_rgb(planes, h["width"], h["height"], h["hs"], h["vs"])


def decode(data):
    """bytes -> uint8 [h, w, 3], what Image.open(...).convert("RGB") gives"""
    return decode_coefficients(*entropy(data))
