"""The PNG decode restated in numpy, for the tests of madtp_amd/png.py: the chunk walk, the five unfilter recurrences and the sample
expansion are its own; its inflate is Python's zlib.  deflate_stats() walks a deflate stream symbol by symbol (slowly) to say what a
corpus holds: block types, match distances."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_pil.npz")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def corpus():
    """-> {name: (file bytes, Pillow's recorded uint8 [h, w, 3])}"""
    z = np.load(GOLDEN)
    return {str(n): (z["file_" + str(n)].tobytes(), z["rgb_" + str(n)]) for n in z["names"]}


def chunks(data):
    """-> [(type, body)] up to and with IEND"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while True:
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        out.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
        if kind == b"IEND":
            return out


def parse(data):
    """-> dict(width, height, depth, color, channels, rowbytes, bpp, raw_bytes, stream (bytes), palette (uint8 [768]), entries)"""
    cs = chunks(data)
    w, h, depth, color, _, _, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    assert cs[0][0] == b"IHDR" and interlace == 0
    ch = CHANNELS[color]
    rowbytes = (w * ch * depth + 7) // 8
    palette = np.zeros(768, np.uint8)
    entries = 0
    if color == 3:
        plte = [b for k, b in cs if k == b"PLTE"][0]
        palette[:len(plte)] = np.frombuffer(plte, np.uint8)
        entries = len(plte) // 3
    return dict(width=w, height=h, depth=depth, color=color, channels=ch, rowbytes=rowbytes, bpp=max(1, ch * depth // 8),
                raw_bytes=h * (1 + rowbytes), stream=b"".join(b for k, b in cs if k == b"IDAT"), palette=palette, entries=entries)


def unfilter(raw, h, rowbytes, bpp):
    """filtered scanlines (bytes) -> uint8 [h, rowbytes]"""
    lines = np.frombuffer(raw, np.uint8).reshape(h, 1 + rowbytes)
    out = np.zeros((h, rowbytes), np.uint8)
    prev = np.zeros(rowbytes, np.int32)
    for r in range(h):
        ft, x = int(lines[r, 0]), lines[r, 1:].astype(np.int32)
        assert ft <= 4
        cur = np.zeros(rowbytes, np.int32)
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        else:
            for i in range(rowbytes):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) >> 1
                else:
                    q = a + b - c
                    pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                    p = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (x[i] + p) & 255
        out[r] = cur
        prev = cur
    return out


def expand(rows, w, depth, color, palette):
    """unfiltered rows uint8 [h, rowbytes] -> what Pillow's convert('RGB') gives, uint8 [h, w, 3]"""
    h = rows.shape[0]
    if depth == 16:
        s = rows.reshape(h, w, CHANNELS[color], 2)[..., 0]  # the high byte
    elif depth == 8:
        s = rows.reshape(h, w, CHANNELS[color])
    else:
        per = 8 // depth
        shifts = np.array([8 - depth * (k + 1) for k in range(per)], np.uint8)
        s = ((rows[:, :, None] >> shifts) & ((1 << depth) - 1)).reshape(h, -1)[:, :w, None]
    if color in (2, 6):
        return np.ascontiguousarray(s[..., :3])
    v = s[..., 0]
    if color == 3:
        return palette.reshape(256, 3)[v]
    if depth < 8:
        v = v * (255 // ((1 << depth) - 1))
    return np.repeat(v[..., None].astype(np.uint8), 3, axis=2)


def decode(data):
    """file bytes -> uint8 [h, w, 3]"""
    p = parse(data)
    raw = zlib.decompress(p["stream"])
    assert len(raw) == p["raw_bytes"]
    return expand(unfilter(raw, p["height"], p["rowbytes"], p["bpp"]), p["width"], p["depth"], p["color"], p["palette"])


# ---- a deflate walker: what a stream is made of ------------------------------------------------------------------------------------
_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
          16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def _table(lengths):
    code, table = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                table[(n, code)] = s
                code += 1
        code <<= 1
    return table


def deflate_stats(stream):
    """a valid zlib stream -> dict(types: set of block types, distances: set of match distances, overlaps: matches with dist < len,
    cross: a dynamic header whose repeat code ran from the literal lengths into the distance lengths, longest: the longest code a
    symbol of a dynamic block was sent with)"""
    body = bytes(stream[2:])
    at = 0

    def take(n):
        nonlocal at
        v = (int.from_bytes(body[at >> 3:(at >> 3) + 4], "little") >> (at & 7)) & ((1 << n) - 1)
        at += n
        return v

    def symbol(table):
        code = 0
        for n in range(1, 16):
            code = code << 1 | take(1)
            if (n, code) in table:
                return table[n, code]
        raise AssertionError("no code")

    types, distances, overlaps, cross, produced, longest = set(), set(), 0, False, 0, 0
    while True:
        last, kind = take(1), take(2)
        types.add(kind)
        if kind == 0:
            at = (at + 7) // 8 * 8
            n = take(16)
            take(16)
            at += 8 * n
            produced += n
        else:
            if kind == 1:
                lit, dist = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32)
            else:
                nlen, ndist, ncode = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[_ORDER[i]] = take(3)
                cl, lengths = _table(cl), []
                while len(lengths) < nlen + ndist:
                    s = symbol(cl)
                    rep = [0] * (3 + take(3)) if s == 17 else [0] * (11 + take(7)) if s == 18 else [lengths[-1]] * (3 + take(2)) if s == 16 else [s]
                    cross = cross or (len(lengths) < nlen < len(lengths) + len(rep))
                    lengths += rep
                lit, dist = _table(lengths[:nlen]), _table(lengths[nlen:])
            while True:
                before = at
                s = symbol(lit)
                longest = max(longest, at - before)
                if s == 256:
                    break
                if s < 256:
                    produced += 1
                    continue
                n = _LBASE[s - 257] + take(_LEXT[s - 257])
                before = at
                d = symbol(dist)
                longest = max(longest, at - before)
                d = _DBASE[d] + take(_DEXT[d])
                distances.add(d)
                overlaps += d < n
                produced += n
        if last:
            return dict(types=types, distances=distances, overlaps=overlaps, cross=cross, produced=produced, longest=longest)


# ---- writing files and streams by hand: what the malformed and refused cases of the tests are made of ---------------------------------
def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def ihdr(w, h, depth, color, compression=0, method=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color, compression, method, interlace))


def build(*parts):
    """the signature, the chunks given (bytes each), IEND"""
    return SIGNATURE + b"".join(parts) + chunk(b"IEND")


class BitWriter:
    """a deflate stream written bit by bit"""

    def __init__(self, header=b"\x78\x9c"):
        self.acc, self.n, self.out = 0, 0, bytearray(header)

    def bits(self, value, count):  # LSB first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, value, count):  # a Huffman code: MSB first
        return self.bits(int(format(value, f"0{count}b")[::-1], 2), count)

    def fixed(self, s):  # a literal / length symbol of the fixed code
        return self.code(*((0x30 + s, 8) if s < 144 else (0x190 + s - 144, 9) if s < 256 else (s - 256, 7) if s < 280 else (0xC0 + s - 280, 8)))

    def done(self, adler=0):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out) + struct.pack(">I", adler)
