"""Writes tests/golden/png_pil.npz: the PNG corpus of tests/test_png_cpu.py / test_png_gpu.py - every file's bytes and the RGB that
the installed Pillow's Image.open(f).convert('RGB') gives for it.

    python tools/make_png_golden.py            # rewrite the corpus
    python tools/make_png_golden.py --dump DIR # also write every file as DIR/<name>.png (for tools/png_host_check.cpp)

Pillow's own writer uses few filter types and one deflate setting, so most files come from the small writer below: its own chunk
framing, the filter type of every row forced, the deflate stream made by zlib.compressobj with every strategy - or, for what zlib
never emits (a match at the full distance of 32768), by the bit writer below."""
import io
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "png_pil.npz")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_row(ft, cur, prev, bpp):
    """the filtered bytes of the unfiltered row `cur` under filter type ft (prev: the unfiltered row above, zeros for the first)"""
    cur, prev = cur.astype(np.int32), prev.astype(np.int32)
    a, c = np.zeros_like(cur), np.zeros_like(cur)  # the bytes one pixel to the left, of this row and of the row above
    a[bpp:], c[bpp:] = cur[:-bpp], prev[:-bpp]
    if ft == 0:
        pred = 0
    elif ft == 1:
        pred = a
    elif ft == 2:
        pred = prev
    elif ft == 3:
        pred = (a + prev) >> 1
    else:
        pred = np.array([paeth(int(x), int(y), int(z)) for x, y, z in zip(a, prev, c)], np.int32)
    return ((cur - pred) & 255).astype(np.uint8)


def scanlines(rows, filters, bpp):
    """rows: uint8 [h, rowbytes] unfiltered; filters: one type per row, or "heur" (the least sum of absolute values per row)"""
    out, prev = [], np.zeros(rows.shape[1], np.uint8)
    for r, cur in enumerate(rows):
        if isinstance(filters, str):
            cands = [filter_row(ft, cur, prev, bpp) for ft in range(5)]
            ft = int(np.argmin([np.abs(x.astype(np.int8).astype(np.int32)).sum() for x in cands]))
            line = cands[ft]
        else:
            ft = filters[r % len(filters)]
            line = filter_row(ft, cur, prev, bpp)
        out.append(bytes([ft]) + line.tobytes())
        prev = cur
    return b"".join(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(raw) + c.flush()


class BitWriter:
    """a deflate block written bit by bit: what zlib itself never emits goes through here"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):  # LSB first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, count):  # a Huffman code: MSB first
        self.bits(int(format(value, f"0{count}b")[::-1], 2), count)

    def symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def match258(self, dist_code, extra_bits, extra):
        self.symbol(285)
        self.code(dist_code, 5)
        self.bits(extra, extra_bits)

    def finish(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def deflate_far(raw):
    """zlib stream of `raw`, whose bytes from 32768 on repeat those 32768 before: literals, then matches of 258 at distance 32768
    (distance code 29 with 13 extra bits of 8191), the rest as literals"""
    w = BitWriter()
    w.bits(1, 1)
    w.bits(1, 2)
    at = 0
    while at < len(raw):
        if at >= 32768 and at + 258 <= len(raw) and raw[at:at + 258] == raw[at - 32768:at - 32768 + 258]:
            w.match258(29, 13, 8191)
            at += 258
        else:
            w.symbol(raw[at])
            at += 1
    w.symbol(256)
    return b"\x78\x9c" + w.finish() + struct.pack(">I", zlib.adler32(raw))


def deflate_cross():
    """zlib stream of the scanlines of a 4x2 gray image of 65s, as one dynamic block written by hand: zlib's own encoder sends the two
    code-length lists apart, so only here does a repeat code (17: six zeros) run from the literal / length lengths (258, 259) into
    the distance lengths (0 .. 3).  The distance code is a single code of one bit: incomplete, and accepted by zlib as such."""
    raw = bytes([0, 65, 65, 65, 65] * 2)
    w = BitWriter()
    w.bits(1, 1)
    w.bits(2, 2)
    w.bits(3, 5)   # 260 literal / length codes
    w.bits(4, 5)   # 5 distance codes
    w.bits(14, 4)  # 18 code-length codes: up to symbol 1 in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1
    for n in [0, 2, 2] + [0] * 12 + [2, 0, 2]:
        w.bits(n, 3)
    cl = {1: 0, 2: 1, 17: 2, 18: 3}  # four codes of two bits
    for sym, extra_bits, extra in ((2, 0, 0), (18, 7, 53), (2, 0, 0), (18, 7, 127), (18, 7, 41), (2, 0, 0), (2, 0, 0), (17, 3, 3), (1, 0, 0)):
        w.code(cl[sym], 2)
        w.bits(extra, extra_bits)
    lit = {0: 0, 65: 1, 256: 2, 257: 3}
    for sym in (0, 65, 65, 65, 65):
        w.code(lit[sym], 2)
    w.code(lit[257], 2)  # a match of 3 ...
    w.code(0, 1)         # ... at distance symbol 4 (5 + one extra bit of 0): the row above
    w.bits(0, 1)
    w.code(lit[65], 2)
    w.code(lit[65], 2)
    w.code(lit[256], 2)
    out = b"\x78\x9c" + w.finish() + struct.pack(">I", zlib.adler32(raw))
    assert zlib.decompress(out) == raw
    return out


def png(w, h, ctype, depth, rows, filters=(0,), stream=None, plte=None, trns=None, before=(), between=(), after=(), split=None,
        interlace=0, **z):
    """rows: uint8 [h, rowbytes] of packed samples.  before / between / after: raw chunks around and between the IDAT chunks;
    split: sizes of the IDAT chunks in turn (the last takes the rest)"""
    bits = depth * CHANNELS[ctype]
    bpp = max(1, bits // 8)
    if stream is None:
        stream = deflate(scanlines(rows, filters, bpp), **z)
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))]
    out += list(before)
    if plte is not None:
        out.append(chunk(b"PLTE", bytes(plte)))
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    parts, at = [], 0
    for n in (split or []):
        parts.append(stream[at:at + n])
        at += n
    parts.append(stream[at:])
    for k, p in enumerate(parts):
        out.append(chunk(b"IDAT", p))
        if k < len(between):
            out.append(between[k])
    out += list(after)
    out.append(chunk(b"IEND"))
    return b"".join(out)


def smooth(rng, h, w, c):
    """natural-image-like smooth noise, uint8 [h, w, c]"""
    x = rng.standard_normal((h + 8, w + 8, c)).cumsum(0).cumsum(1)
    x = x[8:, 8:] - x[:-8, 8:] - x[8:, :-8] + x[:-8, :-8]
    x = (x - x.min()) / max(float(x.max() - x.min()), 1e-9)
    return (x * 255 + rng.integers(0, 3, x.shape)).clip(0, 255).astype(np.uint8)


def pack_bits(idx, depth):
    """uint8 [h, w] of values below 2^depth -> uint8 [h, ceil(w * depth / 8)], leftmost pixel in the high bits"""
    h, w = idx.shape
    per = 8 // depth
    pad = (-w) % per
    v = np.pad(idx, ((0, 0), (0, pad))).reshape(h, -1, per).astype(np.uint32)
    shifts = np.array([8 - depth * (k + 1) for k in range(per)], np.uint32)
    return (v << shifts).sum(-1).astype(np.uint8)


def rows_of(img, depth=8):
    """uint8 / uint16 [h, w, c] samples -> packed rows (16-bit big-endian)"""
    h = img.shape[0]
    if depth == 16:
        return img.astype(">u2").reshape(h, -1).view(np.uint8).reshape(h, -1)
    return img.reshape(h, -1).astype(np.uint8)


def corpus():
    rng = np.random.default_rng(20261021)
    files = {}
    text = chunk(b"tEXt", b"Comment\x00made by tools/make_png_golden.py")
    # every accepted colour type and depth, each with a per-row mix of filter types
    mix = (0, 1, 2, 3, 4, 4, 3, 2, 1, 0)
    files["rgb8"] = png(13, 11, 2, 8, rows_of(smooth(rng, 11, 13, 3)), mix)
    files["rgba8"] = png(13, 11, 6, 8, rows_of(smooth(rng, 11, 13, 4)), mix)
    files["gray8"] = png(13, 11, 0, 8, rows_of(smooth(rng, 11, 13, 1)), mix)
    files["graya8"] = png(13, 11, 4, 8, rows_of(smooth(rng, 11, 13, 2)), mix)
    files["rgb16"] = png(9, 7, 2, 16, rows_of(rng.integers(0, 65536, (7, 9, 3)).astype(np.uint16), 16), mix)
    files["rgba16"] = png(9, 7, 6, 16, rows_of(rng.integers(0, 65536, (7, 9, 4)).astype(np.uint16), 16), mix)
    for depth, w in ((1, 13), (2, 7), (4, 5), (1, 8), (2, 4), (4, 2)):  # packed rows that are and are not whole bytes
        idx = rng.integers(0, 1 << depth, (9, w)).astype(np.uint8)
        files[f"gray{depth}_w{w}"] = png(w, 9, 0, depth, pack_bits(idx, depth), mix)
        plte = rng.integers(0, 256, 3 << depth).astype(np.uint8)
        files[f"pal{depth}_w{w}"] = png(w, 9, 3, depth, pack_bits(idx, depth), mix, plte=plte)
    idx = rng.integers(0, 256, (9, 17)).astype(np.uint8)
    files["pal8"] = png(17, 9, 3, 8, idx, mix, plte=rng.integers(0, 256, 768).astype(np.uint8))
    # tRNS on gray, RGB and palette; a short palette (every index within it)
    files["gray8_trns"] = png(13, 11, 0, 8, rows_of(smooth(rng, 11, 13, 1)), mix, trns=b"\x00\x40")
    files["rgb8_trns"] = png(13, 11, 2, 8, rows_of(smooth(rng, 11, 13, 3)), mix, trns=b"\x00\x10\x00\x20\x00\x30")
    files["pal8_trns"] = png(17, 9, 3, 8, idx % 5, mix, plte=rng.integers(0, 256, 15).astype(np.uint8), trns=bytes([0, 128, 255]))
    files["pal4_short"] = png(5, 9, 3, 4, pack_bits((idx[:, :5] % 3).astype(np.uint8), 4), mix, plte=rng.integers(0, 256, 9).astype(np.uint8))
    # each filter type alone, and the per-row heuristic
    img = smooth(rng, 12, 19, 3)
    for ft in range(5):
        files[f"filter{ft}"] = png(19, 12, 2, 8, rows_of(img), (ft,))
    files["filter_heur"] = png(19, 12, 2, 8, rows_of(img), "heur")
    files["filter_odd_one"] = png(19, 12, 2, 8, rows_of(img), (4, 4, 4, 1, 4, 4, 4, 4, 0, 4, 4, 4))
    # every deflate strategy
    img = smooth(rng, 40, 33, 3)
    flat = np.repeat(rng.integers(0, 256, (40, 3, 3)).astype(np.uint8), 11, axis=1)  # runs: distance-1 and distance-3 matches
    files["z_stored"] = png(33, 40, 2, 8, rows_of(img), mix, level=0)
    files["z_fixed"] = png(33, 40, 2, 8, rows_of(img), mix, strategy=zlib.Z_FIXED)
    files["z_huffman"] = png(33, 40, 2, 8, rows_of(img), mix, strategy=zlib.Z_HUFFMAN_ONLY)
    files["z_rle"] = png(33, 40, 0, 8, rows_of(np.repeat(rng.integers(0, 256, (40, 3, 1)).astype(np.uint8), 11, axis=1)), (0,),
                         strategy=zlib.Z_RLE)
    files["z_rle_rgb"] = png(33, 40, 2, 8, rows_of(flat), (0, 1), strategy=zlib.Z_RLE)
    files["z_level9"] = png(33, 40, 2, 8, rows_of(img), "heur", level=9)
    files["z_wbits9"] = png(33, 40, 2, 8, rows_of(img), mix, level=9, wbits=9)
    # above 32 KiB of raster, rows repeating: matches at the full distance of 32768, the window wraps (stride 256, period 128 rows)
    period = rng.integers(0, 256, (128, 255)).astype(np.uint8)
    big = np.concatenate([period, period, period[:14]])
    files["far_32768"] = png(255, 270, 0, 8, big, stream=deflate_far(scanlines(big, (0,), 1)))
    files["cross_repeat"] = png(4, 2, 0, 8, None, stream=deflate_cross())
    files["big_level9"] = png(255, 270, 0, 8, big, (0, 2), level=9)
    # chunk framing: many small IDAT chunks, one of them empty; ancillary chunks before the IDAT chunks and behind them
    img = smooth(rng, 21, 17, 3)
    files["idat_split"] = png(17, 21, 2, 8, rows_of(img), mix, split=[1, 1, 0, 2, 7, 64, 3])
    files["ancillary"] = png(17, 21, 2, 8, rows_of(img), mix, split=[100],
                             before=[chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"sRGB", b"\x00"),
                                     chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)), text, chunk(b"prVt", b"unknown")],
                             after=[text, chunk(b"tIME", struct.pack(">HBBBBB", 2026, 10, 21, 0, 0, 0))])
    files["iccp"] = png(17, 21, 2, 8, rows_of(img), mix, before=[chunk(b"iCCP", b"x\x00\x00" + zlib.compress(b"\x00" * 128))])
    # sizes: 1x1, 1xN, Nx1, and around the unfilter kernel's row band (64) and column tile (384 bytes: 128 RGB pixels, 384 gray)
    files["s1x1"] = png(1, 1, 2, 8, rows_of(smooth(rng, 1, 1, 3)), (4,))
    files["s1x70"] = png(1, 70, 2, 8, rows_of(smooth(rng, 70, 1, 3)), mix)
    files["s300x1"] = png(300, 1, 2, 8, rows_of(smooth(rng, 1, 300, 3)), (3,))
    for h in (63, 64, 65):
        files[f"h{h}"] = png(7, h, 2, 8, rows_of(smooth(rng, h, 7, 3)), (4, 3, 2, 1, 0, 4, 3))
    for w in (127, 128, 129):
        files[f"w{w}"] = png(w, 5, 2, 8, rows_of(smooth(rng, 5, w, 3)), (1, 4, 3, 2, 0))
    for w in (383, 384, 385):
        files[f"gray_w{w}"] = png(w, 3, 0, 8, rows_of(smooth(rng, 3, w, 1)), (4, 3, 1))
    files["band_tile"] = png(130, 66, 6, 8, rows_of(smooth(rng, 66, 130, 4)), "heur")
    files["rgba16_tile"] = png(50, 5, 6, 16, rows_of(rng.integers(0, 65536, (5, 50, 4)).astype(np.uint16), 16), (4, 3, 1, 2, 0))
    files["mid_150x210"] = png(150, 210, 2, 8, rows_of(smooth(rng, 210, 150, 3)), "heur")
    # saved by Pillow itself
    from PIL import Image
    for name, arr, mode in (("pil_rgb", smooth(rng, 45, 60, 3), "RGB"), ("pil_gray", smooth(rng, 31, 29, 1)[..., 0], "L"),
                            ("pil_rgba", smooth(rng, 20, 33, 4), "RGBA")):
        f = io.BytesIO()
        Image.fromarray(arr, mode).save(f, format="PNG")
        files[name] = f.getvalue()
    f = io.BytesIO()
    Image.fromarray(smooth(rng, 24, 24, 3), "RGB").quantize(16).save(f, format="PNG")
    files["pil_palette"] = f.getvalue()
    return files


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    import PIL
    files = corpus()
    names = sorted(files)
    arrays = {"names": np.array(names), "pillow": np.array(PIL.__version__)}
    for n in names:
        arrays["file_" + n] = np.frombuffer(files[n], np.uint8)
        arrays["rgb_" + n] = pil_rgb(files[n])
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(names)} files, {sum(len(files[n]) for n in names)} bytes of PNG, {os.path.getsize(OUT)} on disk")
    if "--dump" in sys.argv:
        d = sys.argv[sys.argv.index("--dump") + 1]
        os.makedirs(d, exist_ok=True)
        for n in names:
            with open(os.path.join(d, n + ".png"), "wb") as f:
                f.write(files[n])


if __name__ == "__main__":
    main()
