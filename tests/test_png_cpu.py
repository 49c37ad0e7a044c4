"""CPU side of the PNG decode (madtp_amd/png.py, csrc/madtp_png.h): the restatement of tests/png_ref.py against Pillow, the host
stage against the restatement, the kernels' routines run on the host (madtp_png_inflate_host, madtp_png_unfilter_host) against zlib
and Pillow's recorded bytes, every malformed and refused case by its code, truncations and byte flips against zlib, the header
against the binding, and the batch plan."""
import ctypes
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

from madtp_amd import abi
from tests import png_ref
from tests.png_ref import BitWriter, build, chunk, ihdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = png_ref.corpus()
NAMES = sorted(CORPUS)
CANARY = 64


@pytest.fixture(scope="module")
def png():
    from madtp_amd import build as _build, png as module
    _build.build(verbose=False)
    module.lib()
    return module


def _inflate(png, stream, raw_bytes, rowbytes=0):
    """madtp_png_inflate_host into a buffer with canaries on both sides -> (code, raw bytes, status); the canaries must be intact"""
    s = np.frombuffer(bytes(stream), np.uint8)
    buf = np.full(raw_bytes + 2 * CANARY, 0xA5, np.uint8)
    status = np.zeros(png.STATUS_FIELDS, np.int32)
    rc = png.lib().madtp_png_inflate_host(s.ctypes.data if s.size else buf.ctypes.data, s.size, buf.ctypes.data + CANARY, raw_bytes, rowbytes,
                                          status.ctypes.data)
    assert (buf[:CANARY] == 0xA5).all() and (buf[CANARY + raw_bytes:] == 0xA5).all(), "a write outside the image's extent"
    assert rc == status[0]
    return rc, buf[CANARY:CANARY + raw_bytes].tobytes(), status


def _zlib_accepts(stream, raw_bytes):
    """what the rule of the device route is measured against: zlib.decompress accepts, with the right length -> the bytes, else None"""
    try:
        raw = zlib.decompress(bytes(stream))
    except zlib.error:
        return None
    return raw if len(raw) == raw_bytes else None


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------
def test_corpus_holds_what_it_must():
    """a corpus without these proves nothing: all five filter types, all three block types, a match at distance 1 and one at 32768,
    an overlapping match, a repeat code across the literal / distance boundary, a code longer than the fast tables look (10 bits),
    every accepted colour type and depth"""
    filters, types, distances, overlaps, cross, formats, longest = set(), set(), set(), 0, False, set(), 0
    for name in NAMES:
        p = png_ref.parse(CORPUS[name][0])
        raw = zlib.decompress(p["stream"])
        filters |= set(raw[::1 + p["rowbytes"]])
        s = png_ref.deflate_stats(p["stream"])
        assert s["produced"] == p["raw_bytes"], name
        types |= s["types"]
        distances |= s["distances"]
        overlaps += s["overlaps"]
        cross = cross or s["cross"]
        longest = max(longest, s["longest"])
        formats.add((p["color"], p["depth"]))
    assert filters == {0, 1, 2, 3, 4} and types == {0, 1, 2}
    assert 1 in distances and 32768 in distances and overlaps > 0 and cross and longest > 10
    assert formats == {(2, 8), (6, 8), (0, 8), (4, 8), (0, 1), (0, 2), (0, 4), (3, 1), (3, 2), (3, 4), (3, 8), (2, 16), (6, 16)}
    assert sum(len(CORPUS[n][0]) for n in NAMES) < 400_000 and os.path.getsize(png_ref.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow_live_and_recorded(name):
    from PIL import Image
    data, recorded = CORPUS[name]
    mine = png_ref.decode(data)
    assert mine.dtype == np.uint8 and np.array_equal(mine, recorded)
    assert np.array_equal(mine, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))


@pytest.mark.parametrize("name", NAMES)
def test_host_stage_and_emulation_equal_the_restatement(png, name):
    data, recorded = CORPUS[name]
    p = png_ref.parse(data)
    info = png.inspect(data)
    im = png.prepare(data)
    for k in "width height depth color channels rowbytes bpp raw_bytes".split():
        assert getattr(info, k) == getattr(im, k) == p[k], k
    assert info.stream_bytes == im.stream_bytes == len(p["stream"]) and info.palette_entries == p["entries"]
    assert im.stream.tobytes() == p["stream"] and np.array_equal(im.palette, p["palette"])
    want = zlib.decompress(p["stream"])
    rc, raw, status = _inflate(png, im.stream, im.raw_bytes, im.rowbytes)
    assert rc == 0 and raw == want
    assert status[png._S["BYTES"]] == len(want) and int(status[png._S["ADLER"]]) & 0xffffffff == zlib.adler32(want)
    assert status[png._S["BLOCKS"]] >= 1
    rc, rgb = png.unfilter_host(np.frombuffer(raw, np.uint8), im.width, im.height, im.depth, im.color, im.palette)
    assert rc == 0 and np.array_equal(rgb, recorded)


def test_pickled_image_is_the_image(png):
    import pickle
    im = png.read(CORPUS["pal8_trns"][0])
    back = pickle.loads(pickle.dumps(im))
    assert all(np.array_equal(getattr(im, k), getattr(back, k)) for k in im.__slots__)


# ---- malformed streams, one per reason ------------------------------------------------------------------------------------------------
RAW = bytes([0, 10, 20, 30, 1, 1, 1, 1, 2, 5, 5, 5])  # 3 x 3 gray: filters 0, 1, 2
GOOD = zlib.compress(RAW)


def _streams():
    e = {}
    e["ZLIB_HEADER"] = [b"\x77\x9c" + GOOD[2:], b"\x88\x1c" + GOOD[2:], b"\x78\x9d" + GOOD[2:]]  # not deflate; a 64 KiB window; the check
    e["DICT"] = [b"\x78\x20" + GOOD[2:]]
    e["BLOCK_TYPE"] = [BitWriter().bits(1, 1).bits(3, 2).done()]
    e["STORED"] = [b"\x78\x9c\x01\x0c\x00\xf3\xfe" + RAW + struct.pack(">I", zlib.adler32(RAW))]
    over = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(15, 4)
    for _ in range(19):
        over.bits(1, 3)  # nineteen codes of one bit
    lone = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4).bits(1, 3).bits(0, 9)  # one code-length code of one bit
    many = BitWriter().bits(1, 1).bits(2, 2).bits(30, 5).bits(0, 5).bits(0, 4)  # 287 literal / length codes
    norepeat = BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4).bits(1, 3).bits(1, 3).bits(0, 6).code(0, 1).bits(0, 2)
    e["LENGTHS"] = [over.done(), lone.done(), many.bits(0, 64).done(), norepeat.bits(0, 64).done()]
    e["SYMBOL"] = [BitWriter().bits(1, 1).bits(1, 2).fixed(286).fixed(256).done(),                        # a length symbol that is none
                   BitWriter().bits(1, 1).bits(1, 2).fixed(0).fixed(257).code(30, 5).fixed(256).done()]  # a distance symbol that is none
    e["DISTANCE"] = [BitWriter().bits(1, 1).bits(1, 2).fixed(0).fixed(257).code(1, 5).fixed(256).done()]  # 2 back after 1 byte
    e["SIZE"] = [zlib.compress(RAW + b"\x00"), zlib.compress(RAW[:-1]), zlib.compress(RAW * 2, 0)]
    e["TRUNCATED"] = [GOOD[:-1], GOOD[:-4], GOOD[:5], GOOD[:2], GOOD[:1], b""]
    e["ADLER"] = [GOOD[:-1] + bytes([GOOD[-1] ^ 1])]
    bad = bytearray(RAW)
    bad[4] = 5
    e["FILTER"] = [zlib.compress(bytes(bad))]
    return [(k, i, s) for k, v in e.items() for i, s in enumerate(v)]


@pytest.mark.parametrize("reason,i,stream", _streams(), ids=[f"{k}-{i}" for k, i, _ in _streams()])
def test_malformed_streams_give_their_code(png, reason, i, stream):
    rc, _, status = _inflate(png, stream, len(RAW), 3)
    assert rc == png.E[reason]
    if reason != "FILTER":  # (zlib knows nothing of filter bytes)
        assert _zlib_accepts(stream, len(RAW)) is None
    assert _inflate(png, GOOD, len(RAW), 3)[:2] == (0, RAW)


def test_malformed_files_give_their_code(png):
    idat, head = chunk(b"IDAT", GOOD), ihdr(3, 3, 8, 0)
    good = build(head, idat)
    assert png.prepare(good).stream.tobytes() == GOOD
    cases = {
        "SIGNATURE": [b"\x88" + good[1:], good[:7], b""],
        "NO_IHDR": [build(chunk(b"tEXt", b"a\x00b"), head, idat), build(chunk(b"IHDR", b"\x00" * 12), idat)],
        "NO_PLTE": [build(ihdr(3, 3, 8, 3), idat), build(ihdr(3, 3, 8, 3), idat, chunk(b"PLTE", b"\x00" * 6))],
        "NO_IDAT": [build(head)],
        "CHUNK": [good[:-12], good[:-1], good[:30], png_ref.SIGNATURE + head + struct.pack(">I", 1 << 20) + idat[4:] + chunk(b"IEND"),
                  png_ref.SIGNATURE + head + struct.pack(">I", 0xffffffff) + idat[4:] + chunk(b"IEND")],
        "HEADER": [build(ihdr(0, 3, 8, 0), idat), build(ihdr(3, 3, 8, 0, compression=1), idat), build(ihdr(3, 3, 8, 0, interlace=2), idat),
                   build(ihdr(3, 3, 8, 3), chunk(b"PLTE", b"\x00" * 7), idat), build(head, head, idat)],
        "IDAT_ORDER": [build(head, chunk(b"IDAT", GOOD[:5]), chunk(b"tEXt", b"a\x00b"), chunk(b"IDAT", GOOD[5:]))],
    }
    for reason, files in cases.items():
        for k, f in enumerate(files):
            with pytest.raises(png.CorruptPng, match=rf"code {png.E[reason]}\b"):
                png.prepare(f)
            with pytest.raises(png.CorruptPng):
                png.read(f, other="pil")  # a corrupt file raises either way
    # a flipped IDAT CRC byte still decodes (Pillow does not verify it either)
    flipped = bytearray(good)
    flipped[-13] ^= 0xff
    assert png.prepare(bytes(flipped)).stream.tobytes() == GOOD


def test_every_unsupported_reason_is_raised_by_name(png):
    idat = chunk(b"IDAT", GOOD)
    cases = {
        "INTERLACE": [build(ihdr(3, 3, 8, 0, interlace=1), idat)],
        "GRAY16": [build(ihdr(3, 3, 16, 0), idat), build(ihdr(3, 3, 16, 4), idat)],
        "APNG": [build(ihdr(3, 3, 8, 0), chunk(b"acTL", struct.pack(">II", 2, 0)), idat),
                 build(ihdr(3, 3, 8, 0), idat, chunk(b"fdAT", b"\x00" * 4 + GOOD))],
        "SIDE": [build(ihdr(8193, 3, 8, 0), idat), build(ihdr(3, 1 << 31, 8, 0), idat)],
        "COLOR_DEPTH": [build(ihdr(3, 3, 4, 2), idat), build(ihdr(3, 3, 16, 3), idat), build(ihdr(3, 3, 8, 1), idat), build(ihdr(3, 3, 3, 0), idat),
                        build(ihdr(3, 3, 2, 6), idat), build(ihdr(3, 3, 1, 4), idat)],
    }
    for reason, files in cases.items():
        for f in files:
            with pytest.raises(png.UnsupportedPng, match=rf"code {png.E[reason]}\b"):
                png.read(f)
    # other="pil": Pillow's decode of a refused file, as preprocess.raw_image makes it
    from PIL import Image
    gray16 = build(ihdr(1, 4, 16, 0), chunk(b"IDAT", zlib.compress(bytes([0, 0, 7] * 4))))
    out = png.read(gray16, other="pil")
    assert np.array_equal(np.asarray(out), np.asarray(Image.open(io.BytesIO(gray16)).convert("RGB")))
    with pytest.raises(ValueError):
        png.read(gray16, other="skip")


def test_a_palette_index_beyond_plte_is_black_as_in_pillow(png):
    from PIL import Image
    idx = bytes([0, 0, 1, 2, 200, 255])
    f = build(ihdr(5, 1, 8, 3), chunk(b"PLTE", bytes([10, 20, 30, 40, 50, 60])), chunk(b"IDAT", zlib.compress(idx)))
    pil = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
    assert pil[0].tolist() == [[10, 20, 30], [40, 50, 60], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    im = png.prepare(f)
    assert im.palette_entries == 2 and np.array_equal(png_ref.decode(f), pil)
    rc, rgb = png.unfilter_host(np.frombuffer(idx, np.uint8), 5, 1, 8, 3, im.palette)
    assert rc == 0 and np.array_equal(rgb, pil)


# ---- truncations and flips: the emulation against zlib -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rgb8", "z_fixed", "z_stored"])
def test_every_truncation_errs(png, name):
    data = CORPUS[name][0]
    for n in range(len(data)):
        with pytest.raises(png.CorruptPng):
            png.prepare(data[:n])
    im = png.prepare(data)
    stream = im.stream.tobytes()
    for n in range(len(stream)):
        rc, _, _ = _inflate(png, stream[:n], im.raw_bytes, im.rowbytes)
        assert -300 < rc <= -200 and _zlib_accepts(stream[:n], im.raw_bytes) is None, n


@pytest.mark.parametrize("name", ["rgb8", "z_fixed", "z_stored", "z_rle", "z_huffman", "cross_repeat", "filter_heur", "pal4_w5", "z_wbits9"])
def test_seeded_flips_err_or_succeed_as_zlib_does(png, name):
    im = png.prepare(CORPUS[name][0])
    stream = im.stream.tobytes()
    rng = np.random.default_rng(sum(name.encode()))
    accepted = 0
    for _ in range(400):
        s = bytearray(stream)
        for _ in range(int(rng.integers(1, 3))):
            s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
        want = _zlib_accepts(s, im.raw_bytes)
        rc, raw, _ = _inflate(png, s, im.raw_bytes)  # (no rowbytes: the filter bytes are not zlib's to check)
        if want is None:
            assert -300 < rc <= -200, bytes(s).hex()
        else:
            accepted += 1
            assert rc == 0 and raw == want, bytes(s).hex()
    assert accepted < 400  # (most flips are caught by the checksum, if by nothing else)


def test_unfilter_emulation_refuses_a_filter_byte_above_4(png):
    bad = np.frombuffer(RAW, np.uint8).copy()
    bad[8] = 5
    assert png.unfilter_host(bad, 3, 3, 8, 0, np.zeros(768, np.uint8))[0] == png.E["FILTER"]
    with pytest.raises(ValueError):
        png.unfilter_host(bad[:-1], 3, 3, 8, 0, np.zeros(768, np.uint8))


# ---- the header, the binding, the library ----------------------------------------------------------------------------------------------
def png_header():
    return os.path.join(ROOT, "madtp_amd", "csrc", "madtp_png.h")


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(png_header()).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))


def test_symbols_are_exported_and_the_other_abis_are_unchanged(png):
    from madtp_amd import augment, build as _build, hip, jpeg, jpeg_device, lists, preprocess, search
    raw = ctypes.CDLL(_build.build(verbose=False))
    syms = _header_symbols()
    assert syms == sorted(png.SIGNATURES) == sorted(
        "madtp_png_" + s for s in "abi_version strerror prepare rowbytes raw_bytes carry_bytes inflate_batch unfilter_batch inflate_host "
                                  "unfilter_host".split())
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in csrc/madtp_png.h but not exported"
    lib = png.lib()
    assert lib.madtp_png_abi_version() == png.ABI_VERSION == 1
    for name, (res, args) in png.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_void_p, c_int64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert png.SIGNATURES["madtp_png_prepare"] == (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64])
    assert png.SIGNATURES["madtp_png_inflate_batch"] == (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p])
    assert png.SIGNATURES["madtp_png_unfilter_batch"] == (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p])
    assert png.SIGNATURES["madtp_png_inflate_host"] == (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p])
    assert (png.FIELDS, png.INFO_FIELDS, png.STATUS_FIELDS, png.MAX_SIDE, png.BAND, png.TILE) == (16, 16, 4, 8192, 64, 384)
    assert sorted(png._F.values()) == list(range(11)) and sorted(png._I.values()) == list(range(10)) and sorted(png._S.values()) == [0, 1, 2, 3]
    assert len(set(png.E.values())) == len(png.E) == 23 and all(lib.madtp_png_strerror(c) for c in png.E.values())
    # the eight other headers
    assert len(abi.SIGNATURES) == 97 and not set(abi.SIGNATURES) & set(syms)
    assert hip.ABI_VERSION == 31 == raw.madtp_abi_version()
    versions = {"madtp_image_abi_version": preprocess.ABI_VERSION, "madtp_augment_abi_version": augment.ABI_VERSION,
                "madtp_search_abi_version": search.ABI_VERSION, "madtp_csearch_abi_version": search.COARSE_ABI_VERSION,
                "madtp_jpeg_abi_version": jpeg.ABI_VERSION, "madtp_jhuff_abi_version": jpeg_device.ABI_VERSION,
                "madtp_lists_abi_version": lists.ABI_VERSION}
    for symbol, bound in versions.items():
        assert getattr(raw, symbol)() == bound == 1, symbol
    assert "png.hip" in _build.SOURCES and "png_device.h" in _build.HEADERS and "madtp_png.h" in _build.HEADERS


def test_entry_points_refuse_before_any_launch(png):
    lib = png.lib()
    bad = abi.DEFINES["MADTP_E_BADARG"]
    assert lib.madtp_png_inflate_batch(None, 16, 16, 16, 1, None) == bad and lib.madtp_png_inflate_batch(16, 16, 16, 16, 0, None) == bad
    assert lib.madtp_png_unfilter_batch(16, None, 16, 16, 1, None) == bad and lib.madtp_png_unfilter_batch(16, 16, 16, 16, 0, None) == bad
    info, pal = np.zeros(16, np.int32), np.zeros(768, np.uint8)
    assert lib.madtp_png_prepare(None, 0, info.ctypes.data, pal.ctypes.data, None, 0) == bad
    data = np.frombuffer(CORPUS["rgb8"][0], np.uint8)
    small = np.full(8, 0xA5, np.uint8)
    assert lib.madtp_png_prepare(data.ctypes.data, data.size, info.ctypes.data, pal.ctypes.data, small.ctypes.data, 4) == bad
    assert (small == 0xA5).all() and info[png._I["WIDTH"]] == 13
    assert lib.madtp_png_rowbytes(13, 1, 0) == 2 and lib.madtp_png_rowbytes(13, 16, 6) == 104 and lib.madtp_png_rowbytes(13, 16, 0) == 0
    assert lib.madtp_png_raw_bytes(8192, 8192, 16, 6) == 8192 * 65537 and lib.madtp_png_raw_bytes(8193, 1, 8, 2) == 0
    assert lib.madtp_png_carry_bytes(7) == 112 and lib.madtp_png_carry_bytes(0) == 0


def test_decoder_needs_a_gpu_and_checks_its_arguments(png, monkeypatch):
    import torch
    with pytest.raises(ValueError):
        png.PngDecoder(inflate="gpu")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for route in ("host", "device"):
        with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
            png.PngDecoder(inflate=route)([CORPUS["rgb8"][0]])
    with pytest.raises(ValueError):
        png.PngDecoder()([])
    with pytest.raises(png.CorruptPng, match="image 1"):
        png.PngDecoder()([CORPUS["rgb8"][0], CORPUS["rgb8"][0][:40]])


# ---- the batch plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_batch_plan_regions_and_alignments(png, route):
    names = ["rgb8", "pal4_w5", "mid_150x210", "rgba16", "s1x1"]
    ims = [png.prepare(CORPUS[n][0]) for n in names]
    items = [("coded", ims[0]), ("raw", (5, 7, 3)), ("coded", ims[1]), ("coded", ims[2]), ("raw", (2, 3, 3)), ("coded", ims[3]), ("coded", ims[4])]
    plan = png.plan_batch(items, route)
    F = png._F
    assert plan.B == 7 and plan.coded == [0, 2, 3, 5, 6] and plan.table.shape == (5, png.FIELDS)
    assert plan.head.size == plan.table_bytes + 768 * 5 and plan.palette_at == plan.table_bytes
    assert np.array_equal(plan.head[:plan.table_bytes].view(np.int64).reshape(5, -1), plan.table)
    spans = []  # (begin, end) of everything that lies in the buffer: nothing overlaps, everything lies where its region is
    for k, im in enumerate(ims):
        row = plan.table[k]
        assert (row[F["W"]], row[F["H"]], row[F["DEPTH"]], row[F["COLOR"]]) == (im.width, im.height, im.depth, im.color)
        assert row[F["RAW_BYTES"]] == im.raw_bytes and row[F["STREAM_BYTES"]] == im.stream_bytes
        assert row[F["PALETTE"]] == plan.palette_at + 768 * k
        assert row[F["RAW"]] % 256 == 0 and row[F["OUT"]] % 16 == 0 and row[F["CARRY"]] % 16 == 0
        spans.append((row[F["RAW"]], row[F["RAW"]] + im.raw_bytes))
        spans.append((row[F["OUT"]], row[F["OUT"]] + 3 * im.width * im.height))
        spans.append((row[F["CARRY"]], row[F["CARRY"]] + 16 * im.height))
        assert plan.out_at <= row[F["OUT"]] and row[F["CARRY"]] + 16 * im.height <= plan.total
        if route == "host":
            assert row[F["RAW"]] == plan.payload[k] and plan.head.size <= row[F["RAW"]] and row[F["RAW"]] + im.raw_bytes <= plan.copy_bytes
        else:
            assert row[F["STREAM"]] == plan.payload[k] and row[F["STREAM"]] % 256 == 0
            assert plan.head.size <= row[F["STREAM"]] and row[F["STREAM"]] + im.stream_bytes <= plan.copy_bytes
            assert plan.raw_at <= row[F["RAW"]] and row[F["RAW"]] + im.raw_bytes <= plan.out_at
            spans.append((row[F["STREAM"]], row[F["STREAM"]] + im.stream_bytes))
    for i, ((hh, ww), o) in enumerate(plan.shapes):
        if items[i][0] == "raw":
            assert (hh, ww) == items[i][1][:2] and o % 16 == 0 and plan.head.size <= o and o + 3 * hh * ww <= plan.copy_bytes
            spans.append((o, o + 3 * hh * ww))
        else:
            k = plan.coded.index(i)
            assert (hh, ww) == (ims[k].height, ims[k].width) and o == plan.table[k, F["OUT"]]
    spans.sort()
    assert spans[0][0] >= plan.head.size and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= plan.total
    assert plan.copy_bytes <= plan.raw_at <= plan.out_at <= plan.total and plan.raw_at % 256 == 0 and plan.out_at % 256 == 0
    # prefix sums: every region follows the one before it
    assert all(plan.payload[k] < plan.payload[k + 1] for k in range(4))
    assert all(plan.table[k, F["OUT"]] < plan.table[k + 1, F["OUT"]] and plan.table[k, F["CARRY"]] < plan.table[k + 1, F["CARRY"]] for k in range(4))


def test_batch_plan_refuses_contradictions(png):
    im = png.prepare(CORPUS["rgb8"][0])
    im.rowbytes += 1
    with pytest.raises(ValueError, match="image 1"):
        png.plan_batch([("raw", (2, 2, 3)), ("coded", im)])
    with pytest.raises(ValueError):
        png.plan_batch([], "pillow")
    only_raw = png.plan_batch([("raw", (2, 2, 3))])
    assert only_raw.coded == [] and only_raw.copy_bytes == only_raw.shapes[0][1] + 12
