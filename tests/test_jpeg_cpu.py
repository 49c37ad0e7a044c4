"""The host side of the JPEG decode (madtp_amd/jpeg.py, csrc/jpeg_entropy.h) without a GPU: tests/jpeg_ref.py - the whole decode
restated in numpy - against Pillow's pixels (recorded in tests/golden/jpeg_pil.npz, and live where Pillow is installed); the host
entropy decoder through ctypes against the restatement's coefficients and header; every refusal and every kind of malformed stream,
decoded into buffers with guard bytes; the binding against include/madtp_jpeg.h.  Every compare is exact."""
import ctypes
import functools
import io
import os
import pickle
import re

import numpy as np
import pytest
import torch

from madtp_amd import abi, hip, jpeg, preprocess
from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")
GUARD = 4096
SIZES = ["1x1", "5x3", "3x5", "8x9", "17x4", "2x70", "16x16", "33x31", "37x53", "48x64", "150x210"]


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def names():
    return [str(n) for n in golden()["names"]]


def data(name):
    return golden()["jpg_" + name].tobytes()


def by_prefix(prefix):
    return data(next(n for n in names() if n.startswith(prefix)))


@functools.lru_cache(maxsize=None)
def restated(name):
    """(header, coefficients, pixels) of the restatement (computed once, shared, never written)"""
    h, coef = jpeg_ref.entropy(data(name))
    return h, coef, jpeg_ref.decode_coefficients(h, coef)


def guarded_decode(raw):
    """the two host calls on exact-size copies, the outputs between guard bytes -> (code, info, coefficients or None)"""
    lib = jpeg.lib()
    buf = np.frombuffer(bytes(raw), dtype=np.uint8).copy()
    info = np.full(jpeg.INFO_FIELDS + 2 * 64, 0x5A5A5A5A, dtype=np.int32)
    q = np.full(3 * 64 + 2 * 64, 0xA5A5, dtype=np.uint16)
    rc = lib.madtp_jpeg_inspect(buf.ctypes.data, buf.size, info[64:].ctypes.data, q[64:].ctypes.data)
    assert (info[:64] == 0x5A5A5A5A).all() and (info[64 + jpeg.INFO_FIELDS:] == 0x5A5A5A5A).all()
    assert (q[:64] == 0xA5A5).all() and (q[64 + 192:] == 0xA5A5).all()
    if rc:
        return rc, None, None
    fields = info[64:64 + jpeg.INFO_FIELDS]
    n = 64 * int(fields[jpeg._I["BLOCKS"]])
    out = np.full(n + 2 * GUARD, 0x7B7B, dtype=np.int16)
    rc = lib.madtp_jpeg_entropy_decode(buf.ctypes.data, buf.size, out[GUARD:].ctypes.data, n)
    assert (out[:GUARD] == 0x7B7B).all() and (out[GUARD + n:] == 0x7B7B).all(), "a write outside the given buffer"
    return rc, fields, out[GUARD:GUARD + n] if rc == 0 else None


def segments(raw):
    """[(marker, offset of the FF, total bytes with the marker)] up to and including SOS"""
    out, p = [], 2
    while True:
        m, n = raw[p + 1], raw[p + 2] << 8 | raw[p + 3]
        out.append((m, p, n + 2))
        p += n + 2
        if m == 0xDA:
            return out


def segment(raw, marker):
    return next(s for s in segments(raw) if s[0] == marker)


def patched(raw, at, new):
    return raw[:at] + bytes(new) + raw[at + len(bytes(new)):]


# ---- the restatement against Pillow ------------------------------------------------------------------------------------------------
def test_corpus_covers_what_it_must():
    ns = names()
    assert os.path.getsize(GOLDEN) <= 400 * 1024 and len(golden()["pillow"]) == 3
    for size in SIZES:
        for sub in ("444", "422", "420"):
            assert any(n.startswith(f"{size}_{sub}_") for n in ns), (size, sub)
    for tag in ("_q30", "_q85", "_q100", "gray", "restart", "optimize", "qt255", "qt1"):
        assert any(tag in n for n in ns), tag
    for n in ns:
        h = restated(n)[0]
        assert (h["height"], h["width"]) == tuple(map(int, n.split("_")[0].split("x")))
        assert h["components"] == (1 if "gray" in n else 3)
        if "gray" not in n:
            assert (h["hs"], h["vs"]) == {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[n.split("_")[1]]
        assert (h["restart"] > 0) == ("restart" in n)
    # the saturating files do clip on both sides
    assert any(golden()["pix_" + n].min() == 0 and golden()["pix_" + n].max() == 255 for n in ns if "qt255" in n)


@pytest.mark.parametrize("name", names())
def test_restatement_equals_recorded_pillow(name):
    assert np.array_equal(restated(name)[2], golden()["pix_" + name])


def test_restatement_and_fixture_equal_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    for name in names():
        live = np.asarray(Image.open(io.BytesIO(data(name))).convert("RGB"))
        assert np.array_equal(live, golden()["pix_" + name]), f"{name}: the installed Pillow decodes other pixels than the fixture's"
        assert np.array_equal(restated(name)[2], live), name


# ---- the host entropy decoder --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names())
def test_entropy_decoder_equals_restatement(name):
    h, coef, _ = restated(name)
    rc, info, out = guarded_decode(data(name))
    assert rc == 0
    e = jpeg.entropy_decode(data(name))
    assert isinstance(e, jpeg.EntropyImage) and e.coef.dtype == torch.int16 and not e.coef.is_cuda and e.qtables.shape == (3, 64)
    assert np.array_equal(e.coef.numpy().reshape(-1), out)
    got = (e.width, e.height, e.components, e.hs, e.vs, e.blocks_x, e.blocks_y, e.restart_interval)
    assert got == (h["width"], h["height"], h["components"], h["hs"], h["vs"], h["blocks_x"], h["blocks_y"], h["restart"])
    assert np.array_equal(e.qtables.numpy().astype(np.int64), h["qtables"].astype(np.int64))
    assert e.blocks == [c.shape[:2] for c in coef]
    for c in range(e.components):
        assert np.array_equal(e.component(c).numpy(), coef[c]), c
    # column-major within the block: element 8 c + r is the coefficient of row r, column c
    y, x = e.blocks[0]
    assert np.array_equal(e.coef[:y * x].numpy().reshape(y, x, 8, 8), coef[0].transpose(0, 1, 3, 2))


def test_input_kinds_and_pickling(tmp_path):
    raw = by_prefix("37x53_420")
    want = jpeg.entropy_decode(raw)
    path = tmp_path / "a.jpg"
    path.write_bytes(raw)
    for src in (bytearray(raw), memoryview(raw), np.frombuffer(raw, dtype=np.uint8), torch.frombuffer(bytearray(raw), dtype=torch.uint8),
                str(path), path):
        assert torch.equal(jpeg.entropy_decode(src).coef, want.coef)
    assert torch.equal(jpeg.read(path).coef, want.coef)
    again = pickle.loads(pickle.dumps(want))  # what a loader worker does with it
    assert torch.equal(again.coef, want.coef) and again.qtables.dtype == want.qtables.dtype and again.width == 53
    assert np.array_equal(again.qtables.numpy(), want.qtables.numpy())
    with pytest.raises(ValueError, match="not bytes"):
        jpeg.entropy_decode(np.zeros((4, 4, 3), dtype=np.uint8))
    lib = jpeg.lib()
    buf = np.frombuffer(raw, dtype=np.uint8)
    E_BADARG = abi.DEFINES["MADTP_E_BADARG"]
    assert lib.madtp_jpeg_entropy_decode(buf.ctypes.data, buf.size, want.coef.data_ptr(), want.coef.numel() - 1) == E_BADARG
    assert lib.madtp_jpeg_entropy_decode(None, buf.size, want.coef.data_ptr(), want.coef.numel()) == E_BADARG
    assert lib.madtp_jpeg_inspect(buf.ctypes.data, buf.size, None, None) == E_BADARG


def test_fill_bytes_comments_and_16_bit_tables_are_accepted():
    raw = by_prefix("33x31_422")
    want = jpeg.entropy_decode(raw)
    _, at, n = segment(raw, 0xDB)
    com = b"\xff\xfe\x00\x07hello" + b"\xff\xe5\x00\x04ab"
    padded = raw[:at] + com + b"\xff\xff\xff" + raw[at:at + n] + b"\xff" + raw[at + n:-2] + b"\xff\xff" + raw[-2:]
    assert torch.equal(jpeg.entropy_decode(padded).coef, want.coef)
    # the first DQT rewritten with 16-bit entries
    body = raw[at + 4:at + n]
    assert len(body) % 65 == 0
    wide = b"".join(bytes([0x10 | body[i]]) + b"".join(bytes([0, v]) for v in body[i + 1:i + 65]) for i in range(0, len(body), 65))
    raw16 = raw[:at] + b"\xff\xdb" + (len(wide) + 2).to_bytes(2, "big") + wide + raw[at + n:]
    got = jpeg.entropy_decode(raw16)
    assert torch.equal(got.coef, want.coef) and np.array_equal(got.qtables.numpy(), want.qtables.numpy())
    # SOF1 (extended sequential, Huffman) is decoded like SOF0
    _, sof, _ = segment(raw, 0xC0)
    assert torch.equal(jpeg.entropy_decode(patched(raw, sof + 1, [0xC1])).coef, want.coef)
    # a grayscale file is 1x1 whatever its sampling byte says
    gray = by_prefix("33x31_gray")
    _, sof, _ = segment(gray, 0xC0)
    assert torch.equal(jpeg.entropy_decode(patched(gray, sof + 11, [0x22])).coef, jpeg.entropy_decode(gray).coef)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _refusals():
    raw = by_prefix("16x16_444")
    _, sof, _ = segment(raw, 0xC0)
    _, sos, sos_n = segment(raw, 0xDA)
    adobe = lambda t: raw[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t]) + raw[2:]
    cases = {
        "progressive (SOF2)": (patched(raw, sof + 1, [0xC2]), "progressive"),
        "arithmetic (SOF9)": (patched(raw, sof + 1, [0xC9]), "arithmetic"),
        "lossless (SOF3)": (patched(raw, sof + 1, [0xC3]), "SOF2 and up"),
        "12-bit": (patched(raw, sof + 4, [12]), "precision is not 8"),
        "four components": (raw[:sof] + b"\xff\xc0\x00\x14" + raw[sof + 4:sof + 9] + b"\x04" + raw[sof + 10:sof + 19] + b"\x04\x11\x00"
                            + raw[sof + 19:], "component count"),
        "two components": (raw[:sof] + b"\xff\xc0\x00\x0e" + raw[sof + 4:sof + 9] + b"\x02" + raw[sof + 10:sof + 16] + raw[sof + 19:],
                           "component count"),
        "Adobe transform 0": (adobe(0), "Adobe APP14 transform 0"),
        "ids R G B": (patched(patched(patched(raw, sof + 10, b"R"), sof + 13, b"G"), sof + 16, b"B"), "component ids R, G, B"),
        "chroma 2x1": (patched(raw, sof + 14, [0x21]), "chroma sampling is not 1x1"),
        "chroma 1x2 (Cr)": (patched(raw, sof + 17, [0x12]), "chroma sampling is not 1x1"),
        "luma 1x2": (patched(raw, sof + 11, [0x12]), "luma sampling"),
        "luma 4x1": (patched(raw, sof + 11, [0x41]), "luma sampling"),
        "luma 2x4": (patched(raw, sof + 11, [0x24]), "luma sampling"),
        "a scan of one component": (raw[:sos] + b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00" + raw[sos + sos_n:], "more than one scan"),
        "a second scan": (raw[:-2] + raw[sos:sos + sos_n] + raw[-8:], "more than one scan"),
        "DNL": (raw[:sos] + b"\xff\xdc\x00\x04\x00\x10" + raw[sos:], "DNL"),
        "height 0": (patched(raw, sof + 5, [0, 0]), "DNL"),
        "width 8193": (patched(raw, sof + 7, [0x20, 0x01]), "over 8192"),
        "height 9000": (patched(raw, sof + 5, [0x23, 0x28]), "over 8192"),
        "Se 62": (patched(raw, sos + sos_n - 2, [62]), "spectral selection"),
        "Al 1": (patched(raw, sos + sos_n - 1, [0x01]), "successive approximation"),
    }
    return cases


@pytest.mark.parametrize("case", list(_refusals()))
def test_refused_files_name_their_reason(case):
    raw, message = _refusals()[case]
    with pytest.raises(jpeg.UnsupportedJpeg, match=re.escape(message)) as e:
        jpeg.entropy_decode(raw)
    assert "no fallback" in str(e.value)
    rc, _, _ = guarded_decode(raw)
    assert -200 < rc <= -100
    if case != "a second scan":  # (that one shows only behind the first scan) the decoder refuses the batch before it needs a device
        with pytest.raises(jpeg.UnsupportedJpeg, match="image 1"):
            jpeg.JpegDecoder()([by_prefix("8x9_420"), raw])


def test_adobe_ycc_and_gray_adobe_are_accepted():
    raw = by_prefix("16x16_444")
    ycc = raw[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + raw[2:]
    assert torch.equal(jpeg.entropy_decode(ycc).coef, jpeg.entropy_decode(raw).coef)
    gray = by_prefix("33x31_gray")
    g0 = gray[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + gray[2:]
    assert torch.equal(jpeg.entropy_decode(g0).coef, jpeg.entropy_decode(gray).coef)


def test_files_pillow_writes_but_this_decoder_refuses():
    Image = pytest.importorskip("PIL.Image")
    img = Image.fromarray(np.random.RandomState(3).randint(0, 256, (24, 40, 3), dtype=np.uint8))
    buf = io.BytesIO()
    img.save(buf, "JPEG", progressive=True)
    with pytest.raises(jpeg.UnsupportedJpeg, match="progressive"):
        jpeg.read(buf.getvalue())
    got = jpeg.read(buf.getvalue(), other="pil")  # the loud default can be traded for Pillow's decode of a REFUSED file
    assert torch.is_tensor(got) and got.dtype == torch.uint8
    assert np.array_equal(got.numpy(), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")))
    buf = io.BytesIO()
    img.convert("CMYK").save(buf, "JPEG")
    with pytest.raises(jpeg.UnsupportedJpeg, match="component count"):
        jpeg.read(buf.getvalue())
    assert jpeg.read(buf.getvalue(), other="pil").shape == (24, 40, 3)
    with pytest.raises(jpeg.CorruptJpeg):  # ... never for a corrupt one
        jpeg.read(by_prefix("16x16_444")[:-40], other="pil")
    with pytest.raises(ValueError, match="other="):
        jpeg.read(buf.getvalue(), other="quiet")


# ---- malformed streams -------------------------------------------------------------------------------------------------------------
def _code_of(lut, symbol):
    """(code, length) of a symbol in one of the restatement's 16-bit lookup tables"""
    i = next(i for i, e in enumerate(lut) if e is not None and e[1] == symbol)
    return i >> (16 - lut[i][0]), lut[i][0]


def _pack(bits):
    bits += "1" * (-len(bits) % 8)
    out = bytearray()
    for i in range(0, len(bits), 8):
        out.append(int(bits[i:i + 8], 2))
        if out[-1] == 0xFF:
            out.append(0)
    return bytes(out)


def _malformed():
    raw = by_prefix("16x16_444")
    h = jpeg_ref.parse(raw)
    scan = h["scan"]
    _, dqt, dqt_n = segment(raw, 0xDB)
    _, dht, dht_n = segment(raw, 0xC4)
    dc, ac = h["dc"][h["tables"][0][0]], h["ac"][h["tables"][0][1]]
    bits = lambda sym, lut: format(_code_of(lut, sym)[0], f"0{_code_of(lut, sym)[1]}b")
    zrl4 = bits(0, dc) + bits(0xF0, ac) * 4       # four runs of sixteen zeros: index 65
    run = bits(0, dc) + bits(0xF0, ac) * 3 + bits(0xF1, ac) + "1"  # index 49 + 15 = 64 for a coefficient
    restart = by_prefix("37x53_420_q85_restart")
    rs = jpeg_ref.parse(restart)["scan"]
    first_rst = restart.index(b"\xff\xd0", rs)
    second_rst = restart.index(b"\xff\xd1", rs)
    return {
        "no SOI": (b"\x00\x00" + raw[2:], "does not begin with SOI"),
        "empty": (b"", "does not begin with SOI"),
        "SOI alone": (raw[:2], "ends before"),
        "no EOI": (raw[:-2], "ends before"),
        "half the scan": (raw[:(scan + len(raw)) // 2], "ends before"),
        "the header cut inside a segment": (raw[:dqt + 20], "segment length"),
        "all-ones scan": (raw[:scan] + b"\xff\x00" * 64 + b"\xff\xd9", "no Huffman code"),
        "index beyond 63 (runs)": (raw[:scan] + _pack(zrl4) + b"\xff\xd9", "index beyond 63"),
        "index beyond 63 (coefficient)": (raw[:scan] + _pack(run) + b"\xff\xd9", "index beyond 63"),
        "no quantisation table": (raw[:dqt] + raw[dqt + dqt_n:], "never defined"),
        "no Huffman table": (raw[:dht] + raw[dht + dht_n:], "never defined"),
        "restart out of sequence": (patched(restart, first_rst + 1, [0xD1]), "restart marker"),
        "restart missing": (restart[:second_rst] + restart[second_rst + 2:], "restart marker"),
        "segment length beyond the data": (patched(raw, dqt + 2, [0xFF, 0xFF]), "segment length"),
        "segment length 1": (patched(raw, dqt + 2, [0, 1]), "segment length"),
        "bytes after the last MCU": (raw[:-2] + b"\x12\x34\x56" + raw[-2:], "not followed by EOI"),
        "two frames": (raw[:scan - segment(raw, 0xDA)[2]] + raw[segment(raw, 0xC0)[1]:], "impossible content"),
        "a scan before the frame": (raw[:segment(raw, 0xC0)[1]] + raw[segment(raw, 0xDA)[1]:], "impossible content"),
        # three codes of one bit, taken from the five of three bits (the standard DC table Pillow writes): the total stays
        "too many Huffman codes": (patched(raw, dht + 5, [3, raw[dht + 6], raw[dht + 7] - 3]), "impossible content"),
    }


@pytest.mark.parametrize("case", list(_malformed()))
def test_malformed_streams_are_errors(case):
    raw, message = _malformed()[case]
    rc, _, out = guarded_decode(raw)
    assert -300 < rc <= -200 and out is None
    with pytest.raises(jpeg.CorruptJpeg, match=re.escape(message)):
        jpeg.entropy_decode(raw)


@pytest.mark.parametrize("name", names())
def test_truncations_and_byte_flips_never_leave_the_buffers(name):
    raw = data(name)
    scan = restated(name)[0]["scan"]
    whole = jpeg.entropy_decode(raw).coef.numpy().reshape(-1)
    size = len(raw)
    lengths = sorted(set(list(range(0, size, max(1, size // 40))) + list(range(max(0, scan - 6), min(size, scan + 6)))
                         + list(range(max(0, size - 6), size))))
    for n in lengths:  # truncation anywhere is an error, never a partial image
        rc, _, out = guarded_decode(raw[:n])
        assert -300 < rc <= -200 and out is None, n
    rng = np.random.RandomState(len(raw))
    for _ in range(60):  # single bytes inside the scan: CorruptJpeg, or an image - of the same geometry, since the header is whole
        at = int(rng.randint(scan, size - 2))
        bad = bytearray(raw)
        bad[at] ^= int(rng.randint(1, 256))
        rc, info, out = guarded_decode(bytes(bad))
        assert rc == 0 or -300 < rc <= -200, (at, rc)
        if rc == 0:
            assert out.size == whole.size


# ---- the binding and the device side without a device ------------------------------------------------------------------------------
def _header_symbols():
    with open(jpeg.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_jpeg_[a-z0-9_]+)\s*\(", text)))


def test_jpeg_symbols_are_exported_and_the_other_abis_are_unchanged():
    from madtp_amd import build
    raw = ctypes.CDLL(build.build(verbose=False))
    syms = _header_symbols()
    assert syms == sorted(jpeg.SIGNATURES) and len(syms) == 12
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/madtp_jpeg.h but not exported"
    lib = jpeg.lib()
    assert lib.madtp_jpeg_abi_version() == jpeg.ABI_VERSION == 1
    for name, (res, args) in jpeg.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_int64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert jpeg.SIGNATURES["madtp_jpeg_idct_batch"] == (c_int, [c_void_p] * 4 + [c_int] * 2 + [c_void_p])
    assert jpeg.SIGNATURES["madtp_jpeg_rgb_batch"] == (c_int, [c_void_p] * 3 + [c_int] * 2 + [c_void_p])
    assert jpeg.SIGNATURES["madtp_jpeg_entropy_decode"] == (c_int, [c_void_p, c_int64, c_void_p, c_int64])
    assert jpeg.SIGNATURES["madtp_jpeg_inspect"] == (c_int, [c_void_p, c_int64, c_void_p, c_void_p])
    assert not set(abi.SIGNATURES) & set(syms) and not set(preprocess.SIGNATURES) & set(syms)
    assert jpeg.FIELDS == 16 and sorted(jpeg._F.values()) == list(range(13)) and sorted(jpeg._I.values()) == list(range(9))
    assert "jpeg.hip" in build.SOURCES and "jpeg_entropy.h" in build.HEADERS


def test_codes_have_names():
    lib = jpeg.lib()
    codes = {k: v for k, v in jpeg.DEFINES.items() if k.startswith("MADTP_JPEG_E_")}
    assert len(codes) == 20 and len(set(codes.values())) == 20
    for k, v in codes.items():
        text = lib.madtp_jpeg_strerror(v).decode()
        assert text.startswith("unsupported JPEG" if v > -200 else "corrupt JPEG"), k
    assert lib.madtp_jpeg_strerror(abi.DEFINES["MADTP_E_BADARG"]) == hip.load().madtp_strerror(abi.DEFINES["MADTP_E_BADARG"])


def test_entry_points_refuse_before_any_launch():
    lib = jpeg.lib()
    E_BADARG = abi.DEFINES["MADTP_E_BADARG"]
    assert lib.madtp_jpeg_idct_batch(None, 16, 16, 16, 1, 1, None) == E_BADARG
    assert lib.madtp_jpeg_idct_batch(16, 16, 16, 16, 0, 1, None) == E_BADARG
    assert lib.madtp_jpeg_idct_batch(16, 16, 16, 16, 1, 0, None) == E_BADARG
    assert lib.madtp_jpeg_rgb_batch(16, None, 16, 1, 1, None) == E_BADARG
    assert lib.madtp_jpeg_rgb_batch(16, 16, 16, 1, 0, None) == E_BADARG
    # the size queries
    assert lib.madtp_jpeg_blocks(3, 2, 2, 4, 2) == 12 and lib.madtp_jpeg_blocks(3, 2, 1, 4, 3) == 24 and lib.madtp_jpeg_blocks(1, 1, 1, 5, 3) == 15
    assert lib.madtp_jpeg_blocks(3, 2, 2, 3, 2) == 0 and lib.madtp_jpeg_blocks(1, 2, 2, 4, 2) == 0 and lib.madtp_jpeg_blocks(3, 1, 2, 4, 2) == 0
    assert lib.madtp_jpeg_plane_bytes(3, 2, 2, 4, 2) == 768 and lib.madtp_jpeg_out_bytes(5, 3) == 48 and lib.madtp_jpeg_out_bytes(0, 3) == 0
    assert lib.madtp_jpeg_idct_groups(33) == 2 and lib.madtp_jpeg_idct_groups(32) == 1 and lib.madtp_jpeg_idct_groups(0) == 0
    assert lib.madtp_jpeg_rgb_groups(32, 32) == 1 and lib.madtp_jpeg_rgb_groups(33, 32) == 2 and lib.madtp_jpeg_rgb_groups(8193, 1) == 0
    assert lib.madtp_jpeg_workspace(2, 1000) >= 1000 + 2 * 255 and lib.madtp_jpeg_workspace(0, 1000) == 0


def test_decoder_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    raw = by_prefix("16x16_420")
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        jpeg.JpegDecoder()([raw])
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        jpeg.JpegDecoder(device="cpu")([jpeg.entropy_decode(raw)])
    batch = jpeg.collate([jpeg.read(raw)], then=functools.partial(preprocess.ImagePipeline, 32))
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        batch.to("cuda", non_blocking=True)


def test_decoder_checks_its_items_and_its_pool():
    assert jpeg.JpegDecoder(workers=100).workers == 16 and jpeg.JpegDecoder(workers=0).workers == 1 and jpeg.JpegDecoder().workers == 8
    with pytest.raises(ValueError, match="empty batch"):
        jpeg.JpegDecoder()([])
    with pytest.raises(ValueError, match="image 1"):
        jpeg.JpegDecoder()([by_prefix("8x9_420"), 3.5])
    with pytest.raises(ValueError, match="image 0.*float32"):
        jpeg.JpegDecoder()([np.zeros((4, 4, 3), dtype=np.float32)])
    with pytest.raises(jpeg.CorruptJpeg, match="image 1"):
        jpeg.JpegDecoder()([by_prefix("8x9_420"), by_prefix("8x9_420")[:30]])


def test_collate_keeps_entropy_images():
    a, b = jpeg.read(by_prefix("16x16_420")), jpeg.read(by_prefix("33x31_gray"))
    raw = torch.zeros(5, 4, 3, dtype=torch.uint8)
    then = functools.partial(preprocess.ImagePipeline, 32)
    batch = jpeg.collate([a, raw, b], then=then)
    assert isinstance(batch, jpeg.RawJpegBatch) and len(batch) == 3 and batch.items[2] is b and batch.then is then
    image, caption, idx = jpeg.collate([(a, "one", 4), (b, "two", 7)], then=then)
    assert isinstance(image, jpeg.RawJpegBatch) and caption == ["one", "two"] and idx.tolist() == [4, 7]
    assert torch.equal(jpeg.collate([torch.ones(2), torch.zeros(2)], then=then), torch.tensor([[1.0, 1.0], [0.0, 0.0]]))
    assert jpeg._factory_key(functools.partial(preprocess.ImagePipeline, 32)) == jpeg._factory_key(then)
