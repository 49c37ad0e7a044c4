"""The device Huffman stage (madtp_amd/jpeg_device.py, csrc/jpeg_huff_device.h) without a GPU: madtp_jhuff_decode_host runs the
kernel's lane routines and passes with the lanes in a loop, and is compared with the host decoder (jpeg.entropy_decode) on the whole
corpus at forced subsequence sizes, on the named malformed scans, on truncations and seeded byte flips into guarded buffers; the
pass bound; the binding against include/madtp_jhuff.h.  Every compare is exact."""
import ctypes
import functools
import pickle
import re

import numpy as np
import pytest
import torch

from madtp_amd import abi, augment, jpeg, jpeg_device, preprocess, search
from tests import jpeg_ref
from tests.jpeg_device_cases import (SUBSEQS, by_prefix, data, guarded_lanes, guesses_part, host_code, host_coefficients, malformed,
                                     names, truncations)

S = jpeg_device._S


@functools.lru_cache(maxsize=None)
def lanes(name, subseq):
    """(code, coefficients, status) of the emulation for a corpus file (computed once, shared)"""
    return guarded_lanes(data(name), subseq)


# ---- 1. corpus equality, 4. the pass bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("subseq", SUBSEQS)
@pytest.mark.parametrize("name", names())
def test_corpus_equals_host_decoder(name, subseq):
    assert len(names()) == 42
    rc, coef, status = lanes(name, subseq)
    assert rc == 0 and status[S["CODE"]] == 0
    assert np.array_equal(coef.reshape(-1, 64), host_coefficients(name))
    scan_bytes = len(data(name)) - jpeg_ref.parse(data(name))["scan"]
    size = subseq or jpeg_device.lib().madtp_jhuff_subseq_bytes(scan_bytes)
    assert status[S["SUBSEQS"]] == max(1, -(-scan_bytes // size))
    assert status[S["SERIAL"]] == 0  # a valid file of an encoder never needs the serial lane


def test_small_subsequences_meet_the_hard_cases():
    """what 4-byte subsequences must exercise is in the corpus: stuffed FF 00 pairs on a boundary, codes over 9 bits, lanes without a
    whole symbol (more subsequences than symbols), files of one MCU, a restart marker behind every MCU"""
    split = long_codes = False
    for n in names():
        raw = data(n)
        h = jpeg_ref.parse(raw)
        scan = h["scan"]
        split |= any(raw[p] == 0xFF and raw[p + 1] == 0 and (p + 1 - scan) % 4 == 0 for p in range(scan, len(raw) - 2))
        long_codes |= any(e is not None and e[0] > 9 for lut in list(h["dc"].values()) + list(h["ac"].values()) for e in lut)
    assert split and long_codes
    assert any(n.startswith("1x1_") for n in names()) and any("restart" in n for n in names()) and any("optimize" in n for n in names())
    # more than one round of lanes, and a last round that is not full
    assert max(lanes(n, 4)[2][S["SUBSEQS"]] for n in names()) > 2 * jpeg_device.LANES


@pytest.mark.parametrize("name", names())
def test_passes_never_exceed_subsequences(name):
    for subseq in SUBSEQS:
        status = lanes(name, subseq)[2]
        assert 1 <= status[S["PASSES"]] <= status[S["SUBSEQS"]], (subseq, status)


def test_default_subsequence_size():
    f = jpeg_device.lib().madtp_jhuff_subseq_bytes
    assert f(0) == 32 and f(1) == 32 and f(32 * 1024) == 32 and f(32 * 1024 + 1) == 36 and f(73000) == 72 and f(-1) == 0
    for n in (5000, 73000, 10 ** 6, jpeg_device.MAX_BYTES):
        assert f(n) % 4 == 0 and -(-n // f(n)) <= jpeg_device.LANES


# ---- 2. named malformed streams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subseq", (4, 32, 0))
@pytest.mark.parametrize("case", list(malformed()) + list(truncations()))
def test_malformed_streams_give_the_host_decoders_code(case, subseq):
    raw, message = {**malformed(), **truncations()}[case]
    want, _ = host_code(raw)
    assert -300 < want <= -200
    rc, coef, status = guarded_lanes(raw, subseq)
    assert rc == want and status[S["CODE"]] == want and coef is None
    assert message in jpeg.lib().madtp_jpeg_strerror(rc).decode()


def test_a_file_the_guesses_get_wrong_goes_to_the_serial_lane():
    raw = guesses_part()
    want, coef = host_code(raw)
    assert want == 0 and coef.size == 16 * 64 and not coef.any()
    for subseq in (4, 0):  # (at the default size the one lane starts from the true state and ends in the code itself)
        rc, got, status = guarded_lanes(raw, subseq)
        assert rc == 0 and np.array_equal(got, coef)
        assert status[S["SERIAL"]] == (1 if subseq else 0) and status[S["PASSES"]] <= status[S["SUBSEQS"]]


# ---- 3. truncations and byte flips ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names())
def test_truncations_and_byte_flips_agree_with_the_host_decoder(name):
    raw = data(name)
    scan = jpeg_ref.parse(raw)["scan"]
    size = len(raw)
    lengths = sorted(set(list(range(0, size, max(1, size // 40))) + list(range(max(0, scan - 6), min(size, scan + 6)))
                         + list(range(max(0, size - 6), size))))
    for n in lengths:
        want, _ = host_code(raw[:n])
        assert -300 < want <= -200
        for subseq in (4, 0):
            rc, coef, status = guarded_lanes(raw[:n], subseq)
            assert rc == want and coef is None, (n, subseq, rc, want)
    rng = np.random.RandomState(len(raw))
    for _ in range(60):
        at = int(rng.randint(scan, size - 2))
        bad = bytearray(raw)
        bad[at] ^= int(rng.randint(1, 256))
        want, coef = host_code(bytes(bad))
        for subseq in (4, 0):
            rc, got, status = guarded_lanes(bytes(bad), subseq)
            assert (rc == 0) == (want == 0), (at, subseq, rc, want)
            assert status[S["PASSES"]] <= max(1, status[S["SUBSEQS"]])
            if rc == 0:
                assert np.array_equal(got, coef), (at, subseq)
            else:
                assert -300 < rc <= -200


# ---- 5. the binding ------------------------------------------------------------------------------------------------------------------
def _header_symbols():
    with open(jpeg_device.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_jhuff_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_exported_and_the_other_abis_are_unchanged():
    from madtp_amd import build
    raw = ctypes.CDLL(build.build(verbose=False))
    syms = _header_symbols()
    assert syms == sorted(jpeg_device.SIGNATURES) and len(syms) == 5
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/madtp_jhuff.h but not exported"
    lib = jpeg_device.lib()
    assert lib.madtp_jhuff_abi_version() == jpeg_device.ABI_VERSION == 1
    for name, (res, args) in jpeg_device.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_int64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert jpeg_device.SIGNATURES["madtp_jhuff_decode_batch"] == (c_int, [c_void_p] * 4 + [c_int] * 2 + [c_void_p])
    assert jpeg_device.SIGNATURES["madtp_jhuff_decode_host"] == (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p])
    assert jpeg_device.SIGNATURES["madtp_jhuff_prepare"] == (c_int, [c_void_p, c_int64] + [c_void_p] * 4)
    # the headers that were there keep their versions and their symbols
    assert jpeg.ABI_VERSION == 1 and len(jpeg.SIGNATURES) == 12 and not set(jpeg.SIGNATURES) & set(syms)
    assert len([k for k in jpeg.DEFINES if k.startswith("MADTP_JPEG_E_")]) == 20
    assert abi.DEFINES["MADTP_ABI_VERSION"] == lib.madtp_abi_version() == 31
    assert preprocess.ABI_VERSION == lib.madtp_image_abi_version() == 1
    assert augment.ABI_VERSION == lib.madtp_augment_abi_version() == 1
    assert search.ABI_VERSION == lib.madtp_search_abi_version() == 1
    assert jpeg_device.FIELDS == 16 and sorted(jpeg_device._F.values()) == list(range(11)) and sorted(S.values()) == list(range(4))
    assert jpeg_device.RECORD_BYTES == 6 * jpeg_device.DEFINES["MADTP_JHUFF_TABLE_BYTES"]
    assert "jpeg_huff.hip" in build.SOURCES and "jpeg_huff_device.h" in build.HEADERS


def test_entry_points_refuse_before_any_launch():
    lib = jpeg_device.lib()
    E_BADARG = abi.DEFINES["MADTP_E_BADARG"]
    assert lib.madtp_jhuff_decode_batch(None, 16, 16, 16, 1, 0, None) == E_BADARG
    assert lib.madtp_jhuff_decode_batch(16, None, 16, 16, 1, 0, None) == E_BADARG
    assert lib.madtp_jhuff_decode_batch(16, 16, None, 16, 1, 0, None) == E_BADARG
    assert lib.madtp_jhuff_decode_batch(16, 16, 16, None, 1, 0, None) == E_BADARG
    assert lib.madtp_jhuff_decode_batch(16, 16, 16, 16, 0, 0, None) == E_BADARG
    for bad in (1, 2, 3, 6, 33, -4):
        assert lib.madtp_jhuff_decode_batch(16, 16, 16, 16, 1, bad, None) == E_BADARG
    raw = by_prefix("16x16_420")
    buf = np.frombuffer(raw, dtype=np.uint8)
    coef = np.zeros(64 * 6, dtype=np.int16)
    status = np.zeros(4, dtype=np.int32)
    host = lib.madtp_jhuff_decode_host
    assert host(buf.ctypes.data, buf.size, 0, coef.ctypes.data, coef.size, status.ctypes.data) == 0
    assert host(None, buf.size, 0, coef.ctypes.data, coef.size, status.ctypes.data) == E_BADARG
    assert host(buf.ctypes.data, buf.size, 0, None, coef.size, status.ctypes.data) == E_BADARG
    assert host(buf.ctypes.data, buf.size, 0, coef.ctypes.data, coef.size, None) == E_BADARG
    assert host(buf.ctypes.data, buf.size, 6, coef.ctypes.data, coef.size, status.ctypes.data) == E_BADARG
    before = coef.copy()
    assert host(buf.ctypes.data, buf.size, 0, coef.ctypes.data, coef.size - 1, status.ctypes.data) == E_BADARG
    assert np.array_equal(coef, before)
    info, q, tables, scan = np.zeros(16, np.int32), np.zeros(192, np.uint16), np.zeros(jpeg_device.RECORD_BYTES, np.uint8), ctypes.c_int64()
    prep = lib.madtp_jhuff_prepare
    assert prep(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data, tables.ctypes.data, ctypes.addressof(scan)) == 0
    assert prep(None, buf.size, info.ctypes.data, q.ctypes.data, tables.ctypes.data, ctypes.addressof(scan)) == E_BADARG
    assert prep(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data, None, ctypes.addressof(scan)) == E_BADARG
    assert prep(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data, tables.ctypes.data, None) == E_BADARG
    assert prep(buf.ctypes.data, -1, info.ctypes.data, q.ctypes.data, tables.ctypes.data, ctypes.addressof(scan)) == E_BADARG


# ---- the host stage and the module without a device -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names())
def test_prepare_equals_inspect_and_the_restatements_tables(name):
    raw = data(name)
    s = jpeg_device.prepare_scan(raw)
    e = jpeg.entropy_decode(raw)
    h = jpeg_ref.parse(raw)
    got = (s.width, s.height, s.components, s.hs, s.vs, s.blocks_x, s.blocks_y, s.restart_interval, s.blocks)
    assert got == (e.width, e.height, e.components, e.hs, e.vs, e.blocks_x, e.blocks_y, e.restart_interval, e.coef.shape[0])
    assert np.array_equal(s.qtables, e.qtables.numpy()) and s.scan_begin == h["scan"] and s.data.tobytes() == raw
    # the 9-bit lookahead table of every component against the restatement's 16-bit one
    tables = s.tables.reshape(6, -1)
    for c in range(s.components):
        for kind, lut in ((0, h["dc"][h["tables"][c][0]]), (1, h["ac"][h["tables"][c][1]])):
            look = tables[2 * c + kind][:1024].view(np.uint16)
            for i in range(512):
                entry = lut[i << 7]
                assert look[i] == (entry[0] << 8 | entry[1] if entry is not None and entry[0] <= 9 else 0), (c, kind, i)
    assert not tables[2 * s.components:].any()


def test_header_codes_are_inspects(tmp_path):
    raw = by_prefix("16x16_444")
    for bad in (b"", raw[:2], raw[:40], b"\x00\x00" + raw[2:]):
        want, _ = host_code(bad)
        assert -300 < want <= -200 and guarded_lanes(bad, 0)[0] == want
        with pytest.raises(jpeg.CorruptJpeg):
            jpeg_device.prepare_scan(bad)
    sof = raw.index(b"\xff\xc0")
    progressive = raw[:sof + 1] + b"\xc2" + raw[sof + 2:]
    with pytest.raises(jpeg.UnsupportedJpeg, match="progressive"):
        jpeg_device.read(progressive)
    with pytest.raises(jpeg.UnsupportedJpeg, match="image 1.*progressive"):  # before any launch, before a device is needed
        jpeg_device.DeviceJpegDecoder()([raw, progressive])
    with pytest.raises(ValueError, match="other="):
        jpeg_device.read(raw, other="quiet")
    path = tmp_path / "a.jpg"
    path.write_bytes(raw)
    s = jpeg_device.read(path)
    again = pickle.loads(pickle.dumps(s))  # what a loader worker does with it
    assert isinstance(again, jpeg_device.ScanImage) and again.data.tobytes() == raw and again.scan_begin == s.scan_begin
    assert np.array_equal(again.tables, s.tables) and np.array_equal(again.qtables, s.qtables) and again.width == 16


def test_decoder_needs_a_gpu_and_checks_its_arguments(monkeypatch):
    D = jpeg_device.DeviceJpegDecoder
    assert D(workers=100).workers == 16 and D(workers=0).workers == 1 and D().workers == 8 and D().subseq_bytes == 0
    for bad in (3, 6, -4):
        with pytest.raises(ValueError, match="subseq_bytes"):
            D(subseq_bytes=bad)
    with pytest.raises(ValueError, match="empty batch"):
        D()([])
    with pytest.raises(ValueError, match="image 1"):
        D()([by_prefix("8x9_420"), 3.5])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    raw = by_prefix("16x16_420")
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        D()([raw])
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        D(device="cpu")([jpeg_device.read(raw)])
    then = functools.partial(preprocess.ImagePipeline, 32)
    batch = jpeg_device.collate([jpeg_device.read(raw)], then=then)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        batch.to("cuda", non_blocking=True)
    a, b = jpeg_device.read(raw), jpeg_device.read(by_prefix("33x31_gray"))
    decoded = torch.zeros(5, 4, 3, dtype=torch.uint8)
    batch = jpeg_device.collate([a, decoded, b], then=then)
    assert isinstance(batch, jpeg_device.RawJpegDeviceBatch) and len(batch) == 3 and batch.items[2] is b and batch.then is then
    image, caption, idx = jpeg_device.collate([(a, "one", 4), (b, "two", 7)], then=then)
    assert isinstance(image, jpeg_device.RawJpegDeviceBatch) and caption == ["one", "two"] and idx.tolist() == [4, 7]
