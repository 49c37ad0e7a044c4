"""Byte strings shared by tests/test_jpeg_device_cpu.py and tests/test_jpeg_device_gpu.py: the corpus of tests/golden/jpeg_pil.npz,
the named malformed scans (built the way tests/test_jpeg_cpu.py builds them, from the restatement's tables), fixed truncations, and
one hand-made file that the lanes' guesses get wrong although it is valid.  Nothing here needs a GPU."""
import functools
import os

import numpy as np

from madtp_amd import jpeg, jpeg_device
from tests import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")
GUARD = 4096
SUBSEQS = (4, 8, 12, 32, 128, 0)


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
def host_coefficients(name):
    """int16 [blocks, 64] of jpeg.entropy_decode (computed once, shared, never written)"""
    c = jpeg.entropy_decode(data(name)).coef.numpy()
    c.setflags(write=False)
    return c


def host_code(raw):
    """the code of madtp_jpeg_inspect / madtp_jpeg_entropy_decode for these bytes"""
    lib = jpeg.lib()
    buf = np.frombuffer(bytes(raw), dtype=np.uint8).copy()
    info = np.zeros(jpeg.INFO_FIELDS, dtype=np.int32)
    q = np.zeros((3, 64), dtype=np.uint16)
    rc = lib.madtp_jpeg_inspect(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data)
    if rc:
        return rc, None
    out = np.zeros(64 * int(info[jpeg._I["BLOCKS"]]), dtype=np.int16)
    rc = lib.madtp_jpeg_entropy_decode(buf.ctypes.data, buf.size, out.ctypes.data, out.size)
    return rc, out if rc == 0 else None


def guarded_lanes(raw, subseq):
    """madtp_jhuff_decode_host on an exact-size copy, the coefficients between canary words -> (code, coefficients or None, status)"""
    lib = jpeg_device.lib()
    buf = np.frombuffer(bytes(raw), dtype=np.uint8).copy()
    info = np.zeros(jpeg.INFO_FIELDS, dtype=np.int32)
    q = np.zeros((3, 64), dtype=np.uint16)
    status = np.full(jpeg_device.STATUS_FIELDS + 2, 0x5A5A5A5A, dtype=np.int32)
    blocks = 1
    if lib.madtp_jpeg_inspect(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data) == 0:
        blocks = int(info[jpeg._I["BLOCKS"]])
    n = 64 * blocks
    out = np.full(n + 2 * GUARD, 0x7B7B, dtype=np.int16)
    rc = lib.madtp_jhuff_decode_host(buf.ctypes.data, buf.size, subseq, out[GUARD:].ctypes.data, n, status[1:].ctypes.data)
    assert (out[:GUARD] == 0x7B7B).all() and (out[GUARD + n:] == 0x7B7B).all(), "a write outside the given buffer"
    assert status[0] == 0x5A5A5A5A and status[-1] == 0x5A5A5A5A
    return rc, out[GUARD:GUARD + n].copy() if rc == 0 else None, status[1:-1].copy()


def _code_of(lut, symbol):
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


def patched(raw, at, new):
    return raw[:at] + bytes(new) + raw[at + len(bytes(new)):]


@functools.lru_cache(maxsize=None)
def malformed():
    """name -> (bytes, text of the reason): the six malformed scans of the issue"""
    raw = by_prefix("16x16_444")
    h = jpeg_ref.parse(raw)
    scan = h["scan"]
    dc, ac = h["dc"][h["tables"][0][0]], h["ac"][h["tables"][0][1]]
    bits = lambda sym, lut: format(_code_of(lut, sym)[0], f"0{_code_of(lut, sym)[1]}b")
    zrl4 = bits(0, dc) + bits(0xF0, ac) * 4       # four runs of sixteen zeros: index 65
    run = bits(0, dc) + bits(0xF0, ac) * 3 + bits(0xF1, ac) + "1"  # index 49 + 15 = 64 for a coefficient
    restart = by_prefix("37x53_420_q85_restart")
    rs = jpeg_ref.parse(restart)["scan"]
    first_rst = restart.index(b"\xff\xd0", rs)
    second_rst = restart.index(b"\xff\xd1", rs)
    return {
        "all-ones scan": (raw[:scan] + b"\xff\x00" * 64 + b"\xff\xd9", "no Huffman code"),
        "index beyond 63 (runs)": (raw[:scan] + _pack(zrl4) + b"\xff\xd9", "index beyond 63"),
        "index beyond 63 (coefficient)": (raw[:scan] + _pack(run) + b"\xff\xd9", "index beyond 63"),
        "restart out of sequence": (patched(restart, first_rst + 1, [0xD1]), "restart marker"),
        "restart missing": (restart[:second_rst] + restart[second_rst + 2:], "restart marker"),
        "bytes after the last MCU": (raw[:-2] + b"\x12\x34\x56" + raw[-2:], "not followed by EOI"),
    }


@functools.lru_cache(maxsize=None)
def truncations():
    """three fixed truncations inside the scan -> name -> (bytes, text of the reason)"""
    out = {}
    for prefix, keep in (("48x64_420", 0.5), ("33x31_gray", 0.8), ("37x53_420_q85_restart", 0.6)):
        raw = by_prefix(prefix)
        scan = jpeg_ref.parse(raw)["scan"]
        out[f"{prefix} cut at {keep}"] = (raw[:scan + int((len(raw) - scan) * keep)], "corrupt JPEG")
    return out


def guesses_part():
    """A valid grayscale file of sixteen 8x8 MCUs, restart interval 4, whose DC and AC tables hold one code of one bit each, so a
    block is the two bits 00 and a byte holds a whole restart interval.  A lane that does not know its MCU number sees the restart
    marker behind a whole MCU after two bits and takes it, three MCUs early, so it counts fewer blocks than the exact rules do.  With
    4-byte subsequences the first lane ends in a state, not a code: the chain check must catch the difference and the serial lane
    must give the host decoder's answer (code 0, every coefficient 0)."""
    dqt = b"\xff\xdb\x00\x43\x00" + bytes([1] * 64)
    sof = b"\xff\xc0\x00\x0b\x08\x00\x08\x00\x80\x01\x01\x11\x00"
    dht = lambda tc: b"\xff\xc4\x00\x14" + bytes([tc << 4]) + bytes([1] + [0] * 15) + b"\x00"
    dri = b"\xff\xdd\x00\x04\x00\x04"
    sos = b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    return b"\xff\xd8" + dqt + sof + dht(0) + dht(1) + dri + sos + b"\x00\xff\xd0\x00\xff\xd1\x00\xff\xd2\x00\xff\xd9"
