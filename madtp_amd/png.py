"""PNG decode for the data loader (csrc/madtp_png.h): the chunks are parsed on the host (csrc/png_device.h, no GPU state: a loader
worker may run it), the per-row unfilter and the expansion to RGB run on the device (csrc/png.hip), and the zlib inflate runs either
on the host (the stdlib's zlib in a thread pool, the default) or on the device - with the bytes of the reference's
`Image.open(path).convert('RGB')` (Pillow 12.2.0) either way.

    decoder = png.PngDecoder()                        # opt-in, next to jpeg.JpegDecoder; inflate="device" moves the inflate over
    images = decoder([bytes0, bytes1, ...])           # -> uint8 [h,w,3] device tensors, views of one packed buffer
    x = preprocess.ImagePipeline(384)(images)         # ... which ImagePipeline / TrainTransform take as they are

    transform-free dataset:  sample = png.read(path)                     # a PngImage (host arrays), made in the worker
    collate_fn = functools.partial(png.collate, then=functools.partial(preprocess.ImagePipeline, 384))
    image = image.to(device, non_blocking=True)       # the RawPngBatch decodes and runs `then`: the drivers' line stays as it is

Accepted: non-interlaced files of 8-bit RGB / RGBA / gray / gray + alpha, 1 / 2 / 4-bit gray, 1 / 2 / 4 / 8-bit palette and 16-bit
RGB / RGBA, sides up to 8192.  A palette index beyond PLTE gives black, as in Pillow.  Everything else is UnsupportedPng naming the
reason (read(..., other="pil") hands such a file to Pillow instead); a malformed file or stream is CorruptPng, never a partial image.
There is no fallback: without a GPU the decoder raises."""
import collections
import os
import zlib

import numpy as np
import torch

from . import abi, hip, jpeg, preprocess
from .staging import MAX_WORKERS, align as _align

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "madtp_png.h")
# the one declaration of the madtp_png_* entry points, next to the sources (abi.bind takes an absolute path as it is); lib() is
# hip.load()'s handle with them set on it (no GPU needed)
SIGNATURES, DEFINES, lib = abi.bind(HEADER, "madtp_png_abi_version", prefix="madtp_png_")
ABI_VERSION = DEFINES["MADTP_PNG_ABI_VERSION"]
FIELDS, INFO_FIELDS, STATUS_FIELDS = DEFINES["MADTP_PNG_FIELDS"], DEFINES["MADTP_PNG_INFO_FIELDS"], DEFINES["MADTP_PNG_STATUS_FIELDS"]
MAX_SIDE, BAND, TILE = DEFINES["MADTP_PNG_MAX_SIDE"], DEFINES["MADTP_PNG_BAND"], DEFINES["MADTP_PNG_TILE"]
_F = {k[len("MADTP_PNG_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_PNG_F_")}
_I = {k[len("MADTP_PNG_I_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_PNG_I_")}
_S = {k[len("MADTP_PNG_S_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_PNG_S_")}
E = {k[len("MADTP_PNG_E_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_PNG_E_")}


class UnsupportedPng(ValueError):
    """a valid PNG of a kind this decoder refuses (interlaced, 16-bit gray, animated, ...)"""


class CorruptPng(ValueError):
    """a malformed PNG file or zlib stream"""


def _raise(code, what):
    if code == 0:
        return
    msg = lib().madtp_png_strerror(code).decode()
    if -200 < code <= -100:
        raise UnsupportedPng(f"{what}: {msg} (code {code}); there is no fallback")
    if -300 < code <= -200:
        raise CorruptPng(f"{what}: {msg} (code {code})")
    raise RuntimeError(f"{what} failed: {msg} (code {code})")


PngInfo = collections.namedtuple("PngInfo", "width height depth color channels rowbytes bpp raw_bytes stream_bytes palette_entries")
_INFO = "WIDTH HEIGHT DEPTH COLOR CHANNELS ROWBYTES BPP RAW_BYTES STREAM_BYTES PALETTE".split()


class PngImage:
    """What the host stage makes of one file: the header fields of PngInfo, `palette` (uint8 [768]: PLTE, zero beyond it) and
    `stream` (1-D uint8: the payloads of the IDAT chunks as one zlib stream).  Plain numpy arrays and ints: it pickles from a loader
    worker to the main process."""
    __slots__ = PngInfo._fields + ("palette", "stream")

    def __init__(self, info, palette, stream):
        for k, v in zip(PngInfo._fields, info):
            setattr(self, k, int(v))
        self.palette, self.stream = palette, stream

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, state):
        for k, v in state.items():
            setattr(self, k, v)


def _prepare(buf, what, with_stream):
    info = np.zeros(INFO_FIELDS, dtype=np.int32)
    palette = np.zeros(768, dtype=np.uint8)
    h = lib()
    _raise(h.madtp_png_prepare(buf.ctypes.data, buf.size, info.ctypes.data, palette.ctypes.data, None, 0), what)
    fields = PngInfo(*(int(info[_I[k]]) for k in _INFO))
    if not with_stream:
        return fields, palette, None
    stream = np.empty(max(fields.stream_bytes, 1), dtype=np.uint8)[:fields.stream_bytes]
    _raise(h.madtp_png_prepare(buf.ctypes.data, buf.size, info.ctypes.data, palette.ctypes.data, stream.ctypes.data, stream.size), what)
    return fields, palette, stream


def inspect(data):
    """bytes, a 1-D uint8 array or a path -> PngInfo of the header and the chunk list.  Host only.  UnsupportedPng / CorruptPng."""
    return _prepare(jpeg._byte_array(data, "inspect"), "inspect", False)[0]


def prepare(data, what="prepare"):
    """bytes, a 1-D uint8 array or a path -> PngImage.  Host only (no GPU state is touched, the stream is not inflated): usable in a
    DataLoader worker.  UnsupportedPng / CorruptPng name the reason of a file the decoder refuses."""
    return PngImage(*_prepare(jpeg._byte_array(data, what), what, True))


def read(source, other="raise"):
    """a path or bytes -> PngImage: the dataset's replacement for Image.open(path).convert('RGB').  other="pil": a file this decoder
    REFUSES (UnsupportedPng: interlaced, 16-bit gray, ...) is decoded by Pillow to preprocess.raw_image()'s uint8 [h,w,3] tensor,
    which the decoder passes through; a corrupt file raises either way, a corrupt stream raises when the batch is decoded."""
    if other not in ("raise", "pil"):
        raise ValueError(f"read: other={other!r} is not 'raise' or 'pil'")
    buf = jpeg._byte_array(source, "read")
    try:
        return prepare(buf, str(source) if isinstance(source, (str, os.PathLike)) else "read")
    except UnsupportedPng:
        if other != "pil":
            raise
    import io
    from PIL import Image
    return preprocess.raw_image(Image.open(io.BytesIO(buf.tobytes())))


def inflate_host(stream, raw_bytes, rowbytes=0):
    """The inflate kernel's routines with the lanes in a loop, on the host (madtp_png_inflate_host): a zlib stream -> (code, uint8
    [raw_bytes] or None, int32 [STATUS_FIELDS] status).  For checking without a GPU; the host's inflate is zlib's."""
    s = jpeg._byte_array(stream, "inflate_host")
    raw = np.zeros(int(raw_bytes), dtype=np.uint8)
    status = np.zeros(STATUS_FIELDS, dtype=np.int32)
    rc = lib().madtp_png_inflate_host(s.ctypes.data, s.size, raw.ctypes.data, raw.size, int(rowbytes), status.ctypes.data)
    return rc, raw if rc == 0 else None, status


def unfilter_host(raw, width, height, depth, color, palette):
    """The unfilter kernel's routines with the lanes in a loop, on the host: filtered scanlines -> (code, uint8 [h, w, 3] or None)"""
    raw, palette = np.ascontiguousarray(raw, dtype=np.uint8), np.ascontiguousarray(palette, dtype=np.uint8)
    want = lib().madtp_png_raw_bytes(int(width), int(height), int(depth), int(color))
    if want == 0 or raw.size != want or palette.size != 768:
        raise ValueError("unfilter_host: the scanlines are not those of such an image, or the palette is not 768 bytes")
    out = np.zeros((int(height), int(width), 3), dtype=np.uint8)
    rc = lib().madtp_png_unfilter_host(raw.ctypes.data, int(width), int(height), int(depth), int(color), palette.ctypes.data, out.ctypes.data)
    return rc, out if rc == 0 else None


# ---- the layout of a batch ---------------------------------------------------------------------------------------------------------
# One device buffer per batch; every offset of a table row counts from its beginning:
#   [ table rows of the PNG items | their palettes || payload: filtered scanlines (inflate="host") or zlib streams ("device") |
#     decoded pass-through images ]    <- staged and copied, copy_bytes in all; everything before || is `head`
#   [ filtered scanlines the inflate kernel writes ("device") ]    from raw_at
#   [ decoded images, then the unfilter kernel's carry ]           from out_at .. total
# The three regions begin at multiples of 256 bytes, an image's payload and scanlines at multiples of 256, its pixels of 16.
PngPlan = collections.namedtuple("PngPlan", "B inflate head table table_bytes palette_at coded payload copy_bytes raw_at out_at total "
                                            "workspace shapes")


def plan_batch(items, inflate="host"):
    """The one place that lays a batch out and fills the MADTP_PNG_F_* rows.  Host arithmetic only, with the library's own size
    queries.  items: per image ("raw", shape) or ("coded", fields) with the fields of a PngInfo.  ValueError naming the image whose
    fields contradict each other."""
    if inflate not in ("host", "device"):
        raise ValueError(f"inflate={inflate!r} is not 'host' or 'device'")
    h = lib()
    coded = [i for i, it in enumerate(items) if it[0] == "coded"]
    table = np.zeros((len(coded), FIELDS), dtype=np.int64)
    palette_at = table.nbytes
    at = _align(palette_at + 768 * len(coded), 256)
    payload, sizes = [], []
    for k, i in enumerate(coded):
        im = items[i][1]
        rowbytes = int(h.madtp_png_rowbytes(im.width, im.depth, im.color))
        raw_bytes = int(h.madtp_png_raw_bytes(im.width, im.height, im.depth, im.color))
        if raw_bytes < 1 or (rowbytes, raw_bytes) != (im.rowbytes, im.raw_bytes) or not 0 <= im.stream_bytes < 1 << 31:
            raise ValueError(f"image {i}: a PngImage whose fields contradict each other")
        sizes.append(raw_bytes)
        payload.append(at)
        at = _align(at + (raw_bytes if inflate == "host" else im.stream_bytes), 256)
        table[k, [_F[n] for n in "W H DEPTH COLOR RAW_BYTES STREAM_BYTES PALETTE".split()]] = (
            im.width, im.height, im.depth, im.color, raw_bytes, im.stream_bytes, palette_at + 768 * k)
    places = {}
    for i, it in enumerate(items):
        if it[0] == "raw":
            hh, ww = int(it[1][0]), int(it[1][1])
            at = _align(at, 16)
            places[i] = ((hh, ww), at)
            at += 3 * hh * ww
    copy_bytes = at
    raw_at = at = _align(at, 256)
    for k in range(len(coded)):
        if inflate == "host":
            table[k, _F["RAW"]] = payload[k]
        else:
            table[k, _F["STREAM"]], table[k, _F["RAW"]] = payload[k], at
            at = _align(at + sizes[k], 256)
    out_at = at = _align(at, 256)
    for k, i in enumerate(coded):
        im = items[i][1]
        table[k, _F["OUT"]] = at
        places[i] = ((im.height, im.width), at)
        at = _align(at + 3 * im.height * im.width, 16)
    for k, i in enumerate(coded):
        table[k, _F["CARRY"]] = at
        at += int(h.madtp_png_carry_bytes(items[i][1].height))
    head = np.zeros(palette_at + 768 * len(coded), dtype=np.uint8)
    head[:palette_at] = table.reshape(-1).view(np.uint8)
    return PngPlan(len(items), inflate, head, table, table.nbytes, palette_at, coded, payload, copy_bytes, raw_at, out_at, at, 0,
                   [places[i] for i in range(len(items))])


class PreparedPngBatch(jpeg._Prepared, collections.namedtuple("PreparedPngBatch", "packed plan status")):
    """what prepare() leaves on the device: the packed buffer of the plan, the plan, and the status words of the inflate kernel"""
    __slots__ = ()


class PngDecoder(jpeg._BatchDecoder):
    """PNG files -> uint8 [h,w,3] tensors on `device`, views of one packed buffer: one copy per batch, then one launch
    (inflate="host": madtp_png_unfilter_batch) or two (inflate="device": madtp_png_inflate_batch first).

    An item is a PngImage, the bytes of a file (parsed here) or an already decoded uint8 [h,w,3] host array / tensor, which is
    copied through unchanged.  inflate="host": `workers` threads inflate with the stdlib's zlib, which releases the GIL (at most
    MAX_WORKERS, never sized from the machine's CPU count), into one of two pinned staging buffers (guarded by events, as
    ImagePipeline's); every stream is checked before anything is launched.  inflate="device": the zlib streams cross as they are;
    the call waits for the status words of the inflate kernel only - on a side stream, behind an event recorded after that kernel -
    and raises CorruptPng naming the image if one is not 0."""

    def __init__(self, device="cuda", workers=8, inflate="host"):
        if inflate not in ("host", "device"):
            raise ValueError(f"PngDecoder: inflate={inflate!r} is not 'host' or 'device'")
        super().__init__(device, workers, "madtp-png")
        self.inflate = inflate
        self._side = None
        self._host_status = None
        self.last_status = None  # int32 [coded images, STATUS_FIELDS] of the last inflate="device" batch (numpy), for tools and tests

    def prepare(self, items):
        """the checks, the parsing of byte items, the host inflate or the packing of the streams, and the copy -> PreparedPngBatch"""
        items = list(items)
        if len(items) < 1:
            raise ValueError("PngDecoder: an empty batch")
        lib()  # (bound before the pool's threads call it)

        def parse(i):
            it = items[i]
            if isinstance(it, PngImage):
                return it
            host = self._decoded(it, i)
            return host if host is not None else prepare(jpeg._byte_array(it, f"image {i}"), f"image {i}")

        parsed = self._pool.map(parse, list(range(len(items))))  # (a file this decoder refuses raises here, before any launch)
        self._need_gpu("png.inflate_host / png.unfilter_host run the kernels' routines on the host for CPU checking.")
        decoded = {i: it for i, it in enumerate(parsed) if not isinstance(it, PngImage)}
        plan = plan_batch([("raw", it.shape) if i in decoded else ("coded", it) for i, it in enumerate(parsed)], self.inflate)

        def fill(view, stage):
            for k, i in enumerate(plan.coded):
                view[plan.palette_at + 768 * k:plan.palette_at + 768 * (k + 1)] = parsed[i].palette

            def one(job):
                k, i = job
                im, o = parsed[i], plan.payload[k]
                if self.inflate == "device":
                    view[o:o + im.stream_bytes] = im.stream
                    return
                z = zlib.decompressobj()
                try:
                    raw = z.decompress(im.stream.data, im.raw_bytes + 1)
                except zlib.error as e:
                    raise CorruptPng(f"image {i}: {e}") from None
                if len(raw) != im.raw_bytes:
                    _raise(E["SIZE"] if len(raw) > im.raw_bytes or z.eof else E["TRUNCATED"], f"image {i}")
                if not z.eof:
                    _raise(E["TRUNCATED"], f"image {i}")
                view[o:o + im.raw_bytes] = np.frombuffer(raw, dtype=np.uint8)
                if int(view[o:o + im.raw_bytes:1 + im.rowbytes].max()) > 4:
                    _raise(E["FILTER"], f"image {i}")

            self._pool.map(one, list(enumerate(plan.coded)))

        packed, _ = self._send(plan, decoded, fill)
        status = torch.empty(max(len(plan.coded), 1), STATUS_FIELDS, dtype=torch.int32, device=packed.device)
        return PreparedPngBatch(packed, plan, status)

    @staticmethod
    def scanlines(batch):
        """-> the filtered scanlines of every PNG item of a batch (on the device route: one that has run), views of its packed buffer"""
        rows = batch.plan.table
        return [batch.packed[int(r[_F["RAW"]]):int(r[_F["RAW"]]) + int(r[_F["RAW_BYTES"]])] for r in rows]

    def launches(self, batch):
        """-> [(entry point, launch(stream) -> code)] of a prepared batch, in order (tools time them one by one)"""
        h = lib()
        p, n = batch.packed.data_ptr(), len(batch.plan.coded)
        if not n:
            return []
        unfilter = ("madtp_png_unfilter_batch", lambda stream: h.madtp_png_unfilter_batch(p, p, p, p, n, stream))
        if batch.plan.inflate == "host":
            return [unfilter]
        return [("madtp_png_inflate_batch", lambda stream: h.madtp_png_inflate_batch(p, p, p, batch.status.data_ptr(), n, stream)), unfilter]

    def run(self, batch):
        """the launches on the current stream and, on the device route, the wait for the status words -> list of uint8 [h,w,3] views
        of the batch's packed buffer; CorruptPng names the first image whose stream is malformed, and nothing is returned then"""
        with torch.cuda.device(batch.packed.device):
            cur = torch.cuda.current_stream()
            inflated = None
            for name, launch in self.launches(batch):
                hip._check(launch(cur.cuda_stream), name)
                if name == "madtp_png_inflate_batch":
                    inflated = torch.cuda.Event()
                    inflated.record(cur)
            if inflated is not None:
                n = len(batch.coded)
                with self._lock:
                    if self._side is None:
                        self._side = torch.cuda.Stream(device=batch.packed.device)
                    if self._host_status is None or self._host_status.shape[0] < n:
                        self._host_status = torch.empty(max(n, 64), STATUS_FIELDS, dtype=torch.int32, pin_memory=True)
                    side, host = self._side, self._host_status
                    side.wait_event(inflated)
                    batch.status.record_stream(side)
                    with torch.cuda.stream(side):
                        host[:n].copy_(batch.status[:n], non_blocking=True)
                    side.synchronize()
                    status = host[:n].numpy().copy()
                self.last_status = status
                for k, i in enumerate(batch.coded):
                    code = int(status[k, _S["CODE"]])
                    if code < -99:
                        _raise(code, f"image {i}")
                    elif code != 0:
                        hip._check(code, f"madtp_png_inflate_batch (image {i})")
        return self._images(batch)


# ---- the data loader's side ------------------------------------------------------------------------------------------------------
class RawPngBatch(jpeg._DecodedBatch):
    """jpeg._DecodedBatch of what png.read() makes (PngImages, and raw uint8 [h,w,3] tensors of files that went to Pillow)"""
    decoder, item = PngDecoder, PngImage


def collate(samples, then):
    """collate_fn (bind `then` with functools.partial): the PngImages / raw images of the samples become one RawPngBatch, everything
    else goes through torch's default_collate.  Samples are such images or tuples / lists that hold one."""
    return RawPngBatch.collate(samples, then)
