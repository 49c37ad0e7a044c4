"""Baseline JPEG decode with the Huffman entropy stage on the device (include/madtp_jhuff.h, csrc/jpeg_huff.hip): the host parses
the header (microseconds per file), the compressed bytes cross to the GPU, one launch decodes every scan of the batch into the int16
coefficients of jpeg.entropy_decode - bit for bit - and the IDCT and colour kernels of jpeg.py read them where they lie.

    decoder = jpeg_device.DeviceJpegDecoder()          # opt-in, next to jpeg.JpegDecoder, whose default does not change
    images = decoder([bytes0, bytes1, ...])            # -> uint8 [h,w,3] device tensors, views of one packed buffer
    x = preprocess.ImagePipeline(384)(images)

    transform-free dataset:  sample = jpeg_device.read(path)               # a ScanImage (bytes + parsed header), made in the worker
    collate_fn = functools.partial(jpeg_device.collate, then=functools.partial(preprocess.ImagePipeline, 384))
    image = image.to(device, non_blocking=True)        # the RawJpegDeviceBatch decodes and runs `then`

The accepted files, the refusals (jpeg.UnsupportedJpeg) and the malformed streams (jpeg.CorruptJpeg, never a partial image) are
jpeg.py's.  A header-level refusal raises before any launch; a malformed scan is found by the kernel and raises after the wait for
the batch's status words.  There is no fallback: without a GPU the decoder raises."""
import collections
import os

import numpy as np
import torch

from . import abi, hip, jpeg
from .staging import MAX_WORKERS

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_jhuff.h")
# the one declaration of the madtp_jhuff_* entry points; lib() sets them on jpeg.lib()'s handle: the IDCT and colour launches are its
SIGNATURES, DEFINES, lib = abi.bind("madtp_jhuff.h", "madtp_jhuff_abi_version", prefix="madtp_jhuff_", needs=jpeg.lib)
ABI_VERSION = DEFINES["MADTP_JHUFF_ABI_VERSION"]
FIELDS, STATUS_FIELDS, RECORD_BYTES = DEFINES["MADTP_JHUFF_FIELDS"], DEFINES["MADTP_JHUFF_STATUS_FIELDS"], DEFINES["MADTP_JHUFF_RECORD_BYTES"]
LANES, MAX_BYTES = DEFINES["MADTP_JHUFF_LANES"], DEFINES["MADTP_JHUFF_MAX_BYTES"]
_F = {k[len("MADTP_JHUFF_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JHUFF_F_")}
_S = {k[len("MADTP_JHUFF_S_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JHUFF_S_")}
_I, _JF = jpeg._I, jpeg._F
_SCANS = jpeg.ScanFormat(_F, FIELDS, RECORD_BYTES, MAX_BYTES)


def _check_subseq(subseq_bytes):
    s = 0 if subseq_bytes is None else int(subseq_bytes)
    if s < 0 or s % 4:
        raise ValueError(f"subseq_bytes={subseq_bytes!r} is not None / 0 (the library's choice) or a multiple of 4, at least 4")
    return s


class ScanImage:
    """What the host stage makes of one file: the file's bytes as they are (`data`, 1-D uint8), the header fields, `qtables` (uint16
    [3, 64], natural order), `tables` (the Huffman record the kernel reads, uint8 [RECORD_BYTES]) and `scan_begin`.  Plain numpy
    arrays and ints: it pickles from a loader worker to the main process."""
    __slots__ = ("data", "width", "height", "components", "hs", "vs", "blocks_x", "blocks_y", "restart_interval", "blocks", "qtables",
                 "tables", "scan_begin")

    def __init__(self, data, info, qtables, tables, scan_begin):
        self.data = data
        jpeg._set_header(self, info)
        self.blocks = int(info[_I["BLOCKS"]])
        self.qtables, self.tables, self.scan_begin = qtables, tables, int(scan_begin)

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, state):
        for k, v in state.items():
            setattr(self, k, v)


def prepare_scan(data, what="prepare_scan"):
    """bytes, a 1-D uint8 array or a path -> ScanImage.  Host only (no GPU state is touched, the scan is not read): usable in a
    DataLoader worker.  UnsupportedJpeg / CorruptJpeg name the reason of a header the decoder refuses."""
    import ctypes
    buf = jpeg._byte_array(data, what)
    info = np.zeros(jpeg.INFO_FIELDS, dtype=np.int32)
    q = np.zeros((3, 64), dtype=np.uint16)
    tables = np.zeros(RECORD_BYTES, dtype=np.uint8)
    scan = ctypes.c_int64(0)
    jpeg._raise(lib().madtp_jhuff_prepare(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data, tables.ctypes.data,
                                          ctypes.addressof(scan)), what)
    return ScanImage(buf, info, q, tables, scan.value)


def read(source, other="raise"):
    """a path or bytes -> ScanImage: the dataset's replacement for Image.open(path).convert('RGB').  other="pil": a file this
    decoder REFUSES by its header (UnsupportedJpeg) is decoded by Pillow to preprocess.raw_image()'s uint8 [h,w,3] tensor, which the
    decoder passes through; a corrupt header raises either way, a corrupt scan raises when the batch is decoded."""
    return jpeg._read_with(prepare_scan, source, other)


def decode_host(data, subseq_bytes=None):
    """The kernel's lane routines and passes with the lanes in a loop, on the host (madtp_jhuff_decode_host): -> (code, int16
    [blocks, 64] coefficients or None, int32 [STATUS_FIELDS] status).  For checking without a GPU; it is no decoder to use - the
    host's is jpeg.entropy_decode.  A header code comes back as the code, nothing is raised."""
    buf = jpeg._byte_array(data, "decode_host")
    info = np.zeros(jpeg.INFO_FIELDS, dtype=np.int32)
    q = np.zeros((3, 64), dtype=np.uint16)
    status = np.zeros(STATUS_FIELDS, dtype=np.int32)
    rc = lib().madtp_jpeg_inspect(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data)
    if rc:
        return rc, None, status
    coef = np.zeros((int(info[_I["BLOCKS"]]), 64), dtype=np.int16)
    rc = lib().madtp_jhuff_decode_host(buf.ctypes.data, buf.size, _check_subseq(subseq_bytes), coef.ctypes.data, coef.size, status.ctypes.data)
    return rc, coef if rc == 0 else None, status


class PreparedDeviceBatch(jpeg._Prepared, collections.namedtuple("PreparedDeviceBatch", "packed planes plan status subseq_bytes")):
    """what prepare() leaves on the device: the packed buffer of the plan (jpeg.JpegPlan), the plane scratch, the plan, the status
    words of the decode kernel and the subsequence size of its launch"""
    __slots__ = ()


class DeviceJpegDecoder(jpeg._BatchDecoder):
    """JPEG files -> uint8 [h,w,3] tensors on `device`, views of one packed buffer: one copy of the compressed bytes and three
    launches per batch (madtp_jhuff_decode_batch, madtp_jpeg_idct_batch, madtp_jpeg_rgb_batch).

    An item is the bytes of a file (its header is parsed here by `workers` threads - ctypes releases the GIL; at most MAX_WORKERS,
    never sized from the machine's CPU count), a ScanImage, or an already decoded uint8 [h,w,3] host array / tensor, which is copied
    through unchanged.  The files go into one of two pinned staging buffers (guarded by events) and one asynchronous copy on the
    current stream, which the launches follow.  The call waits for the status words of the decode kernel only - on a side stream,
    behind an event recorded after that kernel - and raises jpeg.CorruptJpeg naming the image if one is not 0.
    subseq_bytes: None for the library's choice per image, else the subsequence size of every image (tests force small ones)."""

    def __init__(self, device="cuda", workers=8, subseq_bytes=None):
        super().__init__(device, workers, "madtp-jhuff")
        self.subseq_bytes = _check_subseq(subseq_bytes)
        self._side = None
        self._host_status = None
        self.last_status = None  # int32 [coded images, STATUS_FIELDS] of the last batch (numpy), for tools and tests

    def prepare(self, items):
        """the header checks, the packing and the copy -> PreparedDeviceBatch for run()"""
        items = list(items)
        if len(items) < 1:
            raise ValueError("DeviceJpegDecoder: an empty batch")
        lib()  # (bound before the pool's threads call it)

        def parse(i):
            it = items[i]
            if isinstance(it, ScanImage):
                return it
            host = self._decoded(it, i)
            return host if host is not None else prepare_scan(jpeg._byte_array(it, f"image {i}"), f"image {i}")

        parsed = self._pool.map(parse, list(range(len(items))))  # (a header this decoder refuses raises here, before any launch)
        self._need_gpu("jpeg_device.decode_host runs the kernel's passes on the host for CPU checking.")
        decoded = {i: it for i, it in enumerate(parsed) if not isinstance(it, ScanImage)}
        plan = jpeg.plan_batch([("raw", it.shape) if i in decoded else ("coded", it, it.blocks, (it.data.size, it.scan_begin, it.tables.size))
                                for i, it in enumerate(parsed)], _SCANS)

        def fill(view, stage):
            for row, i in zip(plan.htable, plan.coded):
                it, record, file = parsed[i], int(row[_F["RECORD"]]), int(row[_F["FILE"]])
                view[record:record + RECORD_BYTES] = it.tables
                view[file:file + it.data.size] = it.data

        packed, planes = self._send(plan, decoded, fill)
        status = torch.empty(max(len(plan.coded), 1), STATUS_FIELDS, dtype=torch.int32, device=packed.device)
        return PreparedDeviceBatch(packed, planes, plan, status, self.subseq_bytes)

    @staticmethod
    def coefficients(batch):
        """-> the int16 [blocks, 64] coefficients of every coded image of a batch that has run, views of its packed buffer"""
        out, at = [], batch.coef_at
        for blocks in batch.blocks:
            out.append(batch.packed[at:at + 128 * blocks].view(torch.int16).view(blocks, 64))
            at += 128 * blocks
        return out

    def launches(self, batch):
        """-> [(entry point, launch(stream) -> code)] of a prepared batch, in order (tools time them one by one)"""
        h = lib()
        p, plan = batch.packed.data_ptr(), batch.plan
        if not plan.coded:
            return []
        return [("madtp_jhuff_decode_batch", lambda stream: h.madtp_jhuff_decode_batch(
            p, p + plan.htable_at, p + plan.coef_at, batch.status.data_ptr(), len(plan.coded), batch.subseq_bytes, stream))] + \
            self._pixel_launches(batch)

    def run(self, batch):
        """the three launches on the current stream and the wait for the status words -> list of uint8 [h,w,3] views of the batch's
        packed buffer; CorruptJpeg names the first image whose scan is malformed, and nothing is returned then"""
        with torch.cuda.device(batch.packed.device):
            cur = torch.cuda.current_stream()
            decoded = None
            for name, launch in self.launches(batch):
                hip._check(launch(cur.cuda_stream), name)
                if name == "madtp_jhuff_decode_batch":
                    decoded = torch.cuda.Event()
                    decoded.record(cur)
            if decoded is not None:
                n = len(batch.coded)
                with self._lock:
                    if self._side is None:
                        self._side = torch.cuda.Stream(device=batch.packed.device)
                    if self._host_status is None or self._host_status.shape[0] < n:
                        self._host_status = torch.empty(max(n, 64), STATUS_FIELDS, dtype=torch.int32, pin_memory=True)
                    side, host = self._side, self._host_status
                    side.wait_event(decoded)
                    batch.status.record_stream(side)
                    with torch.cuda.stream(side):
                        host[:n].copy_(batch.status[:n], non_blocking=True)
                    side.synchronize()
                    status = host[:n].numpy().copy()
                self.last_status = status
                for k, i in enumerate(batch.coded):
                    code = int(status[k, _S["CODE"]])
                    if code < -99:
                        jpeg._raise(code, f"image {i}")
                    elif code != 0:
                        hip._check(code, f"madtp_jhuff_decode_batch (image {i})")
        return self._images(batch)


# ---- the data loader's side ------------------------------------------------------------------------------------------------------
class RawJpegDeviceBatch(jpeg._DecodedBatch):
    """jpeg._DecodedBatch of what jpeg_device.read() makes (ScanImages, and raw uint8 [h,w,3] tensors of files that went to
    Pillow), decoded on the device: jpeg.RawJpegBatch's contract"""
    decoder, item = DeviceJpegDecoder, ScanImage


def collate(samples, then):
    """collate_fn (bind `then` with functools.partial): the ScanImages / raw images of the samples become one RawJpegDeviceBatch,
    everything else goes through torch's default_collate.  Samples are such images or tuples / lists that hold one."""
    return RawJpegDeviceBatch.collate(samples, then)
