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
import concurrent.futures
import os
import threading

import numpy as np
import torch

from . import abi, hip, jpeg, preprocess

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_jhuff.h")
with open(HEADER) as _f:
    SIGNATURES, _, DEFINES = abi.parse(_f.read())  # the one declaration of the madtp_jhuff_* entry points
SIGNATURES = {k: v for k, v in SIGNATURES.items() if k.startswith("madtp_jhuff_")}
ABI_VERSION = DEFINES["MADTP_JHUFF_ABI_VERSION"]
FIELDS, STATUS_FIELDS, RECORD_BYTES = DEFINES["MADTP_JHUFF_FIELDS"], DEFINES["MADTP_JHUFF_STATUS_FIELDS"], DEFINES["MADTP_JHUFF_RECORD_BYTES"]
LANES, MAX_BYTES = DEFINES["MADTP_JHUFF_LANES"], DEFINES["MADTP_JHUFF_MAX_BYTES"]
_F = {k[len("MADTP_JHUFF_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JHUFF_F_")}
_S = {k[len("MADTP_JHUFF_S_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JHUFF_S_")}
_I, _JF = jpeg._I, jpeg._F
MAX_WORKERS = 16

_bound = False


def lib():
    """hip.load()'s handle with the madtp_jhuff_* (and madtp_jpeg_*) signatures set on it (no GPU needed)"""
    global _bound
    h = jpeg.lib()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError => header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if h.madtp_jhuff_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libmadtp_hip jhuff ABI {h.madtp_jhuff_abi_version()} != binding {ABI_VERSION}; rebuild")
        _bound = True
    return h


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
        self.width, self.height, self.components = int(info[_I["WIDTH"]]), int(info[_I["HEIGHT"]]), int(info[_I["COMPONENTS"]])
        self.hs, self.vs = int(info[_I["HS"]]), int(info[_I["VS"]])
        self.blocks_x, self.blocks_y, self.restart_interval = int(info[_I["BLOCKS_X"]]), int(info[_I["BLOCKS_Y"]]), int(info[_I["RESTART"]])
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
    if other not in ("raise", "pil"):
        raise ValueError(f"read: other={other!r} is not 'raise' or 'pil'")
    buf = jpeg._byte_array(source, "read")
    try:
        return prepare_scan(buf, str(source) if isinstance(source, (str, os.PathLike)) else "read")
    except jpeg.UnsupportedJpeg:
        if other != "pil":
            raise
    import io
    from PIL import Image
    return preprocess.raw_image(Image.open(io.BytesIO(buf.tobytes())))


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


def _align(n, a):
    return (n + a - 1) // a * a


# what prepare() leaves on the device: one buffer [tables and files as staged | coefficients | decoded images], the plane scratch,
# the status words, and the launches' host arguments
PreparedDeviceBatch = collections.namedtuple(
    "PreparedDeviceBatch", "packed planes status jtable_at qtable_at htable_at coef_at out_at B coded blocks n_idct n_rgb shapes copy_bytes subseq_bytes")


class DeviceJpegDecoder:
    """JPEG files -> uint8 [h,w,3] tensors on `device`, views of one packed buffer: one copy of the compressed bytes and three
    launches per batch (madtp_jhuff_decode_batch, madtp_jpeg_idct_batch, madtp_jpeg_rgb_batch).

    An item is the bytes of a file (its header is parsed here by `workers` threads - ctypes releases the GIL; at most MAX_WORKERS,
    never sized from the machine's CPU count), a ScanImage, or an already decoded uint8 [h,w,3] host array / tensor, which is copied
    through unchanged.  The files go into one of two pinned staging buffers (guarded by events) and one asynchronous copy on the
    current stream, which the launches follow.  The call waits for the status words of the decode kernel only - on a side stream,
    behind an event recorded after that kernel - and raises jpeg.CorruptJpeg naming the image if one is not 0.
    subseq_bytes: None for the library's choice per image, else the subsequence size of every image (tests force small ones)."""

    def __init__(self, device="cuda", workers=8, subseq_bytes=None):
        self.device = torch.device(device)
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.subseq_bytes = _check_subseq(subseq_bytes)
        self._pool = None
        self._stage = [None, None]
        self._events = [None, None]
        self._turn = 0
        self._side = None
        self._host_status = None
        self._lock = threading.Lock()
        self.last_status = None  # int32 [coded images, STATUS_FIELDS] of the last batch (numpy), for tools and tests

    def _staging(self, nbytes):
        i = self._turn
        self._turn ^= 1
        if self._events[i] is not None:
            self._events[i].synchronize()
        if self._stage[i] is None or self._stage[i].numel() < nbytes:
            self._stage[i] = torch.empty(max(nbytes, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
        return i, self._stage[i]

    def _map(self, fn, jobs):
        if self.workers == 1 or len(jobs) < 2:
            return [fn(j) for j in jobs]
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(self.workers, thread_name_prefix="madtp-jhuff")
        futures = [self._pool.submit(fn, j) for j in jobs]
        concurrent.futures.wait(futures)
        return [f.result() for f in futures]

    def __call__(self, items):
        return self.run(self.prepare(items))

    def prepare(self, items):
        """the header checks, the packing and the copy -> PreparedDeviceBatch for run()"""
        items = list(items)
        B = len(items)
        if B < 1:
            raise ValueError("DeviceJpegDecoder: an empty batch")
        h = lib()

        def parse(i):
            it = items[i]
            if isinstance(it, ScanImage):
                return ("scan", it)
            if (torch.is_tensor(it) or isinstance(it, np.ndarray)) and it.ndim == 3:
                host, _ = preprocess._as_uint8_hw3(it, i)
                if host is None:
                    raise ValueError(f"image {i}: a decoded image must be a host array (device images need no decoder)")
                return ("raw", host)
            return ("scan", prepare_scan(jpeg._byte_array(it, f"image {i}"), f"image {i}"))

        kinds = self._map(parse, list(range(B)))  # (a header this decoder refuses raises here, before any launch)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"DeviceJpegDecoder on {self.device}: madtp_amd runs only on an MI355X through the HIP kernels (no CPU / "
                               "eager fallback).  jpeg_device.decode_host runs the kernel's passes on the host for CPU checking.")
        with self._lock, torch.cuda.device(self.device if self.device.index is not None else torch.cuda.current_device()):
            device = torch.device("cuda", torch.cuda.current_device())
            coded = [i for i, (kind, _) in enumerate(kinds) if kind == "scan"]
            jtable = np.zeros((B, jpeg.FIELDS), dtype=np.int64)        # rows of the IDCT and colour kernels: every image
            htable = np.zeros((max(len(coded), 1), FIELDS), dtype=np.int64)  # rows of the decode kernel: the coded images
            jtable_at, qtable_at = 0, jtable.nbytes
            htable_at = qtable_at + B * 384
            at = _align(htable_at + htable.nbytes, 16)
            coef_bytes, plane_at, plane_sum, n_idct, n_rgb = 0, 0, 0, 0, 0
            for n, i in enumerate(coded):
                it = kinds[i][1]
                blocks = int(h.madtp_jpeg_blocks(it.components, it.hs, it.vs, it.blocks_x, it.blocks_y))
                if blocks < 1 or blocks != it.blocks or not (1 <= it.width <= 8 * it.blocks_x and 1 <= it.height <= 8 * it.blocks_y) or \
                        not 0 <= it.scan_begin <= it.data.size <= MAX_BYTES or it.tables.size != RECORD_BYTES:
                    raise ValueError(f"image {i}: a ScanImage whose fields contradict each other")
                row = htable[n]
                row[_F["RECORD"]], at = at, at + RECORD_BYTES
                row[_F["FILE"]], at = at, _align(at + it.data.size, 16)
                row[_F["SIZE"]], row[_F["SCAN"]], row[_F["COEF"]] = it.data.size, it.scan_begin, coef_bytes
                row[_F["COMPONENTS"]], row[_F["HS"]], row[_F["VS"]] = it.components, it.hs, it.vs
                row[_F["BLOCKS_X"]], row[_F["BLOCKS_Y"]], row[_F["RESTART"]] = it.blocks_x, it.blocks_y, it.restart_interval
                jrow = jtable[i]
                jrow[_JF["COEF"]], jrow[_JF["QTABLE"]], jrow[_JF["PLANES"]] = coef_bytes, i * 384, _align(plane_at, 256)
                jrow[_JF["W"]], jrow[_JF["H"]], jrow[_JF["COMPONENTS"]] = it.width, it.height, it.components
                jrow[_JF["HS"]], jrow[_JF["VS"]], jrow[_JF["BLOCKS_X"]], jrow[_JF["BLOCKS_Y"]] = it.hs, it.vs, it.blocks_x, it.blocks_y
                coef_bytes += 128 * blocks
                plane_bytes = 64 * blocks
                plane_at, plane_sum = int(jrow[_JF["PLANES"]]) + plane_bytes, plane_sum + plane_bytes
            raw_at = _align(at, 16)
            raw_bytes = 0
            for i, (kind, it) in enumerate(kinds):
                if kind == "raw":
                    jtable[i, _JF["OUT"]] = raw_bytes
                    raw_bytes += _align(it.size, 16)
            copy_bytes = raw_at + raw_bytes
            coef_at = _align(copy_bytes, 256)
            out_at = _align(coef_at + coef_bytes, 256)
            total = 0
            shapes = []
            for i, (kind, it) in enumerate(kinds):
                jrow = jtable[i]
                jrow[_JF["FIRST_IDCT"]], jrow[_JF["FIRST_RGB"]] = n_idct, n_rgb
                if kind == "scan":
                    jrow[_JF["OUT"]] = total
                    shapes.append(((it.height, it.width), out_at + total))
                    total += _align(int(h.madtp_jpeg_out_bytes(it.width, it.height)), 16)
                    n_idct += h.madtp_jpeg_idct_groups(it.blocks)
                    n_rgb += h.madtp_jpeg_rgb_groups(it.width, it.height)
                else:
                    shapes.append((it.shape[:2], raw_at + int(jrow[_JF["OUT"]])))
            turn, stage = self._staging(copy_bytes)
            view = stage.numpy()
            view[jtable_at:jtable_at + jtable.nbytes] = jtable.view(np.uint8).reshape(-1)
            view[htable_at:htable_at + htable.nbytes] = htable.view(np.uint8).reshape(-1)
            qview = view[qtable_at:qtable_at + B * 384].view(np.uint16).reshape(B, 3, 8, 8)
            qview[:] = 0
            for n, i in enumerate(coded):
                it = kinds[i][1]
                qview[i] = np.asarray(it.qtables, dtype=np.uint16).reshape(3, 8, 8).transpose(0, 2, 1)  # column-major, as the coefficients
                o = int(htable[n, _F["RECORD"]])
                view[o:o + RECORD_BYTES] = it.tables
                o = int(htable[n, _F["FILE"]])
                view[o:o + it.data.size] = it.data
            for i, (kind, it) in enumerate(kinds):
                if kind == "raw":
                    o = raw_at + int(jtable[i, _JF["OUT"]])
                    np.copyto(view[o:o + it.size].reshape(it.shape), it)
            packed = torch.empty(max(out_at + total, 1), dtype=torch.uint8, device=device)
            packed[:copy_bytes].copy_(stage[:copy_bytes], non_blocking=True)
            if self._events[turn] is None:
                self._events[turn] = torch.cuda.Event()
            self._events[turn].record()
            planes = torch.empty(max(int(h.madtp_jpeg_workspace(B, plane_sum)), 1), dtype=torch.uint8, device=device)
            status = torch.empty(max(len(coded), 1), STATUS_FIELDS, dtype=torch.int32, device=device)
        return PreparedDeviceBatch(packed, planes, status, jtable_at, qtable_at, htable_at, coef_at, out_at, B, coded,
                                   [kinds[i][1].blocks for i in coded], n_idct, n_rgb, shapes, copy_bytes, self.subseq_bytes)

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
        p = batch.packed.data_ptr()
        todo = []
        if batch.coded:
            todo.append(("madtp_jhuff_decode_batch", lambda stream: h.madtp_jhuff_decode_batch(
                p, p + batch.htable_at, p + batch.coef_at, batch.status.data_ptr(), len(batch.coded), batch.subseq_bytes, stream)))
            # (a raw image's OUT row is never read: it has no workgroup in either grid)
            todo.append(("madtp_jpeg_idct_batch", lambda stream: h.madtp_jpeg_idct_batch(
                p + batch.coef_at, p + batch.qtable_at, p + batch.jtable_at, batch.planes.data_ptr(), batch.B, batch.n_idct, stream)))
            todo.append(("madtp_jpeg_rgb_batch", lambda stream: h.madtp_jpeg_rgb_batch(
                batch.planes.data_ptr(), p + batch.jtable_at, p + batch.out_at, batch.B, batch.n_rgb, stream)))
        return todo

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
        return [batch.packed[o:o + 3 * hh * ww].view(hh, ww, 3) for (hh, ww), o in batch.shapes]


# ---- the data loader's side ------------------------------------------------------------------------------------------------------
_decoders = {}
_thens = {}


def _is_item(x):
    return isinstance(x, ScanImage) or preprocess._is_raw(x)


class RawJpegDeviceBatch:
    """The images of a batch as jpeg_device.read() made them in the workers (ScanImages, and raw uint8 [h,w,3] tensors of files
    that went to Pillow).  to(device) decodes them on the device and hands the images to `then`: an ImagePipeline / TrainTransform
    instance, or a factory of one called as then(device=device) - jpeg.RawJpegBatch's contract."""

    def __init__(self, items, then):
        self.items, self.then = list(items), then

    def __len__(self):
        return len(self.items)

    def to(self, device, non_blocking=False, **_):
        device = torch.device(device)
        if str(device) not in _decoders:
            _decoders[str(device)] = DeviceJpegDecoder(device)
        then = self.then
        if not hasattr(then, "prepare") and not hasattr(then, "last_plan"):  # a factory, not an instance
            key = (jpeg._factory_key(then), str(device))
            if key not in _thens:
                _thens[key] = (then, then(device=device))
            then = _thens[key][1]
        return then(_decoders[str(device)](self.items))

    def cuda(self, device=None, non_blocking=False):
        return self.to("cuda" if device is None else device)


def collate(samples, then):
    """collate_fn (bind `then` with functools.partial): the ScanImages / raw images of the samples become one RawJpegDeviceBatch,
    everything else goes through torch's default_collate.  Samples are such images or tuples / lists that hold one."""
    from torch.utils.data import default_collate
    first = samples[0]
    if _is_item(first):
        return RawJpegDeviceBatch(samples, then)
    if isinstance(first, (tuple, list)):
        return [RawJpegDeviceBatch(col, then) if _is_item(col[0]) else default_collate(list(col)) for col in zip(*samples)]
    return default_collate(samples)
