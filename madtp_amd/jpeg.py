"""Baseline JPEG decode for the data loader (include/madtp_jpeg.h): Huffman entropy decoding on the host (csrc/jpeg_entropy.h, no GPU
state: a loader worker may run it), dequantisation + IDCT + chroma upsampling + YCbCr -> RGB on the device (csrc/jpeg.hip), with the
bytes of the reference's `Image.open(path).convert('RGB')` (Pillow = libjpeg-turbo: the islow IDCT, fancy upsampling).

    decoder = jpeg.JpegDecoder()                      # opt-in: the decoded-image interface of preprocess / augment stays as it is
    images = decoder([bytes0, bytes1, ...])           # -> uint8 [h,w,3] device tensors, views of one packed buffer
    x = preprocess.ImagePipeline(384)(images)         # ... which ImagePipeline / TrainTransform take as they are

    transform-free dataset:  sample = jpeg.read(path)                    # an EntropyImage (host tensors), made in the worker
    collate_fn = functools.partial(jpeg.collate, then=functools.partial(preprocess.ImagePipeline, 384))
    image = image.to(device, non_blocking=True)       # the RawJpegBatch decodes and runs `then`: the drivers' line stays as it is

Accepted: SOF0 / SOF1 8-bit Huffman files of one interleaved scan, grayscale or YCbCr 4:4:4 / 4:2:2 / 4:2:0, sides up to 8192.
Everything else is UnsupportedJpeg naming the reason (read(..., other="pil") hands such a file to Pillow instead); a malformed
stream is CorruptJpeg, never a partial image.  There is no fallback: without a GPU the decoder raises."""
import collections
import functools
import os
import threading

import numpy as np
import torch

from . import abi, hip, preprocess, staging
from .staging import MAX_WORKERS, align as _align

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_jpeg.h")
# the one declaration of the madtp_jpeg_* entry points; lib() is hip.load()'s handle with them set on it (no GPU needed)
SIGNATURES, DEFINES, lib = abi.bind("madtp_jpeg.h", "madtp_jpeg_abi_version")
ABI_VERSION = DEFINES["MADTP_JPEG_ABI_VERSION"]
FIELDS, INFO_FIELDS = DEFINES["MADTP_JPEG_FIELDS"], DEFINES["MADTP_JPEG_INFO_FIELDS"]
_F = {k[len("MADTP_JPEG_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JPEG_F_")}
_I = {k[len("MADTP_JPEG_I_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JPEG_I_")}


class UnsupportedJpeg(ValueError):
    """a valid JPEG of a kind this decoder refuses (progressive, CMYK, ...)"""


class CorruptJpeg(ValueError):
    """a malformed JPEG stream"""


def _raise(code, what):
    if code == 0:
        return
    msg = lib().madtp_jpeg_strerror(code).decode()
    if -200 < code <= -100:
        raise UnsupportedJpeg(f"{what}: {msg} (code {code}); there is no fallback")
    if -300 < code <= -200:
        raise CorruptJpeg(f"{what}: {msg} (code {code})")
    raise RuntimeError(f"{what} failed: {msg} (code {code})")


def _byte_array(data, what="data"):
    """bytes / bytearray / memoryview / 1-D uint8 array or CPU tensor / path -> contiguous 1-D numpy uint8"""
    if isinstance(data, (str, os.PathLike)):
        with open(data, "rb") as f:
            data = f.read()
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    if torch.is_tensor(data) and data.dtype == torch.uint8 and data.dim() == 1 and not data.is_cuda:
        return np.ascontiguousarray(data.numpy())
    if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1:
        return np.ascontiguousarray(data)
    raise ValueError(f"{what}: {type(data).__name__} is not bytes, a 1-D uint8 array or a path")


def _set_header(image, info):
    """the header fields an EntropyImage and a jpeg_device.ScanImage share, from the int32 [INFO_FIELDS] of madtp_jpeg_inspect"""
    image.width, image.height, image.components = int(info[_I["WIDTH"]]), int(info[_I["HEIGHT"]]), int(info[_I["COMPONENTS"]])
    image.hs, image.vs = int(info[_I["HS"]]), int(info[_I["VS"]])
    image.blocks_x, image.blocks_y, image.restart_interval = int(info[_I["BLOCKS_X"]]), int(info[_I["BLOCKS_Y"]]), int(info[_I["RESTART"]])


class EntropyImage:
    """What the host stage makes of one file: the header fields, `qtables` (uint16 [3, 64], natural order, rows of absent components
    0) and `coef` (int16 [blocks, 64]: component after component, each [blocks_y, blocks_x] blocks, column-major within a block).
    Plain CPU tensors: it pickles from a loader worker to the main process."""
    __slots__ = ("width", "height", "components", "hs", "vs", "blocks_x", "blocks_y", "restart_interval", "qtables", "coef")

    def __init__(self, info, qtables, coef):
        _set_header(self, info)
        self.qtables, self.coef = qtables, coef

    def __getstate__(self):  # (torch's pickling has no uint16 storage: the small table travels as a numpy array)
        state = {k: getattr(self, k) for k in self.__slots__}
        state["qtables"] = state["qtables"].numpy() if torch.is_tensor(state["qtables"]) else state["qtables"]
        return state

    def __setstate__(self, state):
        for k, v in state.items():
            setattr(self, k, torch.from_numpy(v) if k == "qtables" and isinstance(v, np.ndarray) else v)

    @property
    def blocks(self):
        """(blocks_y, blocks_x) of every component"""
        chroma = (self.blocks_y // self.vs, self.blocks_x // self.hs)
        return [(self.blocks_y, self.blocks_x)] + [chroma] * (self.components - 1)

    def component(self, c):
        """int16 [blocks_y, blocks_x, 8, 8] view of component c in natural order (row, column)"""
        shapes = self.blocks
        start = sum(y * x for y, x in shapes[:c])
        y, x = shapes[c]
        return self.coef[start:start + y * x].view(y, x, 8, 8).transpose(2, 3)


def _inspect(buf, what):
    info = np.zeros(INFO_FIELDS, dtype=np.int32)
    q = np.zeros((3, 64), dtype=np.uint16)
    _raise(lib().madtp_jpeg_inspect(buf.ctypes.data, buf.size, info.ctypes.data, q.ctypes.data), what)
    return info, q


def entropy_decode(data, what="entropy_decode"):
    """bytes, a 1-D uint8 array or a path -> EntropyImage.  Host only (no GPU state is touched): usable in a DataLoader worker.
    UnsupportedJpeg / CorruptJpeg name the reason."""
    buf = _byte_array(data, what)
    info, q = _inspect(buf, what)
    coef = torch.empty(int(info[_I["BLOCKS"]]), 64, dtype=torch.int16)
    _raise(lib().madtp_jpeg_entropy_decode(buf.ctypes.data, buf.size, coef.data_ptr(), coef.numel()), what)
    return EntropyImage(info, torch.from_numpy(q), coef)


def _read_with(stage, source, other):
    """read() of this module and of jpeg_device: `stage` is the host stage, entropy_decode or jpeg_device.prepare_scan"""
    if other not in ("raise", "pil"):
        raise ValueError(f"read: other={other!r} is not 'raise' or 'pil'")
    buf = _byte_array(source, "read")
    try:
        return stage(buf, str(source) if isinstance(source, (str, os.PathLike)) else "read")
    except UnsupportedJpeg:
        if other != "pil":
            raise
    import io
    from PIL import Image
    return preprocess.raw_image(Image.open(io.BytesIO(buf.tobytes())))


def read(source, other="raise"):
    """a path or bytes -> EntropyImage: the dataset's replacement for Image.open(path).convert('RGB').  other="pil": a file this
    decoder REFUSES (UnsupportedJpeg: progressive, CMYK, ...) is decoded by Pillow to preprocess.raw_image()'s uint8 [h,w,3] tensor,
    which the decoder passes through; a corrupt file raises either way."""
    return _read_with(entropy_decode, source, other)


# ---- the layout of a batch ---------------------------------------------------------------------------------------------------------
# what plan_batch needs of madtp_jhuff.h (jpeg_device hands it over: this module does not read that header)
ScanFormat = collections.namedtuple("ScanFormat", "F FIELDS RECORD_BYTES MAX_BYTES")

# One device buffer per batch, for both decoders:
#   [ table | quantisation tables | decode-kernel table || coefficients (host route) or Huffman records and files (device route) |
#     decoded pass-through images ]    <- staged and copied, copy_bytes in all; everything before || is `head`
#   [ coefficients the decode kernel writes (device route) ]    at coef_at
#   [ decoded images ]                                          at out_at .. total
# Records and coefficients lie at multiples of 4 bytes (they do of 16), files and images of 16, planes and the two device-made
# regions of 256.  shapes: per image ((h, w), offset of its pixels in the buffer); blocks: of every coded image, in `coded`'s order.
JpegPlan = collections.namedtuple("JpegPlan", "B head table htable table_bytes qtable_at htable_at coded blocks copy_bytes coef_at out_at "
                                              "total plane_bytes workspace n_idct n_rgb shapes")


_ROW = [_F[k] for k in "COEF QTABLE PLANES OUT W H COMPONENTS HS VS BLOCKS_X BLOCKS_Y".split()]
_HROW = "FILE SIZE SCAN RECORD COEF COMPONENTS HS VS BLOCKS_X BLOCKS_Y RESTART".split()


def plan_batch(items, scans=None):
    """The one place that lays a batch out and fills the MADTP_JPEG_F_* rows (and, with `scans`, a ScanFormat, the MADTP_JHUFF_F_*
    rows of the device route).  Host arithmetic only, with the library's own size queries.  items: per image ("raw", shape) or
    ("coded", header, blocks it claims to have or None, None or (file bytes, scan_begin, Huffman record bytes)), where header has the
    fields of an EntropyImage.  ValueError naming the image whose fields contradict each other."""
    h = lib()
    B = len(items)
    table = np.zeros((B, FIELDS), dtype=np.int64)
    qtables = np.zeros((B, 3, 8, 8), dtype=np.uint16)
    qtable_at, htable_at = table.nbytes, table.nbytes + qtables.nbytes
    coded, rows, hrows, qs, blocks, firsts, places = [], [], [], [], [], [], []
    coef_bytes = plane_at = plane_sum = raw_bytes = out_bytes = n_idct = n_rgb = 0
    at = htable_at + (8 * scans.FIELDS * sum(it[0] == "coded" for it in items) if scans else 0)  # the end of `head`
    for i, it in enumerate(items):
        # every row has a place in both grids (the search wants non-decreasing prefixes); a decoded image has no workgroup, and the
        # rest of its row is never read
        firsts.append((n_idct, n_rgb))
        if it[0] == "raw":
            hh, ww = int(it[1][0]), int(it[1][1])
            raw_bytes = _align(raw_bytes, 16)
            places.append((hh, ww, raw_bytes))
            raw_bytes += 3 * hh * ww
            continue
        _, im, claimed, scan = it
        geometry = (im.components, im.hs, im.vs, im.blocks_x, im.blocks_y)
        nb = int(h.madtp_jpeg_blocks(*geometry))
        ok = nb >= 1 and claimed in (None, nb) and 1 <= im.width <= 8 * im.blocks_x and 1 <= im.height <= 8 * im.blocks_y
        if scans is not None:
            file_bytes, scan_begin, record_bytes = scan
            ok = ok and 0 <= scan_begin <= file_bytes <= scans.MAX_BYTES and record_bytes == scans.RECORD_BYTES
        if not ok:
            raise ValueError(f"image {i}: {'an EntropyImage' if scans is None else 'a ScanImage'} whose fields contradict each other")
        planes, plane_bytes = _align(plane_at, 256), int(h.madtp_jpeg_plane_bytes(*geometry))
        coded.append(i)
        rows.append((coef_bytes, 384 * i, planes, out_bytes, im.width, im.height) + geometry)
        qs.append(im.qtables.numpy() if torch.is_tensor(im.qtables) else im.qtables)
        if scans is not None:
            record = _align(at, 16)
            at = record + record_bytes + file_bytes  # (a record is a multiple of 16 bytes: the file behind it is aligned as it is)
            hrows.append((record + record_bytes, file_bytes, scan_begin, record, coef_bytes) + geometry + (im.restart_interval,))
        places.append((im.height, im.width, out_bytes))
        blocks.append(nb)
        coef_bytes += 128 * nb
        plane_at, plane_sum = planes + plane_bytes, plane_sum + plane_bytes
        out_bytes += _align(int(h.madtp_jpeg_out_bytes(im.width, im.height)), 16)
        n_idct += h.madtp_jpeg_idct_groups(nb)
        n_rgb += h.madtp_jpeg_rgb_groups(im.width, im.height)
    if scans is None:  # the host route stages the coefficients themselves
        coef_at, at = at, at + coef_bytes
    raw_at = _align(at, 16)
    copy_bytes = at = raw_at + raw_bytes if len(coded) < B else at  # (without a decoded image nothing a launch does not read is copied)
    if scans is not None:
        coef_at = _align(at, 256)
        at = coef_at + coef_bytes
    out_at = _align(at, 256)
    htable = np.zeros((len(coded), scans.FIELDS) if scans else (0, 1), dtype=np.int64)
    table[:, [_F["FIRST_IDCT"], _F["FIRST_RGB"]]] = firsts
    if coded:
        table[np.ix_(coded, _ROW)] = rows
        qtables[coded] = np.asarray(qs, dtype=np.uint16).reshape(-1, 3, 8, 8).transpose(0, 1, 3, 2)  # column-major, as the coefficients
        if scans is not None:
            htable[:, [scans.F[k] for k in _HROW]] = hrows
    head = np.concatenate([a.reshape(-1).view(np.uint8) for a in (table, qtables, htable)])
    shapes = [((hh, ww), (out_at if it[0] == "coded" else raw_at) + o) for it, (hh, ww, o) in zip(items, places)]
    return JpegPlan(B, head, table, htable, table.nbytes, qtable_at, htable_at, coded, blocks, copy_bytes, coef_at, out_at, out_at + out_bytes,
                    plane_sum, int(h.madtp_jpeg_workspace(B, plane_sum)), n_idct, n_rgb, shapes)


class _Prepared:
    """a prepared batch reads its plan's fields as its own: batch.B, batch.shapes, batch.table_bytes, batch.out_at, batch.copy_bytes"""
    __slots__ = ()

    def __getattr__(self, name):
        return getattr(self.plan, name)


class PreparedJpegBatch(_Prepared, collections.namedtuple("PreparedJpegBatch", "packed planes plan")):
    """what prepare() leaves on the device: the packed buffer of the plan, the plane scratch, and the plan with the launches' arguments"""
    __slots__ = ()


class _BatchDecoder:
    """What JpegDecoder and jpeg_device.DeviceJpegDecoder share: the pool, the staging ring (two pinned buffers guarded by events, as
    ImagePipeline's), the one copy of a planned batch, and the IDCT and colour launches."""

    def __init__(self, device, workers, thread_name):
        self.device = torch.device(device)
        self._pool = staging.Pool(workers, thread_name)
        self.workers = self._pool.workers
        self._ring = staging.StagingRing()
        self._lock = threading.Lock()

    def __call__(self, items):
        return self.run(self.prepare(items))

    @staticmethod
    def _decoded(it, i):
        """an already decoded uint8 [h,w,3] item -> its host array, None for an item of another kind"""
        if not ((torch.is_tensor(it) or isinstance(it, np.ndarray)) and it.ndim == 3):
            return None
        host, _ = preprocess._as_uint8_hw3(it, i)
        if host is None:
            raise ValueError(f"image {i}: a decoded image must be a host array (device images need no decoder)")
        return host

    def _need_gpu(self, for_cpu_checking):
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} on {self.device}: madtp_amd runs only on an MI355X through the HIP kernels (no CPU / "
                               f"eager fallback).  {for_cpu_checking}")

    def _send(self, plan, decoded, fill):
        """the plan's head, the decoded images {index: host array} and what fill(view, stage) writes go into the next staging buffer
        and, in one asynchronous copy on the current stream, to the device -> (packed buffer, plane scratch)"""
        with self._lock, torch.cuda.device(self.device if self.device.index is not None else torch.cuda.current_device()):
            device = torch.device("cuda", torch.cuda.current_device())
            turn, stage = self._ring.acquire(plan.copy_bytes)
            view = stage.numpy()
            view[:plan.head.size] = plan.head
            for i, host in decoded.items():
                o = plan.shapes[i][1]
                np.copyto(view[o:o + host.size].reshape(host.shape), host)
            fill(view, stage)  # (an exception of any item surfaces here, before the copy and the launches)
            packed = torch.empty(max(plan.total, 1), dtype=torch.uint8, device=device)
            packed[:plan.copy_bytes].copy_(stage[:plan.copy_bytes], non_blocking=True)
            self._ring.sent(turn)
            planes = torch.empty(max(plan.workspace, 1), dtype=torch.uint8, device=device)
        return packed, planes

    def _pixel_launches(self, batch):
        h = lib()
        p, plan = batch.packed.data_ptr(), batch.plan
        if not plan.n_idct:
            return []
        return [("madtp_jpeg_idct_batch", lambda stream: h.madtp_jpeg_idct_batch(
                    p + plan.coef_at, p + plan.qtable_at, p, batch.planes.data_ptr(), plan.B, plan.n_idct, stream)),
                ("madtp_jpeg_rgb_batch", lambda stream: h.madtp_jpeg_rgb_batch(
                    batch.planes.data_ptr(), p, p + plan.out_at, plan.B, plan.n_rgb, stream))]

    @staticmethod
    def _images(batch):
        return [batch.packed[o:o + 3 * hh * ww].view(hh, ww, 3) for (hh, ww), o in batch.plan.shapes]


class JpegDecoder(_BatchDecoder):
    """JPEG files -> uint8 [h,w,3] tensors on `device`, views of one packed buffer: one copy and two launches per batch.

    An item is an EntropyImage, the bytes of a file (entropy-decoded here by `workers` threads - ctypes releases the GIL; at most
    MAX_WORKERS, never sized from the machine's CPU count) or an already decoded uint8 [h,w,3] host array / tensor, which is copied
    through unchanged.  Coefficients go into one of two pinned staging buffers (guarded by events, as ImagePipeline's) and one
    asynchronous copy on the current stream, which the two launches follow.  Every item is checked before anything is launched."""

    def __init__(self, device="cuda", workers=8):
        super().__init__(device, workers, "madtp-jpeg")

    def prepare(self, items):
        """the checks, the entropy decode of byte items, the packing and the copy -> PreparedJpegBatch for run()"""
        items = list(items)
        if len(items) < 1:
            raise ValueError("JpegDecoder: an empty batch")
        h = lib()
        facts, files, decoded = [], {}, {}  # plan_batch's items; the bytes of the items that are files; the decoded images
        for i, it in enumerate(items):
            if not isinstance(it, EntropyImage):
                host = self._decoded(it, i)
                if host is not None:
                    decoded[i] = host
                    facts.append(("raw", host.shape))
                    continue
                files[i] = _byte_array(it, f"image {i}")
                it = EntropyImage(*_inspect(files[i], f"image {i}"), None)
            claimed = None if it.coef is None else int(it.coef.shape[0]) if tuple(it.coef.shape[1:]) == (64,) else -1
            facts.append(("coded", it, claimed, None))
        self._need_gpu("tests/jpeg_ref.py restates the arithmetic for CPU checking.")
        plan = plan_batch(facts)

        def fill(view, stage):
            def one(job):
                i, blocks = job
                o = plan.coef_at + int(plan.table[i, _F["COEF"]])
                if i in files:  # straight into the pinned buffer
                    buf = files[i]
                    _raise(h.madtp_jpeg_entropy_decode(buf.ctypes.data, buf.size, stage.data_ptr() + o, 64 * blocks), f"image {i}")
                else:
                    np.copyto(view[o:o + 128 * blocks].view(np.int16).reshape(-1, 64), facts[i][1].coef.numpy())

            self._pool.map(one, list(zip(plan.coded, plan.blocks)))

        return PreparedJpegBatch(*self._send(plan, decoded, fill), plan)

    def launches(self, batch):
        """-> [(entry point, launch(stream) -> code)] of a prepared batch, in order (tools time them one by one)"""
        return self._pixel_launches(batch)

    def run(self, batch):
        """the two launches on the current stream -> list of uint8 [h,w,3] views of the batch's packed buffer"""
        with torch.cuda.device(batch.packed.device):
            for name, launch in self.launches(batch):
                hip._check(launch(torch.cuda.current_stream().cuda_stream), name)
        return self._images(batch)


# ---- the data loader's side ------------------------------------------------------------------------------------------------------
_decoders = {}
_thens = {}


def _factory_key(then):
    """a functools.partial by value (every batch of a loader with worker processes brings its own unpickled copy), else by identity"""
    if isinstance(then, functools.partial):
        try:
            key = (then.func, then.args, tuple(sorted(then.keywords.items())))
            hash(key)
            return key
        except TypeError:
            pass
    return id(then)


class _DecodedBatch:
    """The images of a batch as a read() made them in the workers.  to(device) decodes them with one `decoder` per device and hands
    the device images to `then`: an ImagePipeline / TrainTransform instance, or a factory of one called as then(device=device)
    (functools.partial(preprocess.ImagePipeline, 384): what a loader with worker processes needs, since an instance does not pickle)
    - so a driver's `image = image.to(device, non_blocking=True)` works unchanged."""
    decoder = item = None  # the decoder's class and the class of a coded item: a subclass names them

    def __init__(self, items, then):
        self.items, self.then = list(items), then

    def __len__(self):
        return len(self.items)

    @classmethod
    def collate(cls, samples, then):
        is_item = lambda x: isinstance(x, cls.item) or preprocess._is_raw(x)
        return preprocess.collate_with(samples, is_item, lambda col: cls(col, then))

    def to(self, device, non_blocking=False, **_):
        device = torch.device(device)
        if (self.decoder, str(device)) not in _decoders:
            _decoders[self.decoder, str(device)] = self.decoder(device)
        then = self.then
        if not hasattr(then, "prepare") and not hasattr(then, "last_plan"):  # a factory, not an instance
            key = (_factory_key(then), str(device))
            if key not in _thens:
                _thens[key] = (then, then(device=device))  # (the factory is kept: an id in the key stays taken)
            then = _thens[key][1]
        return then(_decoders[self.decoder, str(device)](self.items))

    def cuda(self, device=None, non_blocking=False):
        return self.to("cuda" if device is None else device)


class RawJpegBatch(_DecodedBatch):
    """_DecodedBatch of what jpeg.read() makes: EntropyImages, and raw uint8 [h,w,3] tensors of files that went to Pillow"""
    decoder, item = JpegDecoder, EntropyImage


def collate(samples, then):
    """collate_fn (bind `then` with functools.partial): the EntropyImages / raw images of the samples become one RawJpegBatch,
    everything else goes through torch's default_collate.  Samples are such images or tuples / lists that hold one."""
    return RawJpegBatch.collate(samples, then)
