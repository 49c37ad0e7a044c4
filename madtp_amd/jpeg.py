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
import concurrent.futures
import functools
import os
import threading

import numpy as np
import torch

from . import abi, hip, preprocess

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_jpeg.h")
with open(HEADER) as _f:
    SIGNATURES, _, DEFINES = abi.parse(_f.read())  # the one declaration of the madtp_jpeg_* entry points
ABI_VERSION = DEFINES["MADTP_JPEG_ABI_VERSION"]
FIELDS, INFO_FIELDS = DEFINES["MADTP_JPEG_FIELDS"], DEFINES["MADTP_JPEG_INFO_FIELDS"]
_F = {k[len("MADTP_JPEG_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JPEG_F_")}
_I = {k[len("MADTP_JPEG_I_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_JPEG_I_")}
MAX_WORKERS = 16

_bound = False


class UnsupportedJpeg(ValueError):
    """a valid JPEG of a kind this decoder refuses (progressive, CMYK, ...)"""


class CorruptJpeg(ValueError):
    """a malformed JPEG stream"""


def lib():
    """hip.load()'s handle with the madtp_jpeg_* signatures set on it (no GPU needed)"""
    global _bound
    h = hip.load()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError => header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if h.madtp_jpeg_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libmadtp_hip jpeg ABI {h.madtp_jpeg_abi_version()} != binding {ABI_VERSION}; rebuild")
        _bound = True
    return h


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


class EntropyImage:
    """What the host stage makes of one file: the header fields, `qtables` (uint16 [3, 64], natural order, rows of absent components
    0) and `coef` (int16 [blocks, 64]: component after component, each [blocks_y, blocks_x] blocks, column-major within a block).
    Plain CPU tensors: it pickles from a loader worker to the main process."""
    __slots__ = ("width", "height", "components", "hs", "vs", "blocks_x", "blocks_y", "restart_interval", "qtables", "coef")

    def __init__(self, info, qtables, coef):
        self.width, self.height, self.components = int(info[_I["WIDTH"]]), int(info[_I["HEIGHT"]]), int(info[_I["COMPONENTS"]])
        self.hs, self.vs = int(info[_I["HS"]]), int(info[_I["VS"]])
        self.blocks_x, self.blocks_y, self.restart_interval = int(info[_I["BLOCKS_X"]]), int(info[_I["BLOCKS_Y"]]), int(info[_I["RESTART"]])
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


def read(source, other="raise"):
    """a path or bytes -> EntropyImage: the dataset's replacement for Image.open(path).convert('RGB').  other="pil": a file this
    decoder REFUSES (UnsupportedJpeg: progressive, CMYK, ...) is decoded by Pillow to preprocess.raw_image()'s uint8 [h,w,3] tensor,
    which the decoder passes through; a corrupt file raises either way."""
    if other not in ("raise", "pil"):
        raise ValueError(f"read: other={other!r} is not 'raise' or 'pil'")
    buf = _byte_array(source, "read")
    try:
        return entropy_decode(buf, str(source) if isinstance(source, (str, os.PathLike)) else "read")
    except UnsupportedJpeg:
        if other != "pil":
            raise
    import io
    from PIL import Image
    return preprocess.raw_image(Image.open(io.BytesIO(buf.tobytes())))


def _align(n, a):
    return (n + a - 1) // a * a


class JpegDecoder:
    """JPEG files -> uint8 [h,w,3] tensors on `device`, views of one packed buffer: one copy and two launches per batch.

    An item is an EntropyImage, the bytes of a file (entropy-decoded here by `workers` threads - ctypes releases the GIL; at most
    MAX_WORKERS, never sized from the machine's CPU count) or an already decoded uint8 [h,w,3] host array / tensor, which is copied
    through unchanged.  Coefficients go into one of two pinned staging buffers (guarded by events, as ImagePipeline's) and one
    asynchronous copy on the current stream, which the two launches follow.  Every item is checked before anything is launched."""

    def __init__(self, device="cuda", workers=8):
        self.device = torch.device(device)
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self._pool = None
        self._stage = [None, None]
        self._events = [None, None]
        self._turn = 0
        self._lock = threading.Lock()

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
            self._pool = concurrent.futures.ThreadPoolExecutor(self.workers, thread_name_prefix="madtp-jpeg")
        futures = [self._pool.submit(fn, j) for j in jobs]
        concurrent.futures.wait(futures)  # all of them: a failed batch leaves no thread writing into the staging buffer
        return [f.result() for f in futures]

    def __call__(self, items):
        return self.run(self.prepare(items))

    def prepare(self, items):
        """the checks, the entropy decode of byte items, the packing and the copy -> PreparedJpegBatch for run()"""
        items = list(items)
        B = len(items)
        if B < 1:
            raise ValueError("JpegDecoder: an empty batch")
        h = lib()
        kinds = []  # per item ("coef", EntropyImage, the file's bytes or None) / ("raw", numpy [h,w,3], None)
        for i, it in enumerate(items):
            if isinstance(it, EntropyImage):
                kinds.append(("coef", it, None))
            elif (torch.is_tensor(it) or isinstance(it, np.ndarray)) and it.ndim == 3:
                host, dev = preprocess._as_uint8_hw3(it, i)
                if host is None:
                    raise ValueError(f"image {i}: a decoded image must be a host array (device images need no decoder)")
                kinds.append(("raw", host, None))
            else:
                buf = _byte_array(it, f"image {i}")
                info, q = _inspect(buf, f"image {i}")
                kinds.append(("coef", EntropyImage(info, q, None), buf))
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"JpegDecoder on {self.device}: madtp_amd runs only on an MI355X through the HIP kernels (no CPU / "
                               "eager fallback).  tests/jpeg_ref.py restates the arithmetic for CPU checking.")
        with self._lock, torch.cuda.device(self.device if self.device.index is not None else torch.cuda.current_device()):
            device = torch.device("cuda", torch.cuda.current_device())
            table = np.zeros((B, FIELDS), dtype=np.int64)
            tb = table.nbytes
            qb = B * 3 * 64 * 2
            # the layout: [table | quantisation tables | coefficients | decoded pass-through images] is staged and copied, the
            # decoded outputs follow in the same device buffer; the planes are scratch of their own
            blocks = [0] * B
            coef_at, plane_at, plane_sum, raw_bytes = 0, 0, 0, 0
            for i, (kind, it, _) in enumerate(kinds):
                if kind == "raw":
                    continue
                row = table[i]
                blocks[i] = int(h.madtp_jpeg_blocks(it.components, it.hs, it.vs, it.blocks_x, it.blocks_y))
                if blocks[i] < 1 or not (1 <= it.width <= 8 * it.blocks_x and 1 <= it.height <= 8 * it.blocks_y) or \
                        (it.coef is not None and tuple(it.coef.shape) != (blocks[i], 64)):
                    raise ValueError(f"image {i}: an EntropyImage whose fields contradict each other")
                row[_F["COEF"]], row[_F["QTABLE"]], row[_F["PLANES"]] = coef_at, i * 384, _align(plane_at, 256)
                row[_F["W"]], row[_F["H"]], row[_F["COMPONENTS"]] = it.width, it.height, it.components
                row[_F["HS"]], row[_F["VS"]], row[_F["BLOCKS_X"]], row[_F["BLOCKS_Y"]] = it.hs, it.vs, it.blocks_x, it.blocks_y
                coef_at += 128 * blocks[i]
                plane_bytes = int(h.madtp_jpeg_plane_bytes(it.components, it.hs, it.vs, it.blocks_x, it.blocks_y))
                plane_at, plane_sum = int(row[_F["PLANES"]]) + plane_bytes, plane_sum + plane_bytes
            out_at = _align(tb + qb + coef_at, 256)
            for i, (kind, it, _) in enumerate(kinds):
                if kind == "raw":
                    table[i, _F["OUT"]] = out_at + raw_bytes
                    raw_bytes += _align(it.size, 16)
            copy_bytes = out_at + raw_bytes if raw_bytes else tb + qb + coef_at
            total = out_at + raw_bytes
            n_idct, n_rgb = 0, 0
            for i, (kind, it, _) in enumerate(kinds):
                row = table[i]
                # every row has a place in both grids (the search wants non-decreasing prefixes); a decoded image has no workgroup
                row[_F["FIRST_IDCT"]], row[_F["FIRST_RGB"]] = n_idct, n_rgb
                if kind == "coef":
                    row[_F["OUT"]] = total
                    total += _align(int(h.madtp_jpeg_out_bytes(it.width, it.height)), 16)
                    n_idct += h.madtp_jpeg_idct_groups(blocks[i])
                    n_rgb += h.madtp_jpeg_rgb_groups(it.width, it.height)
            turn, stage = self._staging(copy_bytes)
            view = stage.numpy()
            dev_table = table.copy()
            dev_table[:, _F["OUT"]] -= out_at  # `out` of the launches is the packed buffer past the staged part
            view[:tb] = dev_table.view(np.uint8).reshape(-1)
            qview = view[tb:tb + qb].view(np.uint16).reshape(B, 3, 8, 8)
            base = tb + qb

            def fill(i):
                kind, it, buf = kinds[i]
                if kind == "raw":
                    o = int(table[i, _F["OUT"]])
                    np.copyto(view[o:o + it.size].reshape(it.shape), it)
                    return
                q = np.asarray(it.qtables.numpy() if torch.is_tensor(it.qtables) else it.qtables, dtype=np.uint16)
                qview[i] = q.reshape(3, 8, 8).transpose(0, 2, 1)  # column-major, as the coefficients are
                o = base + int(table[i, _F["COEF"]])
                n = 128 * blocks[i]
                if buf is None:
                    np.copyto(view[o:o + n].view(np.int16).reshape(-1, 64), it.coef.numpy())
                else:
                    _raise(h.madtp_jpeg_entropy_decode(buf.ctypes.data, buf.size, stage.data_ptr() + o, n // 2), f"image {i}")

            self._map(fill, list(range(B)))  # (an exception of any item surfaces here, before the copy and the launches)
            packed = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
            packed[:copy_bytes].copy_(stage[:copy_bytes], non_blocking=True)
            if self._events[turn] is None:
                self._events[turn] = torch.cuda.Event()
            self._events[turn].record()
            planes = torch.empty(max(int(h.madtp_jpeg_workspace(B, plane_sum)), 1), dtype=torch.uint8, device=device)
        shapes = [((it.height, it.width) if kind == "coef" else it.shape[:2], int(table[i, _F["OUT"]])) for i, (kind, it, _) in enumerate(kinds)]
        return PreparedJpegBatch(packed, planes, tb, qb, out_at, B, n_idct, n_rgb, shapes)

    def launches(self, batch):
        """-> [(entry point, launch(stream) -> code)] of a prepared batch, in order (tools time them one by one)"""
        h = lib()
        p = batch.packed.data_ptr()
        todo = []
        if batch.n_idct:
            todo.append(("madtp_jpeg_idct_batch", lambda stream: h.madtp_jpeg_idct_batch(
                p + batch.table_bytes + batch.qtable_bytes, p + batch.table_bytes, p, batch.planes.data_ptr(), batch.B, batch.n_idct, stream)))
            todo.append(("madtp_jpeg_rgb_batch", lambda stream: h.madtp_jpeg_rgb_batch(
                batch.planes.data_ptr(), p, p + batch.out_at, batch.B, batch.n_rgb, stream)))
        return todo

    def run(self, batch):
        """the two launches on the current stream -> list of uint8 [h,w,3] views of the batch's packed buffer"""
        with torch.cuda.device(batch.packed.device):
            for name, launch in self.launches(batch):
                hip._check(launch(torch.cuda.current_stream().cuda_stream), name)
        return [batch.packed[o:o + 3 * hh * ww].view(hh, ww, 3) for (hh, ww), o in batch.shapes]


# what prepare() leaves on the device: table, quantisation tables, coefficients and decoded pass-through images in one buffer (the
# decoded outputs follow in the same buffer), the plane scratch, and the launches' host arguments
PreparedJpegBatch = collections.namedtuple("PreparedJpegBatch", "packed planes table_bytes qtable_bytes out_at B n_idct n_rgb shapes")


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


def _is_item(x):
    return isinstance(x, EntropyImage) or preprocess._is_raw(x)


class RawJpegBatch:
    """The images of a batch as jpeg.read() made them in the workers (EntropyImages, and raw uint8 [h,w,3] tensors of files that
    went to Pillow).  to(device) decodes them and hands the device images to `then`: an ImagePipeline / TrainTransform instance, or
    a factory of one called as then(device=device) (functools.partial(preprocess.ImagePipeline, 384): what a loader with worker
    processes needs, since an instance does not pickle) - so a driver's `image = image.to(device, non_blocking=True)` works
    unchanged."""

    def __init__(self, items, then):
        self.items, self.then = list(items), then

    def __len__(self):
        return len(self.items)

    def to(self, device, non_blocking=False, **_):
        device = torch.device(device)
        if str(device) not in _decoders:
            _decoders[str(device)] = JpegDecoder(device)
        then = self.then
        if not hasattr(then, "prepare") and not hasattr(then, "last_plan"):  # a factory, not an instance
            key = (_factory_key(then), str(device))
            if key not in _thens:
                _thens[key] = (then, then(device=device))  # (the factory is kept: an id in the key stays taken)
            then = _thens[key][1]
        return then(_decoders[str(device)](self.items))

    def cuda(self, device=None, non_blocking=False):
        return self.to("cuda" if device is None else device)


def collate(samples, then):
    """collate_fn (bind `then` with functools.partial): the EntropyImages / raw images of the samples become one RawJpegBatch,
    everything else goes through torch's default_collate.  Samples are such images or tuples / lists that hold one."""
    from torch.utils.data import default_collate
    first = samples[0]
    if _is_item(first):
        return RawJpegBatch(samples, then)
    if isinstance(first, (tuple, list)):
        return [RawJpegBatch(col, then) if _is_item(col[0]) else default_collate(list(col)) for col in zip(*samples)]
    return default_collate(samples)
