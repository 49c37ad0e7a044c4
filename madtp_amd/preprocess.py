"""The image stage of the data loader on the device (include/madtp_image.h, csrc/image.hip): decoded uint8 RGB images of
different sizes -> the normalised f32 [B,3,S,S] batch a model takes, with the bits of the reference's PIL bicubic Resize +
ToTensor + Normalize (data/__init__.py:29-33, clip/clip.py:80-88) and a uint8 instead of an f32 host-to-device copy.

    pipe = ImagePipeline(384)                       # BLIP: Resize((S, S));  mode="short_side_crop": CLIP's Resize(S) + CenterCrop(S)
    x = pipe([img0, img1, ...])                     # uint8 [h,w,3] numpy arrays / tensors / PIL RGB images -> f32 [B,3,S,S] on the GPU

    transform = preprocess.raw_image                # in a dataset: keep the decoded bytes ...
    collate_fn = functools.partial(preprocess.collate, size=384)   # ... and the loader's batch is a RawImageBatch, whose
    image = image.to(device, non_blocking=True)     # .to(device) runs the pipeline: the drivers' line stays as it is

Pillow's resampling is integer arithmetic on fixed-point coefficients; resample_tables() restates how Resample.c makes them, in
IEEE double on the host (on the device FMA contraction would change bits), and the kernel does the two integer passes.  There is
no fallback: without a GPU the pipeline raises, and an unsupported image is a ValueError naming it."""
import collections
import math
import os
import threading

import numpy as np
import torch

from . import abi, hip, staging

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_image.h")
# the one declaration of the image entry points, as abi.SIGNATURES is of madtp_hip.h; lib() is hip.load()'s handle with them set
SIGNATURES, DEFINES, lib = abi.bind("madtp_image.h", "madtp_image_abi_version")
ABI_VERSION = DEFINES["MADTP_IMAGE_ABI_VERSION"]
FIELDS, MAX_KSIZE = DEFINES["MADTP_IMAGE_FIELDS"], DEFINES["MADTP_IMAGE_MAX_KSIZE"]
_F = {k[len("MADTP_IMAGE_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_IMAGE_F_")}
MAX_SIDE = 8192

# the constants of both reference families (data/__init__.py:20, clip/clip.py:87)
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


# ---- Pillow's coefficient tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc) -----------------------------------------
PRECISION_BITS = 22
_tables = {}


def resample_tables(in_size, out_size, box=None):
    """-> (int32 [out, ksize] coefficients with 22 fractional bits, int32 [out, 2] (xmin, n)) of one axis of PIL's bicubic resize
    from in_size to out_size pixels, optionally of the box [in0, in1) of that axis (Image.resize(box=...)).  Every double operation
    is Pillow's, in its order; numpy's elementwise operations round each one as C does.  Cached: the arrays are read-only."""
    key = (int(in_size), int(out_size), None if box is None else (float(box[0]), float(box[1])))
    if key in _tables:
        return _tables[key]
    in_size, out_size = key[0], key[1]
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resample_tables: sizes must be positive, got {in_size} -> {out_size}")
    in0, in1 = (0.0, float(in_size)) if box is None else key[2]
    scale = fs = (in1 - in0) / out_size
    if fs < 1.0:
        fs = 1.0
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = in0 + (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # (astype truncates toward zero, as the C cast does)
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    if n.min() < 1:
        raise ValueError(f"resample_tables: box {box} leaves an output pixel of {in_size} -> {out_size} without a source pixel")
    i = np.arange(ksize, dtype=np.int64)[None, :]
    x = np.abs(((i + xmin[:, None]) - center[:, None] + 0.5) * ss)
    a = -0.5
    w = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))
    w = np.where(i < n[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):  # the sequential sum (a masked 0.0 leaves it as it is)
        ww = ww + w[:, j]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    one = float(1 << PRECISION_BITS)
    k = np.where(w < 0.0, (-0.5 + w * one).astype(np.int64), (0.5 + w * one).astype(np.int64)).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    k.setflags(write=False)
    bounds.setflags(write=False)
    if len(_tables) >= 4096:
        _tables.clear()
    _tables[key] = (k, bounds)
    return k, bounds


def normalize_table(mean=MEAN, std=STD):
    """f32 [3, 256]: ToTensor (f32(v) / 255) and Normalize ((t - mean) / std) of every byte, with torch's own CPU operations in
    torchvision's order, each rounded to f32"""
    t = torch.arange(256, dtype=torch.float32).div(255)
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return t[None, :].sub(m[:, None]).div(s[:, None]).contiguous()


def short_side_geometry(w, h, size):
    """CLIP's Resize(size) + CenterCrop(size) of a w x h image -> (resized w, resized h, crop left, crop top).

    Restated from torchvision (the resized long side is int(size * long / short), a crop offset int(round((n - size) / 2.0)));
    torchvision is not part of this project's environment, so the two formulas are NOT verified against it."""
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    return nw, nh, int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))


# ---- device copies of the tables -------------------------------------------------------------------------------------------------
_DEV_TABLES_MAX = 1024
_dev_tables = collections.OrderedDict()  # (in, out, box, device) -> (coefficients, bounds) on the device: datasets have few sizes


def _device_tables(in_size, out_size, device):
    key = (in_size, out_size, None, str(device))
    hit = _dev_tables.get(key)
    if hit is None:
        k, bounds = resample_tables(in_size, out_size)
        hit = (torch.from_numpy(k.copy()).to(device), torch.from_numpy(bounds.copy()).to(device))
        _dev_tables[key] = hit
        if len(_dev_tables) > _DEV_TABLES_MAX:
            _dev_tables.popitem(last=False)
    else:
        _dev_tables.move_to_end(key)
    return hit


def _as_uint8_hw3(img, index):
    """one input image -> (numpy uint8 [h,w,3] view or None, device tensor or None)"""
    if torch.is_tensor(img):
        arr = img
    elif isinstance(img, np.ndarray):
        arr = img
    elif hasattr(img, "mode") and hasattr(img, "size"):  # a PIL image
        if img.mode != "RGB":
            raise ValueError(f"image {index}: PIL mode {img.mode!r}, only RGB images are supported (convert('RGB') first)")
        arr = np.asarray(img)
    else:
        raise ValueError(f"image {index}: {type(img).__name__} is not a numpy array, a tensor or a PIL image")
    if arr.dtype != (torch.uint8 if torch.is_tensor(arr) else np.uint8):
        raise ValueError(f"image {index}: dtype {arr.dtype}, only uint8 images are supported")
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"image {index}: shape {tuple(arr.shape)}, only [h, w, 3] RGB images are supported")
    h, w = int(arr.shape[0]), int(arr.shape[1])
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"image {index}: {w} x {h}, sides must be 1 .. {MAX_SIDE}")
    if torch.is_tensor(arr):
        return (None, arr) if arr.is_cuda else (arr.numpy(), None)
    return arr, None


# what prepare() leaves on the device: the table and the packed source bytes in one buffer, and the launch's host arguments
PreparedBatch = collections.namedtuple("PreparedBatch", "packed table_bytes B n_blocks max_ksize lut")


class ImagePipeline:
    """uint8 RGB images -> normalised f32 [B,3,Sh,Sw] on `device`, one copy and one launch per batch.

    size: S or (Sh, Sw); mode "stretch" = Resize((Sh, Sw)) (BLIP), "short_side_crop" = Resize(S) + CenterCrop(S) (CLIP, S only).
    CPU inputs are packed into one of two pinned staging buffers (guarded by events: packing batch n+1 does not wait for batch
    n) and sent with one asynchronous copy on the current stream, which the launch follows."""

    def __init__(self, size, mode="stretch", mean=MEAN, std=STD, device="cuda"):
        self.Sh, self.Sw = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if self.Sh < 1 or self.Sw < 1:
            raise ValueError(f"ImagePipeline: size {size} must be positive")
        if mode not in ("stretch", "short_side_crop"):
            raise ValueError(f"ImagePipeline: unknown mode {mode!r}")
        if mode == "short_side_crop" and self.Sh != self.Sw:
            raise ValueError("ImagePipeline: short_side_crop takes one size S (Resize(S) + CenterCrop(S))")
        self.mode = mode
        self.device = torch.device(device)
        self.table = normalize_table(mean, std)
        self._lut = None
        self._ring = staging.StagingRing()
        self._lock = threading.Lock()

    def _axes(self, w, h, index):
        """-> ((in, virtual out, window start) for x, the same for y), after the ratio check"""
        if self.mode == "stretch":
            ax, ay = (w, self.Sw, 0), (h, self.Sh, 0)
        else:
            nw, nh, left, top = short_side_geometry(w, h, self.Sw)
            ax, ay = (w, nw, left), (h, nh, top)
        for n_in, n_out, _ in (ax, ay):
            ksize = int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
            if ksize > MAX_KSIZE:
                raise ValueError(f"image {index}: {w} x {h} -> {n_out} pixels is a downscale ratio of {n_in / n_out:.2f}, beyond "
                                 f"the supported 16")
        return ax, ay

    def __call__(self, images, boxes=None, flips=None, out=None):
        """images: list of uint8 [h,w,3] numpy arrays, CPU tensors, PIL RGB images, or uint8 tensors on the device (all of them
        then); boxes: per image None or PIL's crop box (left, upper, right, lower) - crop, then resize; flips: per image bool -
        resize, then flip left-right; out: an f32 [B,3,Sh,Sw] tensor on the device to write into."""
        return self.run(self.prepare(images, boxes, flips), out)

    def prepare(self, images, boxes=None, flips=None):
        """the checks, the packing and the copy of __call__ -> PreparedBatch for run() (a batch can be run more than once)"""
        images = list(images)
        B = len(images)
        if B < 1:
            raise ValueError("ImagePipeline: an empty batch")
        boxes = [None] * B if boxes is None else list(boxes)
        flips = [False] * B if flips is None else list(flips)
        if len(boxes) != B or len(flips) != B:
            raise ValueError(f"ImagePipeline: {B} images, {len(boxes)} boxes, {len(flips)} flips")
        items = []
        for i, img in enumerate(images):
            host, dev = _as_uint8_hw3(img, i)
            h, w = (host if dev is None else dev).shape[:2]
            l, u, r, d = (0, 0, w, h) if boxes[i] is None else boxes[i]
            if any(int(v) != v for v in (l, u, r, d)) or not (0 <= l < r <= w and 0 <= u < d <= h):
                raise ValueError(f"image {i}: crop box {boxes[i]} is not an integer box inside {w} x {h}")
            l, u, r, d = int(l), int(u), int(r), int(d)
            items.append((host, dev, (l, u, r, d), self._axes(r - l, d - u, i)))
        on_device = [it[1] is not None for it in items]
        if any(on_device) and not all(on_device):
            raise ValueError(f"image {on_device.index(True)}: a device tensor in a batch of CPU images (a batch is one or the other)")
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"ImagePipeline on {self.device}: madtp_amd runs only on an MI355X through the HIP kernels (no CPU / "
                               "eager fallback).  tests/image_ref.py restates the arithmetic for CPU checking.")
        h = lib()
        with self._lock, torch.cuda.device(self.device if self.device.index is not None else torch.cuda.current_device()):
            device = torch.device("cuda", torch.cuda.current_device())
            if self._lut is None or self._lut.device != device:
                self._lut = self.table.to(device)
            table = np.zeros((B, FIELDS), dtype=np.int64)
            tb = table.nbytes
            offset, n_blocks, max_ksize = 0, 0, 1
            for i, (host, dev, (l, u, r, d), (ax, ay)) in enumerate(items):
                bw, bh = r - l, d - u
                row = table[i]
                if dev is None:  # the box's pixels are packed: its rows follow one another
                    row[_F["OFFSET"]], row[_F["STRIDE"]] = offset, 3 * bw
                    offset += 3 * bw * bh
                else:  # the whole image is packed: the box is an offset and the image's stride
                    full_w = int(dev.shape[1])
                    row[_F["OFFSET"]], row[_F["STRIDE"]] = offset + 3 * (u * full_w + l), 3 * full_w
                    offset += dev.numel()
                row[_F["W"]], row[_F["H"]] = bw, bh
                for (n_in, n_out, start), fk, fb, fs in ((ax, "KX", "BX", "KSX"), (ay, "KY", "BY", "KSY")):
                    k, bounds = _device_tables(n_in, n_out, device)
                    ksize = k.shape[1]
                    row[_F[fk]], row[_F[fb]], row[_F[fs]] = k.data_ptr() + 4 * start * ksize, bounds.data_ptr() + 8 * start, ksize
                    max_ksize = max(max_ksize, ksize)
                tile_h = h.madtp_image_tile_rows(ay[0] / ay[1], int(row[_F["KSY"]]))
                if tile_h < 1:
                    raise ValueError(f"image {i}: no tile height fits a row table of {int(row[_F['KSY']])} coefficients")
                row[_F["FLIP"]], row[_F["TILE_H"]], row[_F["FIRST"]] = int(bool(flips[i])), tile_h, n_blocks
                n_blocks += h.madtp_image_blocks(self.Sh, self.Sw, tile_h)
            turn, stage = self._ring.acquire(tb + (0 if all(on_device) else offset))
            view = stage.numpy()
            view[:tb] = table.view(np.uint8).reshape(-1)
            packed = torch.empty(tb + offset, dtype=torch.uint8, device=device)
            if all(on_device):
                packed[:tb].copy_(stage[:tb], non_blocking=True)
                torch.cat([it[1].reshape(-1) for it in items], out=packed[tb:])
            else:
                for i, (host, _, (l, u, r, d), _) in enumerate(items):
                    o = tb + int(table[i, _F["OFFSET"]])
                    np.copyto(view[o:o + 3 * (r - l) * (d - u)].reshape(d - u, r - l, 3), host[u:d, l:r])
                packed.copy_(stage[:tb + offset], non_blocking=True)
            self._ring.sent(turn)
        return PreparedBatch(packed, tb, B, n_blocks, max_ksize, self._lut)

    def run(self, batch, out=None):
        """the launch on the current stream -> f32 [B,3,Sh,Sw]"""
        B = batch.B
        if out is None:
            out = torch.empty(B, 3, self.Sh, self.Sw, dtype=torch.float32, device=batch.packed.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, 3, self.Sh, self.Sw)):
            raise ValueError(f"out must be a contiguous f32 [{B}, 3, {self.Sh}, {self.Sw}] tensor on the device")
        with torch.cuda.device(batch.packed.device):
            p = batch.packed.data_ptr()
            hip._check(lib().madtp_image_resize_batch(p + batch.table_bytes, p, batch.lut.data_ptr(), out.data_ptr(), B, self.Sh, self.Sw,
                                                      batch.n_blocks, batch.max_ksize, torch.cuda.current_stream().cuda_stream),
                       "madtp_image_resize_batch")
        return out


# ---- the data loader's side ------------------------------------------------------------------------------------------------------
def raw_image(pil):
    """dataset transform in place of Resize + ToTensor + Normalize: the decoded RGB image as a uint8 [h,w,3] tensor"""
    if getattr(pil, "mode", "RGB") != "RGB":
        pil = pil.convert("RGB")
    return torch.from_numpy(np.array(pil, dtype=np.uint8))


_pipelines = {}


class RawImageBatch:
    """The images of a batch as the dataset decoded them, of different sizes.  to(device) runs the pipeline and returns the f32
    [B,3,S,S] tensor, so a driver's `image = image.to(device, non_blocking=True)` works unchanged."""

    def __init__(self, images, size, mode="stretch", mean=MEAN, std=STD):
        self.images, self.size, self.mode, self.mean, self.std = list(images), size, mode, tuple(mean), tuple(std)

    def __len__(self):
        return len(self.images)

    def to(self, device, non_blocking=False, **_):
        device = torch.device(device)
        key = (str(device), self.size if isinstance(self.size, int) else tuple(self.size), self.mode, self.mean, self.std)
        if key not in _pipelines:
            _pipelines[key] = ImagePipeline(self.size, self.mode, self.mean, self.std, device)
        return _pipelines[key](self.images)

    def cuda(self, device=None, non_blocking=False):
        return self.to("cuda" if device is None else device)


def _is_raw(x):
    return torch.is_tensor(x) and x.dtype == torch.uint8 and x.dim() == 3 and x.shape[2] == 3


def collate_with(samples, is_item, make):
    """the body of every collate_fn of the image input path: the columns of the samples whose entries are items (is_item) become
    make(column), everything else goes through torch's default_collate.  Samples are items or tuples / lists that hold one."""
    from torch.utils.data import default_collate
    first = samples[0]
    if is_item(first):
        return make(samples)
    if isinstance(first, (tuple, list)):
        return [make(col) if is_item(col[0]) else default_collate(list(col)) for col in zip(*samples)]
    return default_collate(samples)


def collate(samples, size, mode="stretch", mean=MEAN, std=STD):
    """collate_fn (bind `size` with functools.partial): the raw uint8 [h,w,3] images of the samples become one RawImageBatch,
    everything else goes through torch's default_collate.  Samples are raw images or tuples / lists that hold one."""
    return collate_with(samples, _is_raw, lambda col: RawImageBatch(col, size, mode, mean, std))
