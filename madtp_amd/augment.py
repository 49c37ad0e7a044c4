"""The TRAINING transform of the data loader on the device (include/madtp_augment.h, csrc/augment.hip): decoded uint8 RGB images of
different sizes -> the normalised f32 [B,3,Sh,Sw] batch of the reference's training loaders (data/__init__.py:21-28),

    RandomResizedCrop(S, scale=(0.5, 1), BICUBIC) -> RandomHorizontalFlip -> RandomAugment(2, 5, augs=[ten names]) -> ToTensor -> Normalize

    tf = augment.TrainTransform(384)                 # draws a crop box, a flip and up to N ops per image
    x = tf([img0, img1, ...])                        # uint8 [h,w,3] arrays / tensors / PIL RGB images -> f32 [B,3,S,S] on the GPU
    x = tf(images, boxes=..., flips=..., ops=...)    # explicit: per image a list of (name, args), as tf.last_plan["ops"] holds them

    transform = preprocess.raw_image                 # in a dataset: keep the decoded bytes ...
    collate_fn = functools.partial(augment.collate, size=384)   # ... the loader's batch is a RawTrainBatch, whose .to(device) runs it

The crop, the Pillow-exact resize and the flip are preprocess.ImagePipeline's (the same table rows and host packing), stored as
bytes; every RandAugment stage then runs for the whole batch at once, each image with its own op: a histogram launch where an op
needs the whole image (Equalize, AutoContrast) and an apply launch (copy, byte table, affine warp), the last of which normalises.
The host draws and builds tables; it never holds an f32 image.  Byte ops have the reference's bits (tests/golden/augment_ref.npz).
The three warps (shear, translate, rotate) follow THIS project's fixed-point definition in madtp_augment.h, modelled on OpenCV's
warpAffine, which is not part of this project's environment: they are NOT verified against OpenCV.  There is no fallback: without
a GPU the call raises, Sharpness at a factor other than 1.0 (cv2.filter2D) and ops outside the configured ten are ValueErrors."""
import math
import os

import numpy as np
import torch

from . import abi, hip, preprocess
from .preprocess import MEAN, STD

HEADER = os.path.join(os.path.dirname(abi.HEADER), "madtp_augment.h")
# the one declaration of the madtp_augment_* entry points; lib() sets them on preprocess.lib()'s handle (the resize is the image stage's)
SIGNATURES, DEFINES, lib = abi.bind("madtp_augment.h", "madtp_augment_abi_version", needs=preprocess.lib)
ABI_VERSION = DEFINES["MADTP_AUGMENT_ABI_VERSION"]
FIELDS, MAX_PIXELS, FILL = DEFINES["MADTP_AUGMENT_FIELDS"], DEFINES["MADTP_AUGMENT_MAX_PIXELS"], DEFINES["MADTP_AUGMENT_FILL"]
_F_OP, _F_TABLE, _F_A0 = DEFINES["MADTP_AUGMENT_F_OP"], DEFINES["MADTP_AUGMENT_F_TABLE"], DEFINES["MADTP_AUGMENT_F_A0"]
OP_COPY, OP_TABLE, OP_EQUALIZE, OP_AUTOCONTRAST, OP_WARP = (DEFINES["MADTP_AUGMENT_OP_" + n] for n in
                                                            "COPY TABLE EQUALIZE AUTOCONTRAST WARP".split())

# the ten names of the reference's training loaders, in their order (np.random.choice indexes this list)
REFERENCE_AUGS = ("Identity", "AutoContrast", "Brightness", "Sharpness", "Equalize", "ShearX", "ShearY", "TranslateX", "TranslateY",
                  "Rotate")
MAX_LEVEL, TRANSLATE_CONST, REPLACE = 10, 10, (FILL, FILL, FILL)  # transform/randaugment.py's constants

# ---- the draws ---------------------------------------------------------------------------------------------------------------------
def level_to_args(name, level, rng):
    """transform/randaugment.py's arg_dict[name](level), its sign draw taken from `rng`"""
    if name in ("Identity", "AutoContrast", "Equalize"):
        return ()
    if name in ("Brightness", "Sharpness"):
        return ((level / MAX_LEVEL) * 1.8 + 0.1,)
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        v = (level / MAX_LEVEL) * (0.3 if name.startswith("Shear") else float(TRANSLATE_CONST))
        if rng.random() > 0.5:
            v = -v
        return (v, REPLACE)
    if name == "Rotate":
        v = (level / MAX_LEVEL) * 30
        if rng.random() < 0.5:
            v = -v
        return (v, REPLACE)
    raise ValueError(f"op {name!r} is not one of the supported {', '.join(REFERENCE_AUGS)}")


class RandAugmentSampler:
    """The draws of the reference's RandomAugment(N, M, augs) from a numpy RandomState, in its order: choice(augs, N); per op
    random() > 0.5 skips it; then the op's own sign draw.  With the same seeded state, sample() is the list of (name, args) the
    reference hands to its functions (skipped ops are absent: they are copies in the plan)."""

    def __init__(self, N=2, M=5, augs=REFERENCE_AUGS, rng=None):
        self.N, self.M, self.augs = int(N), M, list(augs)
        for name in self.augs:
            if name not in REFERENCE_AUGS:
                raise ValueError(f"op {name!r} is not one of the supported {', '.join(REFERENCE_AUGS)}")
        if self.N < 0 or (self.N and not self.augs):
            raise ValueError(f"RandAugmentSampler: N = {N} ops of {len(self.augs)} names")
        self.rng = np.random.RandomState() if rng is None else rng
        self._names = np.array(self.augs)  # (what choice() makes of the list, once)

    def sample(self):
        calls = []
        for name in (self.rng.choice(self._names, self.N) if self.N else ()):
            if self.rng.random() > 0.5:
                continue
            calls.append((str(name), level_to_args(str(name), self.M, self.rng)))
        return calls


def random_resized_crop_box(w, h, scale=(0.5, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """-> PIL crop box (left, upper, right, lower) of a w x h image, drawn from the torch `generator`.

    Restated from torchvision's RandomResizedCrop.get_params: ten attempts at an area uniform in `scale` of the image's and an
    aspect ratio log-uniform in `ratio`, then the centre crop at the nearest allowed ratio.  torchvision is not part of this
    project's environment, so this is NOT verified against it (only the distribution matters: no draw-for-draw equality is claimed)."""
    area = h * w
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    u = torch.rand(10, 4, generator=generator).tolist()  # one draw for the ten attempts: (area, log ratio, top, left) each
    for ua, ur, ut, ul in u:
        target = area * (scale[0] + (scale[1] - scale[0]) * ua)
        aspect = math.exp(log_ratio[0] + (log_ratio[1] - log_ratio[0]) * ur)
        cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            top, left = min(int(ut * (h - ch + 1)), h - ch), min(int(ul * (w - cw + 1)), w - cw)
            return left, top, left + cw, top + ch
    in_ratio = w / h
    if in_ratio < ratio[0]:
        cw, ch = w, int(round(w / ratio[0]))
    elif in_ratio > ratio[1]:
        cw, ch = int(round(h * ratio[1])), h
    else:
        cw, ch = w, h
    cw, ch = max(1, min(cw, w)), max(1, min(ch, h))
    left, top = (w - cw) // 2, (h - ch) // 2
    return left, top, left + cw, top + ch


# ---- host tables and matrices ------------------------------------------------------------------------------------------------------
def brightness_table(factor):
    """the reference's own expression (brightness_func)"""
    return (np.arange(256, dtype=np.float32) * factor).clip(0, 255).astype(np.uint8)


def scale255_table():
    """f64 [256]: 255 / d, AutoContrast's scale for hi - lo = d (entry 0 is never read)"""
    t = np.zeros(256, dtype=np.float64)
    t[1:] = 255.0 / np.arange(1, 256, dtype=np.float64)
    return t


def forward_matrix(name, value, W, H):
    """the 2 x 3 matrix the reference hands to cv2.warpAffine -> six Python floats, row by row"""
    f = lambda v: float(np.float32(v))  # (np.float32([[...]]) in shear_*_func and translate_*_func)
    if name == "ShearX":
        return [1.0, f(value), 0.0, 0.0, 1.0, 0.0]
    if name == "ShearY":
        return [1.0, 0.0, 0.0, f(value), 1.0, 0.0]
    if name == "TranslateX":
        return [1.0, 0.0, f(-value), 0.0, 1.0, 0.0]
    if name == "TranslateY":
        return [1.0, 0.0, 0.0, 0.0, 1.0, f(-value)]
    if name == "Rotate":  # cv2.getRotationMatrix2D((W / 2, H / 2), degree, 1)
        cx, cy = W / 2, H / 2
        angle = value * math.pi / 180.0
        alpha, beta = math.cos(angle), math.sin(angle)
        return [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    raise ValueError(f"op {name!r} is not a warp")


def inverse_map(m):
    """the forward matrix -> the six doubles a0 .. a5 of the plan row (source = A (x, y, 1))"""
    m0, m1, m2, m3, m4, m5 = m
    det = m0 * m4 - m1 * m3
    if det == 0.0:
        raise ValueError(f"the matrix {m} has no inverse")
    D = 1.0 / det
    a0, a1, a3, a4 = m4 * D, -m1 * D, -m3 * D, m0 * D
    return [a0, a1, -a0 * m2 - a1 * m5, a3, a4, -a3 * m2 - a4 * m5]


def compile_op(name, args, Sh, Sw, where="op"):
    """one (name, args) of the reference's call list -> ("copy",) | ("table", uint8 [256]) | ("equalize",) | ("autocontrast",) |
    ("warp", [six floats]); ValueError naming `where`, the op and the argument for anything else"""
    args = tuple(args)
    if name not in REFERENCE_AUGS:
        raise ValueError(f"{where}: op {name!r} is not one of the supported {', '.join(REFERENCE_AUGS)}")
    if name in ("Identity", "AutoContrast", "Equalize"):
        if args:
            raise ValueError(f"{where}: {name} takes no arguments, got {args}")
        return {"Identity": ("copy",), "AutoContrast": ("autocontrast",), "Equalize": ("equalize",)}[name]
    if not args or len(args) > 2 or not isinstance(args[0], (int, float, np.integer, np.floating)) or not math.isfinite(args[0]):
        raise ValueError(f"{where}: {name} takes one finite number, got {args}")
    value = float(args[0])
    if name == "Brightness":
        if len(args) != 1:
            raise ValueError(f"{where}: Brightness takes one factor, got {args}")
        table = brightness_table(value)
        return ("copy",) if np.array_equal(table, np.arange(256)) else ("table", table)
    if name == "Sharpness":
        if len(args) != 1 or value != 1.0:
            raise ValueError(f"{where}: Sharpness at factor {value} needs cv2.filter2D, which this project does not have; only factor "
                             "1.0 (the reference's level 5, where it returns its input) is supported")
        return ("copy",)
    if len(args) == 2 and tuple(args[1]) != REPLACE:
        raise ValueError(f"{where}: {name} fills with {REPLACE}, got {args[1]}")
    a = inverse_map(forward_matrix(name, value, Sw, Sh))
    if not all(math.isfinite(v) for v in a):
        raise ValueError(f"{where}: {name}({value}) has no finite inverse map")
    return ("warp", a)


def _check_size(Sh, Sw):
    if Sh < 1 or Sw < 1:
        raise ValueError(f"TrainTransform: size ({Sh}, {Sw}) must be positive")
    if Sh * Sw >= MAX_PIXELS:
        raise ValueError(f"TrainTransform: {Sh} x {Sw} = {Sh * Sw} pixels; Equalize equals the reference's float32 arithmetic only "
                         f"below 2^24 = {MAX_PIXELS} pixels")


def build_plan(ops, Sh, Sw):
    """per image a list of (name, args) -> (int64 [stages, B, FIELDS] rows without addresses, [stages][B] table or None, [stages]
    op masks).  Copies are dropped and the rest moves up, so the stages of a batch are as many as its busiest image has ops that do
    something (at least one: the pass that normalises)."""
    _check_size(Sh, Sw)
    compiled = []
    for i, calls in enumerate(ops):
        row = [compile_op(name, args, Sh, Sw, f"image {i}") for name, args in calls]
        compiled.append([c for c in row if c[0] != "copy"])
    stages = max(1, max(len(c) for c in compiled))
    rows = np.zeros((stages, len(compiled), FIELDS), dtype=np.int64)
    tables = [[None] * len(compiled) for _ in range(stages)]
    masks = [0] * stages
    codes = {"table": OP_TABLE, "equalize": OP_EQUALIZE, "autocontrast": OP_AUTOCONTRAST, "warp": OP_WARP}
    for i, row in enumerate(compiled):
        for s in range(stages):
            c = row[s] if s < len(row) else ("copy",)
            code = codes.get(c[0], OP_COPY)
            rows[s, i, _F_OP] = code
            masks[s] |= 1 << code
            if code == OP_TABLE:
                tables[s][i] = c[1]
            elif code == OP_WARP:
                rows[s, i, _F_A0:_F_A0 + 6] = np.asarray(c[1], dtype=np.float64).view(np.int64)
    return rows, tables, masks


# ---- the transform -----------------------------------------------------------------------------------------------------------------
class TrainTransform:
    """uint8 RGB images -> the normalised f32 [B,3,Sh,Sw] training batch on `device`: one copy and at most 1 + 2 N launches.

    size: S or (Sh, Sw).  What is not given to the call is drawn: boxes by random_resized_crop_box(scale, ratio) and flips with
    probability 1/2 from a torch generator, ops by RandAugmentSampler(N, M, augs) from a numpy RandomState, both seeded with `seed`
    (None: from the system).  last_plan holds the boxes, flips and ops of the last call; handing them back replays it."""

    def __init__(self, size, scale=(0.5, 1.0), N=2, M=5, augs=REFERENCE_AUGS, mean=MEAN, std=STD, device="cuda", seed=None,
                 ratio=(3.0 / 4.0, 4.0 / 3.0)):
        self.pipe = preprocess.ImagePipeline(size, "stretch", mean, std, device)
        self.Sh, self.Sw = self.pipe.Sh, self.pipe.Sw
        _check_size(self.Sh, self.Sw)
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        if not 0.0 < self.scale[0] <= self.scale[1] or not 0.0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError(f"TrainTransform: scale {scale} and ratio {ratio} must be positive and ordered")
        self.sampler = RandAugmentSampler(N, M, augs, np.random.RandomState(seed))
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))
        self.last_plan = None
        self._scale255 = None

    def __call__(self, images, boxes=None, flips=None, ops=None, out=None):
        images = list(images)
        B = len(images)
        if B < 1:
            raise ValueError("TrainTransform: an empty batch")
        arrays = []
        for i, img in enumerate(images):
            host, dev = preprocess._as_uint8_hw3(img, i)
            arrays.append(host if dev is None else dev)
        if boxes is None:
            boxes = [random_resized_crop_box(int(a.shape[1]), int(a.shape[0]), self.scale, self.ratio, self.generator) for a in arrays]
        if flips is None:
            flips = (torch.rand(B, generator=self.generator) < 0.5).tolist()
        if ops is None:
            ops = [self.sampler.sample() for _ in arrays]
        boxes, flips, ops = list(boxes), [bool(f) for f in flips], [[(str(n), tuple(a)) for n, a in calls] for calls in ops]
        if len(ops) != B:
            raise ValueError(f"TrainTransform: {B} images, {len(ops)} op lists")
        rows, tables, masks = build_plan(ops, self.Sh, self.Sw)  # (every op is checked before anything reaches the device)
        batch = self.pipe.prepare(arrays, boxes, flips)
        self.last_plan = {"boxes": boxes, "flips": flips, "ops": ops}
        return self._run(batch, rows, tables, masks, out)

    def _run(self, batch, rows, tables, masks, out):
        out, launches, _ = self.launches(batch, rows, tables, masks, out)
        with torch.cuda.device(out.device):
            for name, _, launch in launches:
                hip._check(launch(torch.cuda.current_stream().cuda_stream), name)
        return out

    def launches(self, batch, rows, tables, masks, out=None):
        """the work of one call after prepare() and build_plan(): the plan's copy to the device, then -> (out, [(entry point,
        stage or -1, launch(stream) -> code)] in order, the buffers they use).  __call__ runs them once; tools time them one by one."""
        B, Sh, Sw = batch.B, self.Sh, self.Sw
        device = batch.packed.device
        if out is None:
            out = torch.empty(B, 3, Sh, Sw, dtype=torch.float32, device=device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, 3, Sh, Sw)):
            raise ValueError(f"out must be a contiguous f32 [{B}, 3, {Sh}, {Sw}] tensor on the device")
        h = lib()
        stages = rows.shape[0]
        with torch.cuda.device(device):
            if self._scale255 is None or self._scale255.device != device:
                self._scale255 = torch.from_numpy(scale255_table()).to(device)
            # the plan rows and the host-made byte tables in one buffer and one copy
            host = np.zeros(rows.nbytes + 256 * sum(t is not None for st in tables for t in st), dtype=np.uint8)
            aux = torch.empty(host.size, dtype=torch.uint8, device=device)
            at = rows.nbytes
            for s in range(stages):
                for i, t in enumerate(tables[s]):
                    if t is not None:
                        host[at:at + 256] = t
                        rows[s, i, _F_TABLE] = aux.data_ptr() + at
                        at += 256
            host[:rows.nbytes] = rows.view(np.uint8).reshape(-1)
            aux.copy_(torch.from_numpy(host))
            planes = [torch.empty(B, 3, Sh, Sw, dtype=torch.uint8, device=device) for _ in range(min(stages, 2))]
            lut_u8 = torch.empty(B, 3, 256, dtype=torch.uint8, device=device)
        p, scale, lut, norm = batch.packed.data_ptr(), self._scale255.data_ptr(), lut_u8.data_ptr(), batch.lut.data_ptr()
        todo = [("madtp_augment_resize_u8", -1, lambda stream, dst=planes[0].data_ptr(): h.madtp_augment_resize_u8(
            p + batch.table_bytes, p, dst, B, Sh, Sw, batch.n_blocks, batch.max_ksize, stream))]
        stats_mask = 1 << OP_EQUALIZE | 1 << OP_AUTOCONTRAST
        for s in range(stages):
            last = s == stages - 1
            cur, plan, mask = planes[s % 2].data_ptr(), aux.data_ptr() + s * B * FIELDS * 8, masks[s]
            dst = out.data_ptr() if last else planes[(s + 1) % 2].data_ptr()
            if mask & stats_mask:  # (the entry point would return without a launch)
                todo.append(("madtp_augment_stats", s, lambda stream, cur=cur, plan=plan, mask=mask: h.madtp_augment_stats(
                    cur, plan, scale, lut, B, Sh, Sw, mask, stream)))
            todo.append(("madtp_augment_apply", s, lambda stream, cur=cur, plan=plan, mask=mask, dst=dst, last=last: h.madtp_augment_apply(
                cur, plan, lut, norm if last else None, dst, B, Sh, Sw, mask, stream)))
        return out, todo, (batch, aux, planes, lut_u8)

    def resize_u8(self, images, boxes=None, flips=None):
        """the byte stage alone: uint8 [B,3,Sh,Sw] on the device (what the augmentation stages start from)"""
        batch = self.pipe.prepare(images, boxes, flips)
        out = torch.empty(batch.B, 3, self.Sh, self.Sw, dtype=torch.uint8, device=batch.packed.device)
        with torch.cuda.device(out.device):
            p = batch.packed.data_ptr()
            hip._check(lib().madtp_augment_resize_u8(p + batch.table_bytes, p, out.data_ptr(), batch.B, self.Sh, self.Sw, batch.n_blocks,
                                                     batch.max_ksize, torch.cuda.current_stream().cuda_stream), "madtp_augment_resize_u8")
        return out


# ---- the data loader's side --------------------------------------------------------------------------------------------------------
_transforms = {}


class RawTrainBatch:
    """The images of a training batch as the dataset decoded them.  to(device) runs TrainTransform (one per device and setting,
    drawing from the system's entropy) and returns the f32 [B,3,S,S] tensor: `image = image.to(device, non_blocking=True)`."""

    def __init__(self, images, size, scale=(0.5, 1.0), N=2, M=5, augs=REFERENCE_AUGS, mean=MEAN, std=STD):
        self.images, self.size, self.scale, self.N, self.M = list(images), size, tuple(scale), N, M
        self.augs, self.mean, self.std = tuple(augs), tuple(mean), tuple(std)

    def __len__(self):
        return len(self.images)

    def to(self, device, non_blocking=False, **_):
        device = torch.device(device)
        key = (str(device), self.size if isinstance(self.size, int) else tuple(self.size), self.scale, self.N, self.M, self.augs,
               self.mean, self.std)
        if key not in _transforms:
            _transforms[key] = TrainTransform(self.size, self.scale, self.N, self.M, self.augs, self.mean, self.std, device)
        return _transforms[key](self.images)

    def cuda(self, device=None, non_blocking=False):
        return self.to("cuda" if device is None else device)


def collate(samples, size, scale=(0.5, 1.0), N=2, M=5, augs=REFERENCE_AUGS, mean=MEAN, std=STD):
    """collate_fn of a training loader (bind `size` with functools.partial): preprocess.collate with RawTrainBatch for the images"""
    return preprocess.collate_with(samples, preprocess._is_raw, lambda col: RawTrainBatch(col, size, scale, N, M, augs, mean, std))
