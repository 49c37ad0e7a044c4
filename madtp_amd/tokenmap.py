"""Token maps (csrc/madtp_tokenmap.h, csrc/tokenmap.hip): which patches and words of a sample are still there after layer l, and
what every surviving slot stands for - composed on the device from the `last_prune` records a forward leaves on its layers.

    tm = tokenmap.from_vit(model.visual_encoder)         # right after a forward; from_text(bert_encoder), from_clip(tower) likewise
    tm.kept(l)                                           # bool [B, n0]: the patches that still own a token after layer l
    y = tm.push(x, l)                                    # f32 [B, n0, C] per-patch quantity -> [B, n_out[l], C], pruned as the forward did
    grid = tm.pull(v, l)                                 # f32 [B, n_out[l], C] per-token quantity -> [B, n0, C], back on the patch grid
    agreement(tm_a, tm_b).jaccard                        # [B, L]: the kept sets of two runs compared in original coordinates
    figure = shade(images_u8, tm, (gh, gw))              # uint8 [B, H, W, 3]: every patch dimmed by the layer it was pruned at

A pruned layer keeps k tokens and merges the rest into one, so after every layer the original positions form a partition over the
slots: slot[b, l, p] (row slot + 1 of the layer's output; row 0, CLS / [ENC], is not part of the map), coef[b, l, p] (the product of
the merge weights p has passed through, exactly 1.0 while p owns its slot) and depth[b, p] (the number of leading layers after which p
still owned a slot alone) describe the whole run.  Device tensors only: a CPU tensor raises, there is no fallback (the *_host
functions run the kernels' lane routines on the host for checking without a GPU)."""
import collections
import os

import numpy as np
import torch

from . import abi, hip, staging

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "madtp_tokenmap.h")
# the one declaration of the madtp_tokenmap_* entry points, next to the sources (abi.bind takes an absolute path as it is); lib() is
# hip.load()'s handle with them set on it (no GPU needed)
SIGNATURES, DEFINES, lib = abi.bind(HEADER, "madtp_tokenmap_abi_version", prefix="madtp_tokenmap_")
ABI_VERSION = DEFINES["MADTP_TOKENMAP_ABI_VERSION"]
MAX_N, MAX_LAYERS, MAX_BATCH, MAX_C = (DEFINES["MADTP_TOKENMAP_" + k] for k in ("MAX_N", "MAX_LAYERS", "MAX_BATCH", "MAX_C"))
FIELDS, LAYER_BITS = DEFINES["MADTP_TOKENMAP_FIELDS"], DEFINES["MADTP_TOKENMAP_STATUS_LAYER_BITS"]
_F = {k[len("MADTP_TOKENMAP_F_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_TOKENMAP_F_")}
E = {k[len("MADTP_TOKENMAP_E_"):]: v for k, v in DEFINES.items() if k.startswith("MADTP_TOKENMAP_E_")}


def status_fields(word):
    """a status word -> (code, layer); (0, None) for 0"""
    word = int(word)
    if word == 0:
        return 0, None
    return -((-word) >> LAYER_BITS), (-word) & ((1 << LAYER_BITS) - 1)


def _raise_status(status):
    """ValueError naming the first sample whose records break a rule, and the layer"""
    for b, word in enumerate(status):
        code, layer = status_fields(word)
        if code:
            raise ValueError(f"sample {b}, layer {layer}: {lib().madtp_tokenmap_strerror(code).decode()} (code {code})")


def _sizes(n0, L, B):
    if not 1 <= int(n0) <= MAX_N:
        raise ValueError(f"n0 = {n0} outside [1, {MAX_N}]")
    if not 1 <= L <= MAX_LAYERS:
        raise ValueError(f"records: {L} layers, outside [1, {MAX_LAYERS}]")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"records: a batch of {B}, outside [1, {MAX_BATCH}]")


def _pruned(rec):
    return rec is not None and bool(rec.get("pruned"))


_DTYPES = (("indices", "int64"), ("indices_sort", "int64"), ("score", "float32"))


def _table(records, n0, ptr, is_ok):
    """The checks of the records that need no device and the MADTP_TOKENMAP_F_* rows -> (int64 [L, FIELDS] numpy, B, n_out, pruned).
    ptr(t) -> address, is_ok(t, dtype name) -> None or what is wrong with the tensor.  The widths are checked against the chain of
    lengths as far as the ks fit; a k that does not fit is the kernel's to name (the layers behind it are never read)."""
    records = list(records)
    L = len(records)
    B = None
    for l, rec in enumerate(records):
        if _pruned(rec):
            for name, dt in _DTYPES:
                t = rec.get(name)
                if t is None:
                    raise ValueError(f"records[{l}]: a pruned layer without '{name}'")
                bad = is_ok(t, dt)
                if bad:
                    raise ValueError(f"records[{l}]['{name}']: {bad}")
                if B is None:
                    B = int(t.shape[0])
                if int(t.shape[0]) != B:
                    raise ValueError(f"records[{l}]['{name}']: {t.shape[0]} samples, the layers before have {B}")
        elif rec is not None and rec.get("score") is not None and is_ok(rec["score"], "float32") is None:
            B = int(rec["score"].shape[0]) if B is None else B  # (a run in which no layer pruned still says how many samples it had)
    _sizes(n0, L, 1 if B is None else B)
    table = np.zeros((L, FIELDS), dtype=np.int64)
    n, chain, n_out, pruned = int(n0), True, [], []
    for l, rec in enumerate(records):
        table[l, _F["N_IN"]] = n
        if not _pruned(rec):
            table[l, _F["K"]] = -1
            n_out.append(n)
            pruned.append(False)
            continue
        k = int(rec["k"])
        if k == -1:
            raise ValueError(f"records[{l}]['k']: -1 stands for a layer that did not prune")
        table[l, _F["K"]] = k
        fits = chain and 1 <= k < n
        for name, dt in _DTYPES:
            t = rec[name]
            need = k if name == "indices" else n
            if fits and t.shape[1] < need:
                raise ValueError(f"records[{l}]['{name}']: {t.shape[1]} columns, the layer reads {need}")
            key = {"indices": "INDICES", "indices_sort": "SORT", "score": "SCORE"}[name]
            table[l, _F[key]] = ptr(t)
            table[l, _F[key + "_STRIDE"]] = t.shape[1] if B == 1 else _stride0(t)
        chain = fits
        n = k + 1 if fits else n
        n_out.append(n)
        pruned.append(True)
    return table, (1 if B is None else B), n_out, pruned


def _stride0(t):
    return int(t.stride(0)) if torch.is_tensor(t) else int(t.strides[0] // t.itemsize)


def _gpu_ok(t, dt):
    if not torch.is_tensor(t):
        return f"a {type(t).__name__}, not a tensor"
    if not t.is_cuda:
        return "a CPU tensor: the kernels take device tensors only (no CPU fallback)"
    if t.dtype != getattr(torch, dt) or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        return f"must be a {dt} [B, n] tensor with unit stride in a row, not {t.dtype} {tuple(t.shape)} strides {tuple(t.stride())}"
    return None


_Waiter = staging.StatusWaiter  # (the wait for a launch's status words, shared with text.py)


_waiter = _Waiter()


def _build(records, n0, fill=None):
    """The launch without the wait: -> (slot, coef, depth, status, n_out, pruned).  A sample whose status word is not 0 is left
    unwritten: at `fill` where one is given, else at whatever torch.empty held."""
    records = list(records)
    table, B, n_out, pruned = _table(records, n0, lambda t: t.data_ptr(), _gpu_ok)
    devs = {rec[name].device for rec in records if _pruned(rec) for name, _ in _DTYPES}
    devs |= {rec["score"].device for rec in records if rec is not None and torch.is_tensor(rec.get("score")) and rec["score"].is_cuda}
    if len(devs) > 1:
        raise ValueError(f"records: tensors on {sorted(map(str, devs))}")
    if not devs:
        raise ValueError("records: no layer has a device tensor, so nothing says which device or batch the map is for")
    dev, L = devs.pop(), len(table)
    with torch.cuda.device(dev):
        staging = torch.from_numpy(table).pin_memory()  # a NEW pinned buffer per upload (hip.AdamWTable): never rewritten in flight
        dtable = staging.to(dev, non_blocking=True)
        make = torch.empty if fill is None else (lambda *shape, **kw: torch.full(shape, fill, **kw))
        slot = make(B, L, n0, dtype=torch.int32, device=dev)
        coef = make(B, L, n0, dtype=torch.float32, device=dev)
        depth = make(B, n0, dtype=torch.int32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        hip._check(lib().madtp_tokenmap_build(dtable.data_ptr(), L, B, int(n0), slot.data_ptr(), coef.data_ptr(), depth.data_ptr(),
                                              status.data_ptr(), hip._stream()), "madtp_tokenmap_build")
    return slot, coef, depth, status, n_out, pruned


class TokenMap:
    """slot int32 [B, L, n0], coef f32 [B, L, n0], depth int32 [B, n0] on the device; n_out[l]: slots of layer l's output (without
    row 0); pruned[l]: whether layer l pruned."""

    def __init__(self, slot, coef, depth, n_out, pruned):
        self.slot, self.coef, self.depth, self.n_out, self.pruned = slot, coef, depth, list(n_out), list(pruned)
        self.B, self.L, self.n0 = slot.shape

    def _layer(self, l):
        if not isinstance(l, int) or not 0 <= l < self.L:
            raise ValueError(f"l = {l!r} is not a layer in [0, {self.L})")
        return l

    def kept(self, l):
        """bool [B, n0]: the positions that still own a slot alone after layer l"""
        return self.depth > self._layer(l)

    def _values(self, t, name, rows):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor, not {getattr(t, 'dtype', type(t).__name__)}")
        if t.dim() not in (2, 3) or t.shape[0] != self.B or t.shape[1] != rows:
            raise ValueError(f"{name} {tuple(t.shape)} must be [{self.B}, {rows}] or [{self.B}, {rows}, C]")
        flat = t.dim() == 2
        t = t.unsqueeze(2) if flat else t
        if not 1 <= t.shape[2] <= MAX_C:
            raise ValueError(f"{name}: C = {t.shape[2]} outside [1, {MAX_C}]")
        if not t.is_cuda:
            raise ValueError(f"{name} is a CPU tensor: the kernels take device tensors only (no CPU fallback)")
        if t.device != self.slot.device:
            raise ValueError(f"{name} is on {t.device}, the map on {self.slot.device}")
        return t, flat

    def push(self, x, l):
        """x f32 [B, n0, C] (or [B, n0]) -> f32 [B, n_out[l], C]: y[b, s] = sum of coef[p] x[b, p] over the positions of slot s in
        ascending p - the pruning of layers 0 .. l replayed on x.  x is read in place when its channels have unit stride."""
        l = self._layer(l)
        x, flat = self._values(x, "x", self.n0)
        if x.shape[2] > 1 and x.stride(2) != 1 or min(x.stride(0), x.stride(1)) < 0 or x.stride(1) < x.shape[2] or \
                (self.B > 1 and x.stride(0) < (self.n0 - 1) * x.stride(1) + x.shape[2]):
            x = x.contiguous()
        C, n_out = x.shape[2], self.n_out[l]
        y = torch.empty(self.B, n_out, C, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            hip._check(lib().madtp_tokenmap_push(x.data_ptr(), x.stride(0), x.stride(1), self.slot[:, l].data_ptr(), self.coef[:, l].data_ptr(),
                                                 self.L * self.n0, y.data_ptr(), self.B, self.n0, n_out, C, hip._stream()),
                       "madtp_tokenmap_push")
        return y.squeeze(2) if flat else y

    def pull(self, v, l, weighted=False):
        """v f32 [B, n_out[l], C] (or [B, n_out[l]]) -> f32 [B, n0, C]: out[b, p] = v[b, slot[b, l, p]], times coef[b, l, p] when
        weighted (the share of p in its slot) - a quantity of layer l's tokens back in the input's coordinates."""
        l = self._layer(l)
        v, flat = self._values(v, "v", self.n_out[l])
        v = v.contiguous()
        C = v.shape[2]
        out = torch.empty(self.B, self.n0, C, dtype=torch.float32, device=v.device)
        with torch.cuda.device(v.device):
            hip._check(lib().madtp_tokenmap_pull(v.data_ptr(), self.slot[:, l].data_ptr(), self.coef[:, l].data_ptr(), self.L * self.n0,
                                                 out.data_ptr(), self.B, self.n0, self.n_out[l], C, int(bool(weighted)), hip._stream()),
                       "madtp_tokenmap_pull")
        return out.squeeze(2) if flat else out


def from_records(records, n0):
    """`last_prune` records of the L layers of one encoder run (None or pruned == False: the layer did not prune), n0 prunable
    positions -> TokenMap.  Read them right after the forward: the records of an encoder-level call are VIEWS of that call's one
    buffer, which the next forward of the model reuses.  The call waits for the kernel's status words only (on a side stream, behind
    an event).  A record whose indices leave [0, n_in), repeat, or whose k does not fit raises ValueError naming the sample and the
    layer; there is never a partial map."""
    slot, coef, depth, status, n_out, pruned = _build(records, n0)
    _raise_status(_waiter.read(status))
    return TokenMap(slot, coef, depth, n_out, pruned)


def _layer_records(layers, what):
    records = [getattr(m, "last_prune", None) for m in layers]
    if not records:
        raise ValueError(f"{what}: no layers")
    return records


def _n0(records, what):
    for rec in records:
        if rec is not None and rec.get("score") is not None:
            return int(rec["score"].shape[1])  # the first scored layer sees every position
    raise ValueError(f"{what}: no layer has a prune record - run a forward with a temperature first")


def from_vit(visual_encoder):
    """vit.VisionTransformer right after a forward -> TokenMap over its patches (see from_records on the records' lifetime)"""
    records = _layer_records(visual_encoder.blocks, "from_vit")
    n0 = getattr(getattr(visual_encoder, "patch_embed", None), "num_patches", None)
    return from_records(records, _n0(records, "from_vit") if n0 is None else int(n0))


def from_text(bert_encoder):
    """a BERT encoder (bert.BertModel, or its .encoder) right after a forward -> TokenMap over the text tokens behind [CLS] / [ENC]"""
    enc = getattr(bert_encoder, "encoder", bert_encoder)
    records = _layer_records(enc.layer, "from_text")
    return from_records(records, _n0(records, "from_text"))


def from_clip(tower):
    """a CLIP tower (clip_model.VisionTransformer or a Transformer with .resblocks) right after a forward -> TokenMap"""
    blocks = getattr(getattr(tower, "transformer", tower), "resblocks")
    records = _layer_records(blocks, "from_clip")
    return from_records(records, _n0(records, "from_clip"))


class Agreement(collections.namedtuple("Agreement", "intersection union")):
    """int32 [B, L] tensors: per sample and layer the size of the intersection and of the union of two runs' kept sets"""
    __slots__ = ()

    @property
    def exact(self):
        """bool [B, L]: the two kept sets are equal"""
        return self.intersection == self.union

    @property
    def jaccard(self):
        """f32 [B, L]: |A & B| / |A | B|, 1.0 where both sets are empty"""
        u = self.union.to(torch.float32)
        return torch.where(self.union > 0, self.intersection.to(torch.float32) / u.clamp(min=1.0), torch.ones_like(u))


def agreement(a, b):
    """two TokenMaps of the same inputs (two precision modes, two models, two temperatures) -> Agreement (madtp_tokenmap_agree)"""
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, TokenMap):
            raise ValueError(f"{name} must be a TokenMap, not {type(t).__name__}")
    if (a.B, a.L, a.n0) != (b.B, b.L, b.n0) or a.depth.device != b.depth.device:
        raise ValueError(f"a is a map of [B, L, n0] = {(a.B, a.L, a.n0)} on {a.depth.device}, b of {(b.B, b.L, b.n0)} on {b.depth.device}")
    out = torch.empty(a.B, a.L, 2, dtype=torch.int32, device=a.depth.device)
    with torch.cuda.device(out.device):
        hip._check(lib().madtp_tokenmap_agree(a.depth.data_ptr(), b.depth.data_ptr(), out.data_ptr(), a.B, a.n0, a.L, hip._stream()),
                   "madtp_tokenmap_agree")
    return Agreement(out[..., 0], out[..., 1])


def default_levels(L):
    """uint8 [L + 1]: a patch pruned by the first layer at a quarter of its brightness, one that survives every layer untouched"""
    return [int(round(255 * (0.25 + 0.75 * d / L))) for d in range(L + 1)]


def shade(images, tm, grid, levels=None):
    """images uint8 [B, H, W, 3] on the device, grid = (gh, gw) with gh gw == tm.n0 -> uint8 [B, H, W, 3]: every pixel times
    levels[depth of its patch] / 255, rounded (madtp_tokenmap_shade) - the figure of the kept patches per layer."""
    if not isinstance(tm, TokenMap):
        raise ValueError(f"tm must be a TokenMap, not {type(tm).__name__}")
    if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("images must be a uint8 [B, H, W, 3] tensor")
    if not images.is_cuda:
        raise ValueError("images is a CPU tensor: the kernels take device tensors only (no CPU fallback)")
    gh, gw = (int(g) for g in grid)
    B, H, W, _ = images.shape
    if B != tm.B or images.device != tm.depth.device:
        raise ValueError(f"images: {B} on {images.device}, the map has {tm.B} samples on {tm.depth.device}")
    if gh < 1 or gw < 1 or gh * gw != tm.n0 or H % gh or W % gw:
        raise ValueError(f"grid = {(gh, gw)} does not divide {H} x {W} into the map's {tm.n0} patches")
    if (H * W * 3) % 16:
        raise ValueError(f"images: {H} x {W} x 3 bytes per image is not a multiple of 16")
    levels = default_levels(tm.L) if levels is None else [int(v) for v in (levels.tolist() if torch.is_tensor(levels) else levels)]
    if len(levels) != tm.L + 1 or not all(0 <= v <= 255 for v in levels):
        raise ValueError(f"levels must be {tm.L + 1} values in [0, 255]")
    images = images.contiguous()
    with torch.cuda.device(images.device):
        table = torch.tensor(levels, dtype=torch.uint8).pin_memory().to(images.device, non_blocking=True)
        out = torch.empty_like(images)
        hip._check(lib().madtp_tokenmap_shade(images.data_ptr(), tm.depth.data_ptr(), table.data_ptr(), out.data_ptr(), B, gh, gw, H // gh,
                                              W // gw, tm.L, hip._stream()), "madtp_tokenmap_shade")
    return out


# ---- the host emulation: the kernels' lane routines with the lanes in a loop, numpy in and out (no GPU) -------------------------------
def _np_ok(t, dt):
    if not isinstance(t, np.ndarray) or t.dtype != np.dtype(dt) or t.ndim != 2 or (t.shape[1] > 1 and t.strides[1] != t.itemsize):
        return f"must be a numpy {dt} [B, n] array with unit stride in a row"
    return None


def build_host(records, n0, fill=None):
    """records of numpy arrays -> (slot, coef, depth, status) numpy arrays of madtp_tokenmap_build_host; `fill`: the value the
    outputs are made of before the call (a sample with a status word is left at it)"""
    table, B, n_out, pruned = _table(records, n0, lambda t: t.ctypes.data, _np_ok)
    L = len(table)
    slot = np.full((B, L, n0), -7 if fill is None else fill, dtype=np.int32)
    coef = np.full((B, L, n0), -7 if fill is None else fill, dtype=np.float32)
    depth = np.full((B, n0), -7 if fill is None else fill, dtype=np.int32)
    status = np.full(B, 1, dtype=np.int32)
    hip._check(lib().madtp_tokenmap_build_host(table.ctypes.data, L, B, int(n0), slot.ctypes.data, coef.ctypes.data, depth.ctypes.data,
                                               status.ctypes.data), "madtp_tokenmap_build_host")
    return slot, coef, depth, status


def push_host(x, slot, coef, n_out):
    """x f32 [B, n0, C], one layer's slot / coef [B, n0] -> y f32 [B, n_out, C] (madtp_tokenmap_push_host)"""
    x, slot, coef = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(slot, np.int32), np.ascontiguousarray(coef, np.float32)
    B, n0, C = x.shape
    y = np.zeros((B, n_out, C), dtype=np.float32)
    hip._check(lib().madtp_tokenmap_push_host(x.ctypes.data, n0 * C, C, slot.ctypes.data, coef.ctypes.data, n0, y.ctypes.data, B, n0,
                                              int(n_out), C), "madtp_tokenmap_push_host")
    return y


def pull_host(v, slot, coef, weighted=False):
    """v f32 [B, n_l, C], one layer's slot / coef [B, n0] -> out f32 [B, n0, C] (madtp_tokenmap_pull_host)"""
    v, slot, coef = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(slot, np.int32), np.ascontiguousarray(coef, np.float32)
    B, n_l, C = v.shape
    n0 = slot.shape[1]
    out = np.zeros((B, n0, C), dtype=np.float32)
    hip._check(lib().madtp_tokenmap_pull_host(v.ctypes.data, slot.ctypes.data, coef.ctypes.data, n0, out.ctypes.data, B, n0, n_l, C,
                                              int(bool(weighted))), "madtp_tokenmap_pull_host")
    return out


def agree_host(depth_a, depth_b, L):
    """two depth arrays int32 [B, n0] -> int32 [B, L, 2] (madtp_tokenmap_agree_host)"""
    a, b = np.ascontiguousarray(depth_a, np.int32), np.ascontiguousarray(depth_b, np.int32)
    B, n0 = a.shape
    out = np.zeros((B, L, 2), dtype=np.int32)
    hip._check(lib().madtp_tokenmap_agree_host(a.ctypes.data, b.ctypes.data, out.ctypes.data, B, n0, int(L)), "madtp_tokenmap_agree_host")
    return out


def _aligned_u8(shape):
    raw = np.zeros(int(np.prod(shape)) + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + int(np.prod(shape))].reshape(shape)


def shade_host(images, depth, grid, levels):
    """images uint8 [B, H, W, 3], depth int32 [B, gh gw], levels (L + 1 values) -> uint8 [B, H, W, 3] (madtp_tokenmap_shade_host)"""
    B, H, W, _ = images.shape
    gh, gw = grid
    src, out = _aligned_u8(images.shape), _aligned_u8(images.shape)
    src[...] = images
    depth, level = np.ascontiguousarray(depth, np.int32), np.asarray(levels, dtype=np.uint8)
    hip._check(lib().madtp_tokenmap_shade_host(src.ctypes.data, depth.ctypes.data, level.ctypes.data, out.ctypes.data, B, gh, gw, H // gh,
                                               W // gw, len(level) - 1), "madtp_tokenmap_shade_host")
    return out.copy()
