"""Pillow's bicubic resize (Resample.c) restated with Python floats and numpy integers, independent of madtp_amd/preprocess.py:
the reference the image-pipeline tests compare with, byte for byte.  Coefficients: IEEE double, one operation at a time, in
Pillow's order; passes: horizontal first, rounded to uint8, then vertical on those bytes, int32 accumulation from 2^21 and an
arithmetic shift by 22."""
import math

import numpy as np
import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coefficients(in_size, out_size, box=None):
    """-> (ksize, [xmin], [n], [[int coefficient] * n]) of one axis"""
    in0, in1 = (0.0, float(in_size)) if box is None else (float(box[0]), float(box[1]))
    scale = fs = (in1 - in0) / out_size
    if fs < 1.0:
        fs = 1.0
    support = 2.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmins, ns, ks = [], [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        n = xmax - xmin
        w, ww = [], 0.0
        for i in range(n):
            v = bicubic((i + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        ks.append([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w])
        xmins.append(xmin)
        ns.append(n)
    return ksize, xmins, ns, ks


def resample_axis(img, axis, out_size, box=None):
    """one pass over `axis` (0 = vertical, 1 = horizontal) of a uint8 [h, w, c] array"""
    _, xmins, ns, ks = coefficients(img.shape[axis], out_size, box)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        k = np.asarray(ks[xx], dtype=np.int32).reshape((-1,) + (1,) * (src.ndim - 1))
        acc = (1 << 21) + (src[xmins[xx]:xmins[xx] + ns[xx]] * k).sum(axis=0, dtype=np.int32)
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h):
    """PIL.Image.resize((out_w, out_h), BICUBIC) of a uint8 [h, w, 3] array"""
    return resample_axis(resample_axis(np.ascontiguousarray(img), 1, out_w), 0, out_h)


def short_side_crop(img, size):
    """torchvision's Resize(size) + CenterCrop(size) on PIL images, restated (see preprocess.short_side_geometry)"""
    h, w = img.shape[:2]
    nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
    left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
    return resize(img, nw, nh)[top:top + size, left:left + size]


def to_tensor_normalize(img, mean=MEAN, std=STD):
    """ToTensor + Normalize of a uint8 [h, w, 3] array with torch CPU operations -> f32 [3, h, w]"""
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return t.sub(m[:, None, None]).div(s[:, None, None])


def random_image(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def checkerboard(h, w):
    """0 / 255 squares of one pixel: the input that drives the bicubic overshoot into both clamps"""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
