"""The ten RandAugment ops of the reference's training loaders (transform/randaugment.py) restated in numpy on uint8 [h, w, 3]
arrays, independent of madtp_amd/augment.py: the reference the augmentation tests compare with, byte for byte.  No torch-GPU,
Pillow or OpenCV.  The byte ops are checked against the reference's own functions through tests/golden/augment_ref.npz; the three
warps follow the project's fixed-point definition (include/madtp_augment.h), in Python / numpy integers."""
import math

import numpy as np

FILL = 128
AUGS = ["Identity", "AutoContrast", "Brightness", "Sharpness", "Equalize", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"]


def brightness_table(factor):
    return (np.arange(256, dtype=np.float32) * factor).clip(0, 255).astype(np.uint8)


def equalize_table(ch):
    """integers throughout (the reference's float32 holds them exactly while the channel has fewer than 2^24 pixels)"""
    hist = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    last = int(np.nonzero(hist)[0][-1])
    step = (int(ch.size) - int(hist[last])) // 255
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    below = np.concatenate([[0], np.cumsum(hist)[:-1]])
    return np.minimum(255, (step // 2 + below) // step).astype(np.uint8)


def autocontrast_table(ch):
    lo, hi = int(ch.min()), int(ch.max())
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = float((256 - lo) % 256) * scale  # the reference negates a numpy uint8
    table = [min(max(i * scale + offset, 0.0), 255.0) for i in range(256)]  # Python floats: IEEE double, one operation at a time
    return np.asarray([int(t) for t in table], dtype=np.uint8)


def per_channel(img, make_table):
    return np.stack([make_table(img[:, :, c])[img[:, :, c]] for c in range(3)], axis=2)


def forward_matrix(name, value, W, H):
    f = lambda v: float(np.float32(v))
    if name == "ShearX":
        return [1.0, f(value), 0.0, 0.0, 1.0, 0.0]
    if name == "ShearY":
        return [1.0, 0.0, 0.0, f(value), 1.0, 0.0]
    if name == "TranslateX":
        return [1.0, 0.0, f(-value), 0.0, 1.0, 0.0]
    if name == "TranslateY":
        return [1.0, 0.0, 0.0, 0.0, 1.0, f(-value)]
    assert name == "Rotate", name
    cx, cy = W / 2, H / 2
    alpha, beta = math.cos(value * math.pi / 180.0), math.sin(value * math.pi / 180.0)
    return [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]


def inverse_map(m):
    D = 1.0 / (m[0] * m[4] - m[1] * m[3])
    a0, a1, a3, a4 = m[4] * D, -m[1] * D, -m[3] * D, m[0] * D
    return [a0, a1, -a0 * m[2] - a1 * m[5], a3, a4, -a3 * m[2] - a4 * m[5]]


def warp_coords(a, W, H):
    """-> int64 [H, W] X and Y in 1/32 pixel: (rint((a1 y + a2) 1024) + 16 + rint(a0 x 1024)) >> 5 (numpy rounds every operation to
    double and np.rint rounds half to even)"""
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    out = []
    for ax, ay, ac in (a[0:3], a[3:6]):
        t = np.rint((ay * y + ac) * 1024.0).astype(np.int64)
        u = np.rint((ax * x) * 1024.0).astype(np.int64)
        out.append((t + 16 + u) >> 5)
    return out


def warp(img, a):
    """the fixed-point bilinear warp of madtp_augment.h with the inverse map a0 .. a5; a tap outside the image is FILL"""
    H, W = img.shape[:2]
    X, Y = warp_coords(a, W, H)
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    src = img.astype(np.int64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        return np.where(inside[:, :, None], v, FILL)

    w00, w01, w10, w11 = 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy
    assert ((w00 + w01 + w10 + w11) == 32768).all()
    acc = (w00[:, :, None] * tap(sy, sx) + w01[:, :, None] * tap(sy, sx + 1) + w10[:, :, None] * tap(sy + 1, sx)
           + w11[:, :, None] * tap(sy + 1, sx + 1) + 16384)
    return (acc >> 15).astype(np.uint8)


def apply(img, name, args=()):
    """one call of the reference's func_dict[name](img, *args)"""
    if name == "Identity":
        return img
    if name == "AutoContrast":
        return per_channel(img, autocontrast_table)
    if name == "Equalize":
        return per_channel(img, equalize_table)
    if name == "Brightness":
        return brightness_table(args[0])[img]
    if name == "Sharpness":
        if args[0] != 1.0:
            raise ValueError(f"Sharpness({args[0]}) needs cv2.filter2D")
        return img
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        assert len(args) == 1 or tuple(args[1]) == (FILL, FILL, FILL)
        return warp(img, inverse_map(forward_matrix(name, args[0], img.shape[1], img.shape[0])))
    raise ValueError(f"unknown op {name!r}")


def apply_all(img, calls):
    for name, args in calls:
        img = apply(img, name, args)
    return img


def sample(rng, N=2, M=5, augs=AUGS):
    """the (name, args) calls of one RandomAugment(N, M, augs)(img), drawn from the numpy RandomState `rng` in the reference's order"""
    calls = []
    for name in rng.choice(augs, N):
        if rng.random_sample() > 0.5:
            continue
        name = str(name)
        if name in ("Identity", "AutoContrast", "Equalize"):
            args = ()
        elif name in ("Brightness", "Sharpness"):
            args = ((M / 10) * 1.8 + 0.1,)
        elif name == "Rotate":
            level = (M / 10) * 30
            args = (-level if rng.random_sample() < 0.5 else level, (FILL, FILL, FILL))
        else:
            level = (M / 10) * (0.3 if name.startswith("Shear") else float(10))
            args = (-level if rng.random_sample() > 0.5 else level, (FILL, FILL, FILL))
        calls.append((name, args))
    return calls
