"""Records what Pillow itself returns for small seeded uint8 images in tests/golden/imgprep_pil.npz (CPU only, needs Pillow):

    python tools/make_image_golden.py

The file holds data only - the inputs, Pillow's outputs and Pillow's version - so that the image-pipeline tests have Pillow's
bits on a machine without Pillow.  Keys:
    in_<name>                              uint8 [h, w, 3] input
    resize_<name>_<W>x<H>                  Image.resize((W, H), BICUBIC)
    crop_<name>_<l>_<u>_<r>_<d>_<W>x<H>    Image.crop(box).resize((W, H), BICUBIC)
    ssc_<name>_<S>                         resize of the short side to S (long side int(S * long / short)), then the centre crop
    flip_<name>_<W>x<H>                    the resize, then transpose(FLIP_LEFT_RIGHT)
    sweep_in_<n>, sweep_<n>_<m>            uint8 [2, n, 3] and its resize to (m, 2): one axis from n to m pixels
    pillow_version"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "imgprep_pil.npz")

# (name, width, height); "checker" is the 0 / 255 board, the rest is seeded noise
SOURCES = [("p1x1", 1, 1), ("p1x7", 1, 7), ("p7x1", 7, 1), ("p33x41", 33, 41), ("checker97x131", 97, 131), ("p100x75", 100, 75),
           ("p300x50", 300, 50), ("p384x36", 384, 36)]
SIZES = [(32, 32), (40, 40), (96, 40)]
CROPS = {"p33x41": (0, 0, 20, 41), "checker97x131": (5, 7, 90, 100), "p100x75": (30, 10, 100, 75), "p300x50": (100, 0, 160, 50)}
SHORT_SIDE = {"p33x41": (32, 40), "checker97x131": (32, 40), "p100x75": (32, 40), "p300x50": (32,), "p7x1": (32,)}
# one axis, in -> out: ratios below 1, equal to 1, in (1, 2) and above 2, non-integer ratios, in == 1
SWEEP = [(1, 1), (1, 5), (1, 32), (2, 1), (2, 7), (3, 3), (3, 10), (5, 2), (7, 7), (7, 8), (7, 13), (8, 7), (9, 4), (10, 3), (11, 32),
         (13, 40), (16, 16), (16, 32), (17, 5), (19, 96), (23, 7), (31, 32), (32, 31), (33, 32), (37, 11), (40, 32), (41, 40), (47, 32),
         (50, 33), (63, 32), (64, 32), (65, 32), (70, 9), (81, 40), (96, 32), (97, 40), (100, 7), (127, 96), (128, 5), (131, 40),
         (150, 32), (190, 96), (200, 13), (250, 40), (257, 17), (300, 96)]


def source(name, w, h, seed):
    if name.startswith("checker"):
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def main():
    data = {"pillow_version": np.array(PIL.__version__)}
    for seed, (name, w, h) in enumerate(SOURCES):
        arr = source(name, w, h, 1000 + seed)
        img = Image.fromarray(arr, "RGB")
        data[f"in_{name}"] = arr
        for W, H in SIZES if name in CROPS else SIZES[:2]:  # (the fixture stays under 300 KB: the wide size for four sources)
            data[f"resize_{name}_{W}x{H}"] = np.asarray(img.resize((W, H), Image.BICUBIC))
        if name in CROPS:
            W, H = SIZES[0]
            data[f"flip_{name}_{W}x{H}"] = np.asarray(img.resize((W, H), Image.BICUBIC).transpose(Image.FLIP_LEFT_RIGHT))
            box = CROPS[name]
            for W, H in SIZES[:2]:
                data["crop_%s_%d_%d_%d_%d_%dx%d" % ((name,) + box + (W, H))] = np.asarray(img.crop(box).resize((W, H), Image.BICUBIC))
        for S in SHORT_SIDE.get(name, ()):
            nw, nh = (S, int(S * h / w)) if w <= h else (int(S * w / h), S)
            left, top = int(round((nw - S) / 2.0)), int(round((nh - S) / 2.0))
            data[f"ssc_{name}_{S}"] = np.asarray(img.resize((nw, nh), Image.BICUBIC).crop((left, top, left + S, top + S)))
    for n in sorted({n for n, _ in SWEEP}):
        arr = np.random.default_rng(5000 + n).integers(0, 256, size=(2, n, 3), dtype=np.uint8)
        if n % 2:
            arr[0] = (np.arange(n) % 2 * 255).astype(np.uint8)[:, None]  # a 0 / 255 row next to the noise
        data[f"sweep_in_{n}"] = arr
        for m in sorted(m for k, m in SWEEP if k == n):
            data[f"sweep_{n}_{m}"] = np.asarray(Image.fromarray(arr, "RGB").resize((m, 2), Image.BICUBIC))
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes,", len(data), "arrays, Pillow", PIL.__version__)
    return 0


if __name__ == "__main__":
    sys.exit(main())
