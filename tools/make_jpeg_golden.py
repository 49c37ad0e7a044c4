"""Records tests/golden/jpeg_pil.npz: JPEG byte strings that Pillow encoded from seeded images, the pixels Pillow decodes them to
(Image.open(...).convert("RGB")), and the identification of the Pillow / libjpeg that did both.  CPU only, needs Pillow.

    python tools/make_jpeg_golden.py [--out tests/golden/jpeg_pil.npz] [--dump DIR]

--dump DIR also writes every byte string as DIR/<name>.jpg (the input of tools/jpeg_host_check.cpp).  The tests read the recorded
file and need no Pillow; test_jpeg_cpu.py re-decodes the byte strings with the installed Pillow where there is one."""
import argparse
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (height, width): one pixel, sides below a block, one block and a bit, narrow chroma planes (replication rules), whole MCUs, odd
# sizes, and one of several workgroups and MCU rows
SIZES = [(1, 1), (5, 3), (3, 5), (8, 9), (17, 4), (2, 70), (16, 16), (33, 31), (37, 53), (48, 64), (150, 210)]
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
QUALITIES = (30, 85, 100)


def noise(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8)


def smooth(seed, h, w):
    """low-frequency ramps with two hard-edged rectangles"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3), dtype=np.float64)
    for c in range(3):
        a, b, p = rng.uniform(0.5, 2.0, 3)
        img[:, :, c] = 127.5 + 127.5 * np.sin(a * x / max(w, 8) * 3.0 + p) * np.cos(b * y / max(h, 8) * 3.0)
    img[h // 4:h // 2, w // 3:w // 2] = rng.randint(0, 256, 3)
    img[h // 2:, : w // 5] = rng.randint(0, 256, 3)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def hard_edges(seed, h, w):
    """noise of pure 0 / 255: with extreme quantisation tables the IDCT output saturates"""
    return (np.random.RandomState(seed).randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)


def corpus():
    """-> [(name, uint8 image (RGB or L), Pillow save options)]"""
    items = []
    for i, (h, w) in enumerate(SIZES):
        for j, (tag, sub) in enumerate(SUBSAMPLING.items()):
            big = h * w > 10000
            kind = "smooth" if big or (i + j) % 2 else "noise"
            q = 85 if big else QUALITIES[(i + j) % 3]
            img = (smooth if kind == "smooth" else noise)(1000 + 10 * i + j, h, w)
            items.append((f"{h}x{w}_{tag}_q{q}_{kind}", img, dict(quality=q, subsampling=sub)))
    items.append(("33x31_gray_q85", smooth(2000, 33, 31)[:, :, 1].copy(), dict(quality=85)))
    items.append(("37x53_420_q85_restart", noise(2001, 37, 53), dict(quality=85, subsampling=2, restart_marker_blocks=1)))
    items.append(("48x64_422_q30_restart3", smooth(2002, 48, 64), dict(quality=30, subsampling=1, restart_marker_blocks=3)))
    items.append(("40x24_gray_q100_restart", noise(2003, 40, 24)[:, :, 0].copy(), dict(quality=100, restart_marker_blocks=2)))
    items.append(("48x64_422_q85_optimize", noise(2004, 48, 64), dict(quality=85, subsampling=1, optimize=True)))
    items.append(("37x53_420_q30_optimize", smooth(2005, 37, 53), dict(quality=30, subsampling=2, optimize=True)))
    items.append(("33x31_420_qt255", hard_edges(2006, 33, 31), dict(subsampling=2, qtables=[[255] * 64, [255] * 64])))
    items.append(("33x31_444_qt1", hard_edges(2007, 33, 31), dict(subsampling=0, qtables=[[1] * 64, [1] * 64])))
    items.append(("17x23_422_qt255", hard_edges(2008, 17, 23), dict(subsampling=1, qtables=[[255] * 64, [255] * 64])))
    return items


def main():
    from PIL import Image, features, __version__ as pil_version
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz"))
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    arrays = {}
    names = []
    for name, img, options in corpus():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **options)
        data = buf.getvalue()
        pixels = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        arrays["jpg_" + name] = np.frombuffer(data, dtype=np.uint8)
        arrays["pix_" + name] = pixels
        names.append(name)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, name + ".jpg"), "wb") as f:
                f.write(data)
    arrays["names"] = np.array(names)
    arrays["pillow"] = np.array([f"Pillow {pil_version}", f"jpg {features.version('jpg')}",
                                 f"libjpeg_turbo {features.check_feature('libjpeg_turbo')}"])
    np.savez_compressed(args.out, **arrays)
    size = os.path.getsize(args.out)
    print(f"{args.out}: {len(names)} files, {size} bytes; {', '.join(arrays['pillow'].tolist())}")
    if size > 400 * 1024:
        raise SystemExit("the fixture is over 400 KB")


if __name__ == "__main__":
    main()
