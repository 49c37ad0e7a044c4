"""Records tests/golden/augment_ref.npz from the reference's own transform/randaugment.py (data only: inputs, outputs, call lists).

    python tools/make_augment_golden.py --reference /path/to/reference [--out tests/golden/augment_ref.npz]

The reference imports cv2, which this project's environment does not have.  The recorder puts a stand-in module of its own into
sys.modules: split, merge and calcHist are numpy (they only move bytes and count them); warpAffine and getRotationMatrix2D raise;
filter2D returns an object that raises when it is used, because sharpness_func calls it before it looks at the factor and returns
its input untouched at factor 1.0 - the one Sharpness case recorded.  So nothing recorded here was computed by a stand-in for an
OpenCV algorithm.

Recorded: the outputs of Identity, AutoContrast, Equalize, Brightness (1.0, 0.64) and Sharpness (1.0) on five 24 x 20 images, and
for seeds 0 .. 63 the (name, args) calls RandomAugment(2, 5, augs=<the ten names of data/__init__.py>) hands to its functions."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUGS = ["Identity", "AutoContrast", "Brightness", "Sharpness", "Equalize", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"]
W, H = 24, 20


class _Unavailable:
    def __init__(self, what):
        object.__setattr__(self, "_what", what)

    def __getattr__(self, name):
        raise RuntimeError(f"{object.__getattribute__(self, '_what')} is not available: the result of the stand-in was used")

    __getitem__ = __array__ = __getattr__


def _raises(what):
    def f(*a, **k):
        raise RuntimeError(f"cv2.{what} is not available to the recorder")
    return f


def stand_in_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.split = lambda img: [np.ascontiguousarray(img[:, :, c]) for c in range(img.shape[2])]
    cv2.merge = lambda channels: np.stack(channels, axis=2)

    def calc_hist(images, channels, mask, hist_size, ranges):
        assert len(images) == 1 and channels == [0] and mask is None and hist_size == [256] and list(ranges) == [0, 256]
        return np.bincount(images[0].reshape(-1), minlength=256).astype(np.float32).reshape(256, 1)  # cv2's f32 [256, 1]
    cv2.calcHist = calc_hist
    cv2.filter2D = lambda *a, **k: _Unavailable("cv2.filter2D")
    cv2.warpAffine = _raises("warpAffine")
    cv2.getRotationMatrix2D = _raises("getRotationMatrix2D")
    cv2.INTER_LINEAR = 1
    return cv2


def images():
    rng = np.random.default_rng(20240)
    noise = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    constant = np.empty((H, W, 3), dtype=np.uint8)
    constant[:] = (7, 128, 255)
    minima = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) // 2 + np.array([5, 40, 100], dtype=np.uint8)
    two = noise.copy()
    two[:, :, 1] = np.where(rng.random((H, W)) < 0.3, 60, 200)
    ramp = np.empty((H, W, 3), dtype=np.uint8)
    base = (np.arange(H * W).reshape(H, W) * 255 // (H * W - 1))
    ramp[:, :, 0], ramp[:, :, 1], ramp[:, :, 2] = base, 255 - base, base // 3 + 20
    return {"noise": noise, "constant": constant, "minima": minima.astype(np.uint8), "twolevel": two, "ramp": ramp}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project (holds transform/randaugment.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "augment_ref.npz"))
    args = ap.parse_args()
    sys.modules["cv2"] = stand_in_cv2()
    sys.path.insert(0, args.reference)
    from transform import randaugment as R

    out = {"numpy_version": np.array(np.__version__), "augs": np.array(AUGS)}
    cases = [("Identity", ()), ("AutoContrast", ()), ("Equalize", ()), ("Brightness", (1.0,)), ("Brightness", (0.64,)),
             ("Sharpness", (1.0,))]
    for key, img in images().items():
        out[f"in_{key}"] = img
        for name, a in cases:
            got = R.func_dict[name](img.copy(), *a)
            assert got.dtype == np.uint8 and got.shape == img.shape
            out["out_" + "_".join([name] + [repr(v) for v in a]) + f"_{key}"] = got

    calls = []
    real = dict(R.func_dict)
    for name in real:
        R.func_dict[name] = (lambda n: lambda img, *a: (calls.append([n, [v if not isinstance(v, tuple) else list(v) for v in a]]), img)[1])(name)
    sequences = []
    aug = R.RandomAugment(2, 5, isPIL=True, augs=list(AUGS))
    for seed in range(64):
        np.random.seed(seed)
        del calls[:]
        aug(np.zeros((4, 4, 3), dtype=np.uint8))
        sequences.append([list(c) for c in calls])
    R.func_dict.update(real)
    out["sequences"] = np.array(json.dumps(sequences))
    np.savez_compressed(args.out, **out)
    print(args.out, os.path.getsize(args.out), "bytes;", sum(len(s) for s in sequences), "calls in 64 sequences")


if __name__ == "__main__":
    main()
