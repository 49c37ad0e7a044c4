"""CPU side of the training transform (madtp_amd/augment.py, include/madtp_augment.h): tests/augment_ref.py against what the
reference's own functions returned (tests/golden/augment_ref.npz, recorded by tools/make_augment_golden.py), the sampler against
the reference's recorded draws, the properties of the fixed-point warp, the module's host tables, the refusals that need no GPU
and the exported symbols."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from madtp_amd import abi, augment, hip, preprocess
from tests import augment_ref, image_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")
WARPS = [("ShearX", 0.15), ("ShearX", -0.15), ("ShearY", 0.15), ("ShearY", -0.15), ("TranslateX", 5.0), ("TranslateX", -5.0),
         ("TranslateY", 5.0), ("TranslateY", -5.0), ("Rotate", 15.0), ("Rotate", -15.0)]


def _golden():
    return np.load(GOLDEN)


def _recorded_outputs(g):
    """(key, op name, args, input image, recorded output)"""
    for key in g.files:
        if key.startswith("out_"):
            parts = key.split("_")
            yield key, parts[1], tuple(float(v) for v in parts[2:-1]), g["in_" + parts[-1]], g[key]


def test_reference_restatement_equals_every_recorded_output():
    g = _golden()
    assert os.path.getsize(GOLDEN) < 200_000 and list(g["augs"]) == augment_ref.AUGS == list(augment.REFERENCE_AUGS)
    seen = set()
    for key, name, args, img, want in _recorded_outputs(g):
        assert np.array_equal(augment_ref.apply(img, name, args), want), key
        seen.add((name,) + args)
    assert seen == {("Identity",), ("AutoContrast",), ("Equalize",), ("Brightness", 1.0), ("Brightness", 0.64), ("Sharpness", 1.0)}
    inputs = [k for k in g.files if k.startswith("in_")]
    assert len(inputs) == 5 and all(g[k].shape == (20, 24, 3) for k in inputs)
    # the cases the fixture is there for: a flat image (step == 0, hi <= lo), minima above 0 (the wrapped offset), two grey levels
    assert all(np.ptp(g["in_constant"][:, :, c]) == 0 for c in range(3)) and g["in_minima"].min(axis=(0, 1)).min() > 0
    assert len(np.unique(g["in_twolevel"][:, :, 1])) == 2
    assert not np.array_equal(g["out_AutoContrast_minima"], g["in_minima"])


def test_sampler_equals_every_recorded_sequence():
    sequences = json.loads(str(_golden()["sequences"]))
    assert len(sequences) == 64
    names = set()
    for seed, want in enumerate(sequences):
        want = [(n, tuple(tuple(v) if isinstance(v, list) else v for v in a)) for n, a in want]
        assert augment.RandAugmentSampler(2, 5, augment.REFERENCE_AUGS, np.random.RandomState(seed)).sample() == want, seed
        assert augment_ref.sample(np.random.RandomState(seed)) == want, seed
        names.update(n for n, _ in want)
    assert names == set(augment.REFERENCE_AUGS)  # every op, and both signs of some
    # at the configured level Brightness and Sharpness are the identity, and every drawn call compiles
    for want in sequences:
        for n, a in want:
            augment.compile_op(n, tuple(tuple(v) if isinstance(v, list) else v for v in a), 384, 384)
    assert augment.level_to_args("Brightness", 5, None) == (1.0,) and augment.compile_op("Brightness", (1.0,), 8, 8) == ("copy",)


def smooth_image(h=48, w=64):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([np.rint(128 + 100 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c)) for c in range(3)], axis=2).astype(np.uint8)


def float_bilinear(img, a):
    """float64 bilinear sampling at the same inverse map, taps outside the image 128, not rounded"""
    H, W = img.shape[:2]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    X, Y = a[0] * x + a[1] * y + a[2], a[3] * x + a[4] * y + a[5]
    sx, sy = np.floor(X).astype(np.int64), np.floor(Y).astype(np.int64)
    fx, fy = (X - sx)[:, :, None], (Y - sy)[:, :, None]
    src = img.astype(np.float64)

    def tap(yy, xx):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        return np.where(inside[:, :, None], src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 128.0)
    return ((1 - fx) * (1 - fy) * tap(sy, sx) + fx * (1 - fy) * tap(sy, sx + 1) + (1 - fx) * fy * tap(sy + 1, sx)
            + fx * fy * tap(sy + 1, sx + 1))


def test_warp_identity_and_integer_translations():
    img = image_ref.random_image(11, 37, 53)
    for name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        assert np.array_equal(augment_ref.apply(img, name, (0.0,)), img), name
    for off in (5, -5):
        shifted = np.full_like(img, 128)  # Translate(offset): the output pixel x shows the source pixel x + offset
        if off > 0:
            shifted[:, :-off] = img[:, off:]
        else:
            shifted[:, -off:] = img[:, :off]
        assert np.array_equal(augment_ref.apply(img, "TranslateX", (float(off), (128, 128, 128))), shifted), off
        shifted = np.full_like(img, 128)
        if off > 0:
            shifted[:-off] = img[off:]
        else:
            shifted[-off:] = img[:off]
        assert np.array_equal(augment_ref.apply(img, "TranslateY", (float(off),)), shifted), off


def test_warp_against_float64_bilinear():
    """The fixed-point warp against float64 bilinear sampling of the same inverse map on a smooth 64 x 48 image, all ten signed
    ops at the reference's level 5.  Measured on the CPU: the largest difference is 1.933 levels (Rotate(15), on the image's
    border, where a coordinate snapped to 1/32 pixel weighs the 128 fill against the image; the shears reach 1.4 - 1.6 there, the
    integer translations 0); where all four taps are inside the image it stays below 0.72.  Asserted at the measured value plus
    one level."""
    img = smooth_image()
    worst = 0.0
    for name, value in WARPS:
        a = augment_ref.inverse_map(augment_ref.forward_matrix(name, value, 64, 48))
        d = np.abs(augment_ref.warp(img, a).astype(np.float64) - float_bilinear(img, a)).max()
        print(f"{name}({value}): max |fixed - float64| = {d:.3f}")
        worst = max(worst, d)
    print(f"worst {worst:.3f}")
    assert worst <= 1.934 + 1.0


def test_host_tables_equal_the_restatement():
    for factor in (1.0, 0.64, 0.1, 1.9, 0.0, 3.5):
        assert np.array_equal(augment.brightness_table(factor), augment_ref.brightness_table(factor))
    assert np.array_equal(augment.brightness_table(1.0), np.arange(256))
    s = augment.scale255_table()
    assert s.dtype == np.float64 and s.shape == (256,) and all(s[d] == 255.0 / d for d in range(1, 256))
    for W, H in ((64, 48), (5, 7), (130, 130)):
        for name, value in WARPS + [("Rotate", 0.0), ("ShearX", 0.3)]:
            m = augment.forward_matrix(name, value, W, H)
            assert m == augment_ref.forward_matrix(name, value, W, H) and augment.inverse_map(m) == augment_ref.inverse_map(m)
            assert augment.compile_op(name, (value, (128, 128, 128)), H, W) == ("warp", augment_ref.inverse_map(m))
    rows, tables, masks = augment.build_plan([[("Equalize", ()), ("Rotate", (15.0,))], [], [("Identity", ()), ("Brightness", (0.64,))]], 48, 64)
    assert rows.shape == (2, 3, augment.FIELDS) and rows[:, :, 0].tolist() == [[augment.OP_EQUALIZE, 0, augment.OP_TABLE], [augment.OP_WARP, 0, 0]]
    assert np.array_equal(tables[0][2], augment_ref.brightness_table(0.64)) and tables[0][0] is None
    assert masks == [1 << augment.OP_EQUALIZE | 1 | 1 << augment.OP_TABLE, 1 << augment.OP_WARP | 1]
    a = augment_ref.inverse_map(augment_ref.forward_matrix("Rotate", 15.0, 64, 48))
    assert rows[1, 0, 2:8].view(np.float64).tolist() == a
    assert augment.build_plan([[], []], 8, 8)[0].shape == (1, 2, augment.FIELDS)  # N = 0: the one pass that normalises


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "madtp_augment.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))


def test_symbols_are_exported_and_the_other_abis_are_unchanged():
    from madtp_amd import build
    raw = ctypes.CDLL(build.build(verbose=False))
    syms = _header_symbols()
    assert syms == sorted(augment.SIGNATURES) and all(s.startswith("madtp_augment_") for s in syms)
    assert {"madtp_augment_abi_version", "madtp_augment_resize_u8", "madtp_augment_stats", "madtp_augment_apply"} == set(syms)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/madtp_augment.h but not exported"
    lib = augment.lib()
    assert lib.madtp_augment_abi_version() == augment.ABI_VERSION == 1
    for name, (res, args) in augment.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    assert augment.SIGNATURES["madtp_augment_resize_u8"] == (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p])
    assert len(abi.SIGNATURES) == 97 and not set(abi.SIGNATURES) & set(syms) and not set(preprocess.SIGNATURES) & set(syms)
    assert hip.ABI_VERSION == 31 and lib.madtp_image_abi_version() == preprocess.ABI_VERSION == 1
    assert "augment.hip" in build.SOURCES and any(h.endswith("madtp_augment.h") for h in build.HEADERS)


def test_entry_points_refuse_before_any_launch():
    lib = augment.lib()
    E_BADARG, E_SHAPE = abi.DEFINES["MADTP_E_BADARG"], abi.DEFINES["MADTP_E_SHAPE"]
    ok = dict(src=16, table=16, out=16, B=1, Sh=32, Sw=32, n_blocks=1, max_ksize=5)

    def resize(**kw):
        a = dict(ok, **kw)
        return lib.madtp_augment_resize_u8(a["src"], a["table"], a["out"], a["B"], a["Sh"], a["Sw"], a["n_blocks"], a["max_ksize"], 0)
    for name in ("src", "table", "out"):
        assert resize(**{name: 0}) == E_BADARG, name
    assert resize(B=0) == E_BADARG and resize(n_blocks=0) == E_BADARG and resize(Sh=0) == E_SHAPE and resize(Sw=-1) == E_SHAPE
    assert resize(max_ksize=preprocess.MAX_KSIZE + 2) == E_SHAPE and resize(max_ksize=0) == E_SHAPE

    ok2 = dict(inp=16, plan=16, scale=16, lut=16, norm=16, out=16, B=1, Sh=32, Sw=32, mask=1 << augment.OP_EQUALIZE)

    def stats(**kw):
        a = dict(ok2, **kw)
        return lib.madtp_augment_stats(a["inp"], a["plan"], a["scale"], a["lut"], a["B"], a["Sh"], a["Sw"], a["mask"], 0)

    def apply(**kw):
        a = dict(ok2, **kw)
        return lib.madtp_augment_apply(a["inp"], a["plan"], a["lut"], a["norm"], a["out"], a["B"], a["Sh"], a["Sw"], a["mask"], 0)
    for name in ("inp", "plan", "scale", "lut"):
        assert stats(**{name: 0}) == E_BADARG, name
    for name in ("inp", "plan", "lut", "out"):
        assert apply(**{name: 0}) == E_BADARG, name
    unknown = 1 << augment.DEFINES["MADTP_AUGMENT_OPS"]  # an op code the header does not have
    for call in (stats, apply):
        assert call(B=0) == E_BADARG and call(B=-2) == E_BADARG and call(mask=unknown) == E_BADARG and call(mask=0) == E_BADARG
        assert call(mask=unknown | 1) == E_BADARG
        assert call(Sh=0) == E_SHAPE and call(Sw=0) == E_SHAPE and call(Sh=4096, Sw=4096) == E_SHAPE and call(Sh=1 << 20, Sw=1 << 20) == E_SHAPE
    assert stats(mask=1 << augment.OP_COPY | 1 << augment.OP_WARP) == 0  # no image needs statistics: no launch, nothing read


def test_unsupported_ops_and_sizes_raise():
    good = [image_ref.random_image(1, 20, 30)]
    tf = augment.TrainTransform(32, seed=0)
    with pytest.raises(ValueError, match="image 0.*Sharpness.*0.64"):
        tf(good, ops=[[("Sharpness", (0.64,))]])
    with pytest.raises(ValueError, match="image 1.*Color"):
        tf(good * 2, ops=[[], [("Color", (1.0,))]])
    for name in ("Contrast", "Solarize", "Posterize"):
        with pytest.raises(ValueError, match=name):
            augment.compile_op(name, (1,), 32, 32)
    with pytest.raises(ValueError, match="Color"):
        augment.TrainTransform(32, augs=("Identity", "Color"))
    with pytest.raises(ValueError, match="2\\^24"):
        augment.TrainTransform((4097, 4096))
    with pytest.raises(ValueError, match="2\\^24"):
        augment.TrainTransform(4096)
    with pytest.raises(ValueError, match="image 0.*Rotate"):
        tf(good, ops=[[("Rotate", (float("nan"),))]])
    with pytest.raises(ValueError, match="image 0.*fills"):
        tf(good, ops=[[("ShearX", (0.1, (0, 0, 0)))]])
    with pytest.raises(ValueError, match="image 0.*float32"):
        tf([good[0].astype(np.float32)])
    with pytest.raises(ValueError, match="op lists"):
        tf(good, ops=[[], []])


def test_transform_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good = image_ref.random_image(1, 20, 30)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        augment.TrainTransform(32, seed=1)([good])
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        augment.TrainTransform(32, device="cpu")([good])
    batch = augment.collate([(torch.from_numpy(good), "a", 3)], size=32)
    assert isinstance(batch[0], augment.RawTrainBatch) and len(batch[0]) == 1 and batch[1] == ["a"]
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        batch[0].to("cuda", non_blocking=True)


def test_crop_boxes_and_draws_are_seeded():
    g = torch.Generator().manual_seed(3)
    boxes = [augment.random_resized_crop_box(640, 480, (0.5, 1.0), generator=g) for _ in range(200)]
    for l, u, r, d in boxes:
        assert 0 <= l < r <= 640 and 0 <= u < d <= 480
        assert 0.49 <= (r - l) * (d - u) / (640 * 480) <= 1.01 and 0.74 <= (r - l) / (d - u) <= 1.35
    assert len(set(boxes)) > 150
    assert augment.random_resized_crop_box(1, 1, generator=g) == (0, 0, 1, 1)
    l, u, r, d = augment.random_resized_crop_box(1000, 10, (0.9, 1.0), generator=g)  # no attempt fits: the centre crop at ratio 4/3
    assert (u, d) == (0, 10) and r - l == 13 and l == (1000 - 13) // 2
    assert math.isclose(abs(augment.level_to_args("ShearX", 5, np.random.RandomState(0))[0]), 0.15)
