"""The training transform on the GPU (madtp_amd/augment.py, csrc/augment.hip) against tests/image_ref.py (Pillow's resize restated)
followed by tests/augment_ref.py (the reference's ops restated, checked against its recorded outputs in test_augment_cpu.py) and
the torch-CPU ToTensor + Normalize.  Every compare is torch.equal: the arithmetic is integer, there is no tolerance."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from madtp_amd import augment
from tests import augment_ref, image_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment_ref.npz")

# (width, height), as test_preprocess_gpu.SOURCES: one pixel, one column, one row, odd sizes, down- and upscales
SOURCES = [(1, 1), (1, 7), (7, 1), (33, 41), (97, 131), (250, 190), (300, 50), (384, 36)]
# less than a tile; exactly one tile column of the resize; ragged with Sh != Sw; three tile columns, ragged, an odd number of pixels
# per plane is (5, 7): the byte path of the apply kernel, the others take the dword path
SIZES = [(5, 7), 64, (40, 96), 130]
FILL = (128, 128, 128)
SIGNED = {"ShearX": 0.15, "ShearY": 0.15, "TranslateX": 5.0, "TranslateY": 5.0, "Rotate": 15.0}


@functools.lru_cache(maxsize=None)
def source(i):
    w, h = SOURCES[i]
    if i == 3:  # a constant image: Equalize's step == 0, AutoContrast's hi <= lo
        img = np.empty((h, w, 3), dtype=np.uint8)
        img[:] = (9, 130, 255)
        return img
    if i == 5:  # minima above 0 in every channel: AutoContrast's wrapped offset
        return (image_ref.random_image(300 + i, h, w) // 2 + np.array([7, 40, 90], dtype=np.uint8)).astype(np.uint8)
    if i == 4:  # few grey levels: Equalize with most bins empty
        return (image_ref.random_image(300 + i, h, w) // 64 * 60 + 3).astype(np.uint8)
    return image_ref.random_image(300 + i, h, w)


def _hw(size):
    return (size, size) if isinstance(size, int) else size


@functools.lru_cache(maxsize=None)
def resized(i, size, box=None, flip=False):
    """uint8 [Sh, Sw, 3] of source i: crop, image_ref.resize, flip (computed once, shared, never written)"""
    Sh, Sw = _hw(size)
    img = source(i)
    if box is not None:
        l, u, r, d = box
        img = img[u:d, l:r]
    out = image_ref.resize(img, Sw, Sh)
    out = np.ascontiguousarray(out[:, ::-1] if flip else out)
    return out


def want(i, size, calls, box=None, flip=False):
    return image_ref.to_tensor_normalize(augment_ref.apply_all(resized(i, size, box, flip), calls))


@functools.lru_cache(maxsize=None)
def transform(size):
    return augment.TrainTransform(size, seed=0)


def run(size, images, ops, boxes=None, flips=None):
    n = len(images)
    out = transform(size)(images, boxes=[None] * n if boxes is None else boxes, flips=[False] * n if flips is None else flips, ops=ops)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (n, 3) + _hw(size)
    return out.cpu()


def small_box(i, size):
    """None, or the top left corner of source i that keeps the downscale to `size` within the resize's ratio of 16"""
    (w, h), (Sh, Sw) = SOURCES[i], _hw(size)
    return None if w <= 14 * Sw and h <= 14 * Sh else (0, 0, min(w, 14 * Sw), min(h, 14 * Sh))


def call_of(name, sign=1):
    if name in SIGNED:
        return (name, (sign * SIGNED[name], FILL))
    return (name, {"Brightness": (0.64,), "Sharpness": (1.0,)}.get(name, ()))


@pytest.mark.parametrize("size", SIZES, ids=str)
@pytest.mark.parametrize("name", augment.REFERENCE_AUGS)
def test_each_op_alone(name, size):
    images = [source(i) for i in range(len(SOURCES))]
    boxes = [small_box(i, size) for i in range(len(SOURCES))]
    for sign in (1, -1) if name in SIGNED else (1,):
        call = call_of(name, sign)
        got = run(size, images, [[call]] * len(images), boxes)
        for i in range(len(SOURCES)):
            assert torch.equal(got[i], want(i, size, [call], boxes[i])), (name, sign, SOURCES[i])
    if name == "Brightness":  # the identity table of the configured level, and a table that saturates
        for factor in (1.0, 1.9):
            call = ("Brightness", (factor,))
            got = run(size, images[4:6], [[call]] * 2, boxes[4:6])
            assert torch.equal(got[0], want(4, size, [call], boxes[4])) and torch.equal(got[1], want(5, size, [call], boxes[5]))


def test_all_ordered_pairs_in_one_batch():
    """100 ordered pairs x three images, every row of the batch with its own plan; the second op of a pair works on the first
    op's output (a histogram after a warp counts the fill pixels)"""
    ids = (4, 5, 6)
    names = augment.REFERENCE_AUGS
    images, ops, keys = [], [], []
    for a, first in enumerate(names):
        for b, second in enumerate(names):
            for i in ids:
                sign = 1 if (a + b + i) % 2 else -1
                images.append(source(i))
                ops.append([call_of(first, sign), call_of(second, -sign)])
                keys.append((i, first, second, sign))
    got = run(40, images, ops)
    for j, (i, first, second, sign) in enumerate(keys):
        assert torch.equal(got[j], want(i, 40, ops[j])), keys[j]
    # the fill pixels are seen: Equalize after a rotation differs from Equalize of the rotation's input, rotated
    j = keys.index((5, "Rotate", "Equalize", 1 if (9 + 4 + 5) % 2 else -1))
    other = want(5, 40, [ops[j][1], ops[j][0]])
    assert not torch.equal(got[j], other)


def test_every_image_has_its_own_plan_box_and_flip():
    ids = [5, 4, 6, 3, 7, 5, 0, 4]
    boxes = [(101, 33, 250, 80), None, (100, 0, 160, 50), None, None, (13, 0, 38, 190), None, (5, 7, 90, 100)]
    flips = [True, False, True, False, True, False, False, True]
    ops = [[call_of("Rotate", -1), call_of("Equalize")], [], [call_of("AutoContrast")], [call_of("Identity"), call_of("ShearX")],
           [call_of("Sharpness"), call_of("TranslateY"), call_of("Brightness")], [call_of("AutoContrast"), call_of("ShearY", -1)], [],
           [call_of("Brightness"), call_of("TranslateX", -1)]]
    for size in (40, (40, 96)):
        got = run(size, [source(i) for i in ids], ops, boxes, flips)
        for j, i in enumerate(ids):
            assert torch.equal(got[j], want(i, size, ops[j], boxes[j], flips[j])), (size, j)
    # N = 0 on every row: the resize, one table pass
    got = run(40, [source(i) for i in ids], [[]] * len(ids), boxes, flips)
    for j, i in enumerate(ids):
        assert torch.equal(got[j], want(i, 40, [], boxes[j], flips[j])), j


def test_seeded_draws_repeat_and_replay():
    images = [image_ref.random_image(700 + i, 90 + 7 * i, 120 - 5 * i) for i in range(12)]
    a_tf, b_tf = augment.TrainTransform(40, seed=7), augment.TrainTransform(40, seed=7)
    a, b = a_tf(images), b_tf(images)
    assert torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32)) and a_tf.last_plan == b_tf.last_plan
    plan = a_tf.last_plan
    assert len(plan["boxes"]) == len(plan["flips"]) == len(plan["ops"]) == 12 and any(plan["flips"]) and not all(plan["flips"])
    assert any(plan["ops"]) and all(len(c) <= 2 for c in plan["ops"])
    replay = transform(40)(images, **plan)
    assert torch.equal(replay, a)
    for j, img in enumerate(images):
        l, u, r, d = plan["boxes"][j]
        out = image_ref.resize(img[u:d, l:r], 40, 40)
        out = augment_ref.apply_all(np.ascontiguousarray(out[:, ::-1] if plan["flips"][j] else out), plan["ops"][j])
        assert torch.equal(a[j].cpu(), image_ref.to_tensor_normalize(out)), j
    assert not torch.equal(a_tf(images), a)  # the next draw is another one


@pytest.mark.parametrize("size", [32, 40, 96, (40, 96)], ids=str)
def test_byte_stage_equals_the_resize(size):
    got = transform(size).resize_u8([source(i) for i in range(len(SOURCES))]).cpu()
    assert got.dtype == torch.uint8 and got.shape == (len(SOURCES), 3) + _hw(size)
    for i in range(len(SOURCES)):
        assert torch.equal(got[i], torch.from_numpy(resized(i, size)).permute(2, 0, 1)), SOURCES[i]


def test_recorded_reference_outputs():
    """what the reference's own functions returned for the fixture's images (a resize to the image's own size is the identity)"""
    g = np.load(GOLDEN)
    keys = [k for k in g.files if k.startswith("out_")]
    images, ops = [], []
    for key in keys:
        parts = key.split("_")
        images.append(g["in_" + parts[-1]])
        ops.append([(parts[1], tuple(float(v) for v in parts[2:-1]))])
    assert len(keys) == 30
    tf = transform((20, 24))
    assert torch.equal(tf.resize_u8(images[:5]).cpu(), torch.stack([torch.from_numpy(a).permute(2, 0, 1) for a in images[:5]]))
    got = tf(images, boxes=[None] * 30, flips=[False] * 30, ops=ops).cpu()
    for j, key in enumerate(keys):
        assert torch.equal(got[j], image_ref.to_tensor_normalize(g[key])), key
    # and the recorded draws of seeds 0 .. 7 as one batch
    sequences = json.loads(str(g["sequences"]))[:8]
    ops = [[(n, tuple(tuple(v) if isinstance(v, list) else v for v in a)) for n, a in s] for s in sequences]
    got = run(40, [source(5)] * 8, ops)
    for j in range(8):
        assert torch.equal(got[j], want(5, 40, ops[j])), sequences[j]


def test_stream_out_and_loader_batch():
    stream = torch.cuda.Stream()
    ops = [[call_of("Equalize"), call_of("Rotate")], [call_of("ShearX", -1)]]
    ref = torch.stack([want(5, 40, ops[0]), want(6, 40, ops[1])])
    out = torch.full((2, 3, 40, 40), float("nan"), device="cuda")
    with torch.cuda.stream(stream):
        assert transform(40)([source(5), source(6)], boxes=[None] * 2, flips=[False] * 2, ops=ops, out=out) is out
    stream.synchronize()
    assert torch.equal(out.cpu(), ref)
    dev = [torch.from_numpy(source(i).copy()).cuda() for i in (5, 6)]  # device-resident sources
    assert torch.equal(run(40, dev, ops), ref)
    with pytest.raises(ValueError):
        transform(40)([source(5)], out=out)
    samples = [(torch.from_numpy(source(i).copy()), f"caption {i}", i) for i in (5, 3, 6)]
    image, caption, idx = augment.collate(samples, size=40)
    x = image.to(torch.device("cuda"), non_blocking=True)
    assert x.shape == (3, 3, 40, 40) and x.dtype == torch.float32 and torch.isfinite(x).all() and idx.tolist() == [5, 3, 6]
