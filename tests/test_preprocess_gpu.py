"""The image pipeline on the GPU (madtp_amd/preprocess.py, csrc/image.hip) against tests/image_ref.py - Pillow's arithmetic
restated, itself checked against Pillow in test_preprocess_cpu.py - followed by the torch-CPU ToTensor + Normalize, and against
what Pillow returned for the recorded fixture.  Every compare is torch.equal: the arithmetic is integer, there is no tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

from madtp_amd import preprocess
from tests import image_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imgprep_pil.npz")

# (width, height): one pixel, one column, one row, odd sizes, the 0 / 255 board, a downscale of 2.6 to 32, a downscale on one
# axis with an upscale on the other, a row table of 25 coefficients at 32
SOURCES = [(1, 1), (1, 7), (7, 1), (33, 41), (97, 131), (250, 190), (300, 50), (384, 36)]
SIZES = [32, 40, 96, (40, 96)]  # one tile, less than a tile, more than one tile with a ragged edge (96 = 64 + 32), Sh != Sw


@functools.lru_cache(maxsize=None)
def source(i):
    w, h = SOURCES[i]
    return image_ref.checkerboard(h, w) if (w, h) == (97, 131) else image_ref.random_image(300 + i, h, w)


def _hw(size):
    return (size, size) if isinstance(size, int) else size


@functools.lru_cache(maxsize=None)
def reference(i, size, box=None, flip=False):
    """f32 [3, Sh, Sw] of source i: crop, image_ref.resize, flip, torch-CPU normalise (computed once, shared, never written)"""
    Sh, Sw = _hw(size)
    img = source(i)
    if box is not None:
        l, u, r, d = box
        img = img[u:d, l:r]
    out = image_ref.resize(img, Sw, Sh)
    return image_ref.to_tensor_normalize(out[:, ::-1] if flip else out)


@functools.lru_cache(maxsize=None)
def pipeline(size, mode="stretch"):
    return preprocess.ImagePipeline(size, mode)


def run(size, images, **kw):
    out = pipeline(size)(images, **kw)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == (len(images), 3) + _hw(size)
    return out.cpu()


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_every_source_in_one_batch(size):
    got = run(size, [source(i) for i in range(len(SOURCES))])
    for i in range(len(SOURCES)):
        assert torch.equal(got[i], reference(i, size)), SOURCES[i]


def test_mixed_batch_equals_single_image_calls():
    ids = [5, 0, 4, 6, 3]
    got = run(40, [source(i) for i in ids])
    for j, i in enumerate(ids):
        assert torch.equal(run(40, [source(i)])[0], got[j]) and torch.equal(got[j], reference(i, 40))


def test_input_kinds_agree():
    arrays = [source(3), source(5)]
    want = torch.stack([reference(3, 32), reference(5, 32)])
    assert torch.equal(run(32, [torch.from_numpy(a.copy()) for a in arrays]), want)
    assert torch.equal(run(32, [np.asfortranarray(arrays[0]), arrays[1][:, ::1]]), want)
    Image = pytest.importorskip("PIL.Image")
    assert torch.equal(run(32, [Image.fromarray(a, "RGB") for a in arrays]), want)


# boxes (left, upper, right, lower) that touch the border on every side, on some sides and on none; odd offsets (3-byte pixels
# at every alignment) and a box that turns the downscale into an upscale
BOXES = [(4, (0, 0, 97, 131)), (4, (0, 7, 50, 131)), (4, (5, 7, 90, 100)), (5, (1, 1, 249, 189)), (5, (101, 33, 250, 80)),
         (5, (13, 0, 38, 190)), (6, (100, 0, 160, 50)), (3, (32, 40, 33, 41))]


@pytest.mark.parametrize("size", [32, (40, 96)], ids=str)
def test_crop_boxes(size):
    got = run(size, [source(i) for i, _ in BOXES], boxes=[b for _, b in BOXES])
    for j, (i, box) in enumerate(BOXES):
        assert torch.equal(got[j], reference(i, size, box)), (SOURCES[i], box)


def test_flips_and_boxes_in_one_batch():
    ids = [3, 4, 5, 6, 7, 1]
    flips = [True, False, True, True, False, True]
    boxes = [None, (5, 7, 90, 100), (101, 33, 250, 80), None, None, None]
    for size in (40, 96):
        got = run(size, [source(i) for i in ids], boxes=boxes, flips=flips)
        for j, i in enumerate(ids):
            assert torch.equal(got[j], reference(i, size, boxes[j], flips[j])), (size, SOURCES[i])


def test_recorded_pillow_outputs():
    """the fixture's Pillow bytes (resize, crop + resize, resize + flip, short side + centre crop), normalised on the CPU"""
    g = np.load(GOLDEN)
    seen = set()
    for key in g.files:
        parts = key.split("_")
        kind = parts[0]
        if kind not in ("resize", "flip", "crop", "ssc"):
            continue
        want = image_ref.to_tensor_normalize(g[key])
        if kind == "ssc":
            img = g["in_" + "_".join(parts[1:-1])]
            got = pipeline(int(parts[-1]), "short_side_crop")([img])
        else:
            W, H = map(int, parts[-1].split("x"))
            box = tuple(map(int, parts[-5:-1])) if kind == "crop" else None
            img = g["in_" + "_".join(parts[1:-5 if kind == "crop" else -1])]
            got = pipeline((H, W))([img], boxes=[box], flips=[kind == "flip"])
        assert torch.equal(got[0].cpu(), want), key
        seen.add(kind)
    assert seen == {"resize", "flip", "crop", "ssc"}


def test_short_side_crop_batch():
    ids = [3, 4, 5, 6, 2]
    for size in (32, 40):
        got = pipeline(size, "short_side_crop")([source(i) for i in ids]).cpu()
        for j, i in enumerate(ids):
            assert torch.equal(got[j], image_ref.to_tensor_normalize(image_ref.short_side_crop(source(i), size))), (size, SOURCES[i])


def test_identical_calls_give_identical_bits():
    images = [source(i) for i in (5, 4, 6, 7)]
    a, b = run(96, images), run(96, images)
    assert torch.equal(a, b) and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_non_default_stream():
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = pipeline(40)([source(5), source(3)])
    stream.synchronize()
    assert torch.equal(out.cpu(), torch.stack([reference(5, 40), reference(3, 40)]))


def test_out_is_reused():
    out = torch.full((2, 3, 32, 32), float("nan"), device="cuda")
    assert pipeline(32)([source(5), source(3)], out=out) is out
    assert torch.equal(out.cpu(), torch.stack([reference(5, 32), reference(3, 32)]))
    assert pipeline(32)([source(6), source(4)], out=out) is out
    assert torch.equal(out.cpu(), torch.stack([reference(6, 32), reference(4, 32)]))
    with pytest.raises(ValueError):
        pipeline(32)([source(6)], out=out)
    with pytest.raises(ValueError):
        pipeline(32)([source(6), source(4)], out=out.double())


def test_device_resident_input_equals_cpu_input():
    ids = [5, 4, 3, 0]
    boxes = [(101, 33, 250, 80), (5, 7, 90, 100), None, None]
    flips = [False, True, False, False]
    dev = [torch.from_numpy(source(i).copy()).cuda() for i in ids]
    for size in (32, (40, 96)):
        got = run(size, dev, boxes=boxes, flips=flips)
        assert torch.equal(got, run(size, [source(i) for i in ids], boxes=boxes, flips=flips))
        for j, i in enumerate(ids):
            assert torch.equal(got[j], reference(i, size, boxes[j], flips[j]))
    with pytest.raises(ValueError, match="image 0"):
        pipeline(32)([dev[0], source(3)])


def test_staging_buffers_alternate():
    """more calls than staging buffers, back to back, each batch of another size: a buffer is rewritten only after its copy"""
    pipe = preprocess.ImagePipeline(32)
    batches = [[5, 4], [3], [6, 7, 5], [4], [5, 3, 2, 1, 0]]
    outs = [pipe([source(i) for i in ids]) for ids in batches]
    for ids, out in zip(batches, outs):
        assert torch.equal(out.cpu(), torch.stack([reference(i, 32) for i in ids]))


def test_raw_batch_to_device():
    samples = [(torch.from_numpy(source(i).copy()), f"caption {i}", i) for i in (5, 3, 6)]
    image, caption, idx = preprocess.collate(samples, size=40)
    x = image.to(torch.device("cuda"), non_blocking=True)
    assert torch.equal(x.cpu(), torch.stack([reference(i, 40) for i in (5, 3, 6)])) and idx.tolist() == [5, 3, 6]


def test_forward_on_the_pipeline_output():
    """plumbing: the f32 batch the pipeline makes is the tensor a model takes - one fp32-mode forward of the harness's NLVR model on
    it equals the forward on the CPU-prepared tensor"""
    from madtp_amd import harness, runtime
    raw = [image_ref.random_image(900, 300, 260), image_ref.random_image(901, 200, 330)]
    x = preprocess.ImagePipeline(224)(raw)
    ref = torch.stack([image_ref.to_tensor_normalize(image_ref.resize(a, 224, 224)) for a in raw])
    assert torch.equal(x.cpu(), ref)
    model = harness.build_nlvr(224, 0, "cuda")
    _, text, targets = harness.nlvr_inputs(1, 224, 20, seed=5)
    with runtime.precision("fp32"):
        got, _ = harness.run_nlvr(model, x, text, targets, 5.0)
        want, _ = harness.run_nlvr(model, ref.cuda(), text, targets, 5.0)
    assert torch.isfinite(got).all() and torch.equal(got, want)
