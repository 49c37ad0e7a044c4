"""The JPEG decode on the GPU (madtp_amd/jpeg.py, csrc/jpeg.hip) against the pixels Pillow decoded (tests/golden/jpeg_pil.npz) and
against tests/jpeg_ref.py - the decode restated in numpy, itself held against Pillow in test_jpeg_cpu.py.  Every compare is
torch.equal: the arithmetic is integer, there is no tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

from madtp_amd import jpeg, preprocess
from tests import image_ref, jpeg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_pil.npz")


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def names():
    return [str(n) for n in golden()["names"]]


def data(name):
    return golden()["jpg_" + name].tobytes()


def pixels(name):
    return torch.from_numpy(golden()["pix_" + name])


def named(prefix):
    return next(n for n in names() if n.startswith(prefix))


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement's pixels (computed once, shared, never written)"""
    return torch.from_numpy(jpeg_ref.decode(data(name)))


@functools.lru_cache(maxsize=None)
def decoder():
    return jpeg.JpegDecoder()


def check(out, name):
    want = pixels(name)
    assert out.is_cuda and out.dtype == torch.uint8 and out.shape == want.shape, name
    got = out.cpu()
    assert torch.equal(got, want), f"{name}: not Pillow's pixels"
    assert torch.equal(got, restated(name)), f"{name}: not the restatement's pixels"


def test_whole_corpus_as_one_mixed_batch():
    ns = names()
    outs = decoder()([data(n) for n in ns])
    assert len(outs) == len(ns)
    base = outs[0].untyped_storage().data_ptr()
    for n, out in zip(ns, outs):
        assert out.untyped_storage().data_ptr() == base  # views of one packed buffer
        check(out, n)


@pytest.mark.parametrize("name", names())
def test_batches_of_one(name):
    (out,) = decoder()([data(name)])
    check(out, name)


# ---- the device stages alone, at magnitudes no file has ------------------------------------------------------------------------------
def synthetic(seed, w, h, components, hs, vs, q):
    """an EntropyImage of made-up coefficients and the restatement's header for it"""
    rng = np.random.RandomState(seed)
    bx, by = -(-w // (8 * hs)) * hs, -(-h // (8 * vs)) * vs
    shapes = [(by, bx)] + [(by // vs, bx // hs)] * (components - 1)
    coef = []
    for i, (y, x) in enumerate(shapes):
        c = rng.choice(np.array([-2047, 2047], dtype=np.int16), size=(y, x, 8, 8))
        kind = rng.randint(0, 4, size=(y, x, 1, 1))
        c = np.where(kind == 1, c * (rng.rand(y, x, 8, 8) < 0.1), c)                      # a few extreme coefficients
        c = np.where(kind == 2, c * (np.arange(64).reshape(8, 8) == 0), c)                # the DC alone
        c = np.where(kind == 3, rng.randint(-2047, 2048, size=(y, x, 8, 8)), c)           # anything
        coef.append(c.astype(np.int16))
    qt = np.zeros((3, 64), dtype=np.uint16)
    qt[:components] = q
    info = np.zeros(jpeg.INFO_FIELDS, dtype=np.int32)
    for k, v in dict(WIDTH=w, HEIGHT=h, COMPONENTS=components, HS=hs, VS=vs, BLOCKS_X=bx, BLOCKS_Y=by, RESTART=0,
                     BLOCKS=sum(y * x for y, x in shapes)).items():
        info[jpeg._I[k]] = v
    packed = np.concatenate([c.transpose(0, 1, 3, 2).reshape(-1, 64) for c in coef])  # column-major blocks, component after component
    header = dict(width=w, height=h, components=components, hs=hs, vs=vs, qtables=qt)
    return jpeg.EntropyImage(info, torch.from_numpy(qt.copy()), torch.from_numpy(packed.copy())), header, coef


SYNTHETIC = [(53, 37, 3, 2, 2, 255), (53, 37, 3, 2, 1, 255), (31, 33, 3, 1, 1, 255), (40, 24, 1, 1, 1, 255), (3, 5, 3, 2, 2, 255),
             (70, 2, 3, 2, 1, 255), (100, 90, 3, 2, 2, 1), (16, 16, 3, 2, 2, 65535), (40, 40, 3, 1, 1, 16)]


def test_extreme_coefficients_equal_the_restatement():
    """+-2047 times a table of 255 (and of 65535) wraps the 32-bit IDCT and reaches the wrap of the range table; the device and
    the restatement wrap alike.  Both stages are compared: the sample planes, then the pixels."""
    made = [synthetic(50 + i, *spec) for i, spec in enumerate(SYNTHETIC)]
    dec = decoder()
    batch = dec.prepare([m[0] for m in made])
    outs = dec.run(batch)
    torch.cuda.synchronize()
    planes = batch.planes.cpu().numpy()
    table = batch.packed[:batch.table_bytes].cpu().numpy().view(np.int64).reshape(len(made), jpeg.FIELDS)
    wrapped = False
    for i, ((e, header, coef), out) in enumerate(zip(made, outs)):
        want_planes = [jpeg_ref.idct(coef[c], header["qtables"][c]) for c in range(e.components)]
        at = int(table[i, jpeg._F["PLANES"]])
        for c, want in enumerate(want_planes):
            got = planes[at:at + want.size].reshape(want.shape)
            assert np.array_equal(got, want), (SYNTHETIC[i], "plane", c)
            at += want.size
        want = jpeg_ref.planes_to_rgb(want_planes, e.width, e.height, e.hs, e.vs)
        assert torch.equal(out.cpu(), torch.from_numpy(want)), SYNTHETIC[i]
        # the wrap, not the clamp: a sample that a clamp alone would have put elsewhere.  Shown on DC-only blocks of the table of 16,
        # which stay inside 32 bits: such a block is flat at DESCALE(16 dc, 3) before the range table
        if int(header["qtables"][0][0]) != 16:
            continue
        x = coef[0].astype(np.int64) * 16
        dc_only = (np.abs(coef[0]).reshape(coef[0].shape[:2] + (64,))[:, :, 1:] == 0).all(axis=2)
        level = (x[:, :, 0, 0] + 4) >> 3
        far = dc_only & (np.abs(level) > 512 + 128)
        if far.any():
            flat = want_planes[0].reshape(coef[0].shape[0], 8, coef[0].shape[1], 8)[:, 0, :, 0]
            clamped = np.clip(level + 128, 0, 255)
            wrapped = wrapped or bool((flat[far] != clamped[far]).any())
    assert wrapped, "no block of the synthetic set reached the wrap of the range table"


def test_identical_calls_give_identical_bits():
    small = [data(named(p)) for p in ("37x53_420", "33x31_444", "48x64_422", "33x31_gray")]
    a = [o.clone() for o in decoder()(small)]
    big = decoder()([data(n) for n in names() if n.startswith("150x210")] + small[::-1])  # a larger call in between: another workspace
    b = decoder()(small)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a[::-1], big[-4:]):
        assert torch.equal(x, y)
    for n, out in zip([n for n in names() if n.startswith("150x210")], big):
        check(out, n)


def test_mixed_item_kinds_in_one_batch():
    n0, n1, n2 = named("37x53_420"), named("17x4_422"), named("48x64_444")
    raw = image_ref.random_image(7, 19, 23)
    tensor = torch.from_numpy(image_ref.random_image(8, 5, 9))
    outs = decoder()([raw, jpeg.entropy_decode(data(n0)), data(n1), tensor, np.frombuffer(data(n2), dtype=np.uint8), raw[:, ::-1]])
    assert torch.equal(outs[0].cpu(), torch.from_numpy(raw)) and torch.equal(outs[3].cpu(), tensor)
    assert torch.equal(outs[5].cpu(), torch.from_numpy(raw[:, ::-1].copy()))
    check(outs[1], n0)
    check(outs[2], n1)
    check(outs[4], n2)
    only_raw = decoder()([raw, tensor])  # nothing to decode: no launch, the images are copied through
    assert torch.equal(only_raw[0].cpu(), torch.from_numpy(raw)) and torch.equal(only_raw[1].cpu(), tensor)


def test_single_thread_and_pool_agree():
    ns = [n for n in names() if n.startswith(("48x64", "37x53", "2x70"))]
    one, many = jpeg.JpegDecoder(workers=1), jpeg.JpegDecoder(workers=16)
    for x, y, n in zip(one([data(n) for n in ns]), many([data(n) for n in ns]), ns):
        assert torch.equal(x, y)
        check(x, n)


PIPELINE_NAMES = ("150x210_420", "37x53_422", "33x31_gray", "1x1_444", "48x64_420")


@functools.lru_cache(maxsize=None)
def pipeline_reference():
    """image_ref's resize + normalise of the recorded pixels (computed once, shared)"""
    return torch.stack([image_ref.to_tensor_normalize(image_ref.resize(golden()["pix_" + named(p)], 32, 32)) for p in PIPELINE_NAMES])


def test_image_pipeline_on_the_decoded_images():
    items = [data(named(p)) for p in PIPELINE_NAMES]
    x = preprocess.ImagePipeline(32)(decoder()(items))
    assert x.shape == (len(items), 3, 32, 32) and torch.equal(x.cpu(), pipeline_reference())


def test_raw_jpeg_batch_to_device():
    samples = [(jpeg.read(data(named(p))), f"caption {i}", i) for i, p in enumerate(PIPELINE_NAMES)]
    image, caption, idx = jpeg.collate(samples, then=functools.partial(preprocess.ImagePipeline, 32))
    x = image.to(torch.device("cuda"), non_blocking=True)
    assert torch.equal(x.cpu(), pipeline_reference()) and idx.tolist() == list(range(len(PIPELINE_NAMES)))
    again = jpeg.RawJpegBatch([s[0] for s in samples], preprocess.ImagePipeline(32)).cuda()  # an instance instead of a factory
    assert torch.equal(again.cpu(), pipeline_reference())


def test_a_refused_item_raises_before_any_launch(monkeypatch):
    good = data(named("16x16_444"))
    sof = good.index(b"\xff\xc0")
    progressive = good[:sof + 1] + b"\xc2" + good[sof + 2:]
    sos = good.index(b"\xff\xda")
    n = (good[sos + 2] << 8 | good[sos + 3]) + 2
    second_scan = good[:-2] + good[sos:sos + n] + good[-8:]  # refused only behind the first scan, by the entropy decoder
    launched = []
    real = jpeg.JpegDecoder.launches
    monkeypatch.setattr(jpeg.JpegDecoder, "launches", lambda self, batch: launched.append(1) or real(self, batch))
    dec = jpeg.JpegDecoder()
    for bad, message in ((progressive, "progressive"), (second_scan, "more than one scan")):
        with pytest.raises(jpeg.UnsupportedJpeg, match="image 2.*" + message):
            dec([good, good, bad, good])
    with pytest.raises(jpeg.CorruptJpeg, match="image 1"):
        dec([good, good[:-20]])
    assert not launched
    (out,) = dec([good])  # and the decoder goes on
    check(out, named("16x16_444"))
    assert launched == [1]


def test_non_default_stream_and_alternating_staging():
    dec = jpeg.JpegDecoder()
    batches = [["37x53_420", "8x9_444"], ["150x210_422"], ["5x3_420", "3x5_422", "16x16_420"], ["48x64_422"], ["33x31_gray"]]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        outs = [dec([data(named(p)) for p in b]) for b in batches]  # back to back: a buffer is rewritten only after its copy
    stream.synchronize()
    for b, out in zip(batches, outs):
        for p, o in zip(b, out):
            check(o, named(p))
