"""The device Huffman stage on the GPU (madtp_amd/jpeg_device.py, csrc/jpeg_huff.hip): coefficients against the host decoder's
(jpeg.entropy_decode), status words against the host emulation of the same passes (madtp_jhuff_decode_host, itself held against the
host decoder in test_jpeg_device_cpu.py), pixels against the recorded Pillow bytes (tests/golden/jpeg_pil.npz).  Every compare is
exact.  Nothing is fuzzed here: only streams the emulation has already decoded - to coefficients or to a code - go to the device."""
import functools
import re

import numpy as np
import pytest
import torch

from madtp_amd import jpeg, jpeg_device, preprocess
from tests.jpeg_device_cases import data, golden, guarded_lanes, guesses_part, host_coefficients, malformed, names, truncations

pytestmark = pytest.mark.gpu


def pixels(name):
    return torch.from_numpy(golden()["pix_" + name])


def named(prefix):
    return next(n for n in names() if n.startswith(prefix))


@functools.lru_cache(maxsize=None)
def decoder(subseq=None):
    return jpeg_device.DeviceJpegDecoder(subseq_bytes=subseq)


@functools.lru_cache(maxsize=None)
def emulated(name, subseq):
    """(code, coefficients, status) of the host emulation (computed once, shared)"""
    return guarded_lanes(data(name), subseq or 0)


def decode_and_check(ns, subseq):
    dec = decoder(subseq)
    batch = dec.prepare([data(n) for n in ns])
    outs = dec.run(batch)
    coefs = dec.coefficients(batch)
    assert len(outs) == len(coefs) == len(ns) and dec.last_status.shape == (len(ns), 4)
    base = outs[0].untyped_storage().data_ptr()
    for i, n in enumerate(ns):
        rc, _, status = emulated(n, subseq)
        assert rc == 0 and np.array_equal(dec.last_status[i], status), (n, dec.last_status[i], status)
        assert np.array_equal(coefs[i].cpu().numpy(), host_coefficients(n)), f"{n}: not the host decoder's coefficients"
        want = pixels(n)
        assert outs[i].is_cuda and outs[i].dtype == torch.uint8 and outs[i].shape == want.shape
        assert outs[i].untyped_storage().data_ptr() == base  # views of one packed buffer
        assert torch.equal(outs[i].cpu(), want), f"{n}: not Pillow's pixels"
    return outs


@pytest.mark.parametrize("subseq", (None, 4))
def test_whole_corpus_as_one_mixed_batch(subseq):
    assert len(names()) == 42
    decode_and_check(names(), subseq)


@pytest.mark.parametrize("prefix", ["1x1_444", "1x1_420", "8x9_420", "33x31_gray", "37x53_420_q85_restart", "150x210"])
def test_batches_of_one(prefix):
    for subseq in (None, 4):
        decode_and_check([named(prefix)], subseq)


def test_identical_calls_give_identical_bits():
    ns = names()[::3]
    items = [data(n) for n in ns]
    for subseq in (None, 4):
        dec = decoder(subseq)
        a = dec.prepare(items)
        first = [o.clone() for o in dec.run(a)]  # (the images and the coefficients, not the padding between them: it is never written)
        first_coef = [c.clone() for c in dec.coefficients(a)]
        status = dec.last_status.copy()
        for _ in range(2):
            b = dec.prepare(items)
            again = dec.run(b)
            assert all(torch.equal(x, y) for x, y in zip(again, first)) and np.array_equal(dec.last_status, status)
            assert all(torch.equal(x, y) for x, y in zip(dec.coefficients(b), first_coef))


def test_non_default_stream_with_alternating_staging_buffers():
    dec = jpeg_device.DeviceJpegDecoder(workers=2)
    stream = torch.cuda.Stream()
    groups = [names()[0:9], names()[9:14], names()[14:30], names()[30:33]]
    with torch.cuda.stream(stream):
        outs = [dec([data(n) for n in g]) for g in groups]  # four batches in flight: each staging buffer is used twice
    stream.synchronize()
    for g, out in zip(groups, outs):
        for n, o in zip(g, out):
            assert torch.equal(o.cpu(), pixels(n)), n


def test_raw_images_pass_through_next_to_files():
    raw = torch.arange(5 * 7 * 3, dtype=torch.uint8).view(5, 7, 3)
    ns = [named("16x16_420"), named("33x31_gray")]
    outs = decoder()([data(ns[0]), raw, jpeg_device.read(data(ns[1]))])
    assert torch.equal(outs[0].cpu(), pixels(ns[0])) and torch.equal(outs[1].cpu(), raw) and torch.equal(outs[2].cpu(), pixels(ns[1]))


def _bad_streams():
    return {**malformed(), **truncations()}


@pytest.mark.parametrize("subseq", (None, 4))
def test_malformed_streams_raise_naming_the_image_and_return_nothing(subseq):
    good = [data(named("16x16_420")), data(named("33x31_gray"))]
    dec = decoder(subseq)
    for case, (raw, message) in _bad_streams().items():
        want, _, status = guarded_lanes(raw, subseq or 0)  # only what the emulation has decoded to a code goes to the device
        assert -300 < want <= -200, case
        out = None
        with pytest.raises(jpeg.CorruptJpeg, match=r"image 1: .*" + re.escape(message)) as e:
            out = dec([good[0], raw, good[1]])
        assert out is None and f"code {want}" in str(e.value), case
        assert np.array_equal(dec.last_status[1], status), case
        assert dec.last_status[0][0] == 0 and dec.last_status[2][0] == 0  # the neighbours decoded
    with pytest.raises(jpeg.CorruptJpeg, match="image 2"):  # the first one in the batch is named
        bad = list(_bad_streams().values())
        dec([good[0], good[1], bad[0][0], bad[3][0]])
    outs = dec(good)  # and the decoder goes on
    assert torch.equal(outs[0].cpu(), pixels(named("16x16_420")))


def test_a_file_the_guesses_get_wrong_goes_to_the_serial_lane():
    raw = guesses_part()
    rc, coef, status = guarded_lanes(raw, 4)
    assert rc == 0 and status[jpeg_device._S["SERIAL"]] == 1
    dec = decoder(4)
    batch = dec.prepare([raw, data(named("8x9_420"))])
    outs = dec.run(batch)
    assert np.array_equal(dec.last_status[0], status)
    assert np.array_equal(dec.coefficients(batch)[0].cpu().numpy().reshape(-1), coef)
    assert torch.equal(outs[1].cpu(), pixels(named("8x9_420")))
    assert torch.equal(outs[0].cpu(), jpeg.JpegDecoder()([raw])[0].cpu())


def test_image_pipeline_on_the_result_equals_the_host_route():
    items = [data(n) for n in names()[::2]]
    pipe = preprocess.ImagePipeline(32)
    got = pipe(decoder()(items))
    want = pipe(jpeg.JpegDecoder()(items))
    assert got.shape == (len(items), 3, 32, 32) and torch.equal(got, want)
    then = functools.partial(preprocess.ImagePipeline, 32)
    batch = jpeg_device.collate([jpeg_device.read(d) for d in items], then=then)
    assert torch.equal(batch.to("cuda", non_blocking=True), want)
