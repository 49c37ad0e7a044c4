"""The PNG decode on the GPU (madtp_amd/png.py, csrc/png.hip): pixels of both routes against the recorded Pillow bytes
(tests/golden/png_pil.npz), the filtered scanlines the device route leaves against zlib.decompress, its status words against the host
emulation of the same routines (madtp_png_inflate_host, itself held against zlib in test_png_cpu.py).  Every compare is exact.
Nothing is fuzzed here: only streams the emulation has already decoded - to bytes or to a code - go to the device."""
import functools
import zlib

import numpy as np
import pytest
import torch

from madtp_amd import png, preprocess
from tests import png_ref

pytestmark = pytest.mark.gpu

CORPUS = png_ref.corpus()
NAMES = sorted(CORPUS)


def pixels(name):
    return torch.from_numpy(CORPUS[name][1])


@functools.lru_cache(maxsize=None)
def decoder(route):
    return png.PngDecoder(inflate=route)


@functools.lru_cache(maxsize=None)
def emulated(name):
    """(code, scanlines, status) of the host emulation (computed once, shared)"""
    im = png.prepare(CORPUS[name][0])
    return png.inflate_host(im.stream, im.raw_bytes, im.rowbytes)


def decode_and_check(names, route):
    dec = decoder(route)
    batch = dec.prepare([CORPUS[n][0] for n in names])
    outs = dec.run(batch)
    lines = dec.scanlines(batch)
    assert len(outs) == len(lines) == len(names)
    base = outs[0].untyped_storage().data_ptr()
    for i, n in enumerate(names):
        want = pixels(n)
        assert outs[i].is_cuda and outs[i].dtype == torch.uint8 and outs[i].shape == want.shape and outs[i].is_contiguous()
        assert outs[i].untyped_storage().data_ptr() == base  # views of one packed buffer
        assert torch.equal(outs[i].cpu(), want), f"{n} ({route}): not Pillow's pixels"
        assert lines[i].cpu().numpy().tobytes() == zlib.decompress(png_ref.parse(CORPUS[n][0])["stream"]), f"{n} ({route}): not zlib's bytes"
        if route == "device":
            rc, _, status = emulated(n)
            assert rc == 0 and np.array_equal(dec.last_status[i], status), (n, dec.last_status[i], status)
    return outs


@pytest.mark.parametrize("route", ["host", "device"])
def test_whole_corpus_as_one_mixed_batch(route):
    assert len(NAMES) == 62
    decode_and_check(NAMES, route)


@pytest.mark.parametrize("route", ["host", "device"])
def test_batches_of_one(route):
    for n in ["s1x1", "s1x70", "s300x1", "h65", "w129", "gray_w385", "pal1_w13", "rgba16_tile", "far_32768", "z_stored", "cross_repeat",
              "mid_150x210"]:
        decode_and_check([n], route)


@pytest.mark.parametrize("route", ["host", "device"])
def test_identical_calls_give_identical_bits(route):
    names = NAMES[::3]
    items = [CORPUS[n][0] for n in names]
    dec = decoder(route)
    a = dec.prepare(items)
    first = [o.clone() for o in dec.run(a)]  # (the images and the scanlines, not the padding between them: it is never written)
    first_lines = [s.clone() for s in dec.scanlines(a)]
    status = None if route == "host" else dec.last_status.copy()
    for _ in range(2):
        b = dec.prepare(items)
        again = dec.run(b)
        assert all(torch.equal(x, y) for x, y in zip(again, first))
        assert all(torch.equal(x, y) for x, y in zip(dec.scanlines(b), first_lines))
        assert route == "host" or np.array_equal(dec.last_status, status)


def test_non_default_stream_with_alternating_staging_buffers():
    stream = torch.cuda.Stream()
    groups = [NAMES[0:9], NAMES[9:14], NAMES[14:30], NAMES[30:33]]
    for route in ("host", "device"):
        dec = png.PngDecoder(workers=2, inflate=route)
        with torch.cuda.stream(stream):
            outs = [dec([CORPUS[n][0] for n in g]) for g in groups]  # four batches in flight: each staging buffer is used twice
        stream.synchronize()
        for g, out in zip(groups, outs):
            for n, o in zip(g, out):
                assert torch.equal(o.cpu(), pixels(n)), (n, route)


@pytest.mark.parametrize("route", ["host", "device"])
def test_raw_images_pass_through_next_to_files(route):
    raw = torch.arange(5 * 7 * 3, dtype=torch.uint8).view(5, 7, 3)
    arr = (np.arange(3 * 2 * 3, dtype=np.uint8) * 9).reshape(3, 2, 3)
    outs = decoder(route)([CORPUS["rgb8"][0], raw, png.read(CORPUS["pal2_w7"][0]), arr])
    assert torch.equal(outs[0].cpu(), pixels("rgb8")) and torch.equal(outs[1].cpu(), raw)
    assert torch.equal(outs[2].cpu(), pixels("pal2_w7")) and np.array_equal(outs[3].cpu().numpy(), arr)
    only = decoder(route)([raw])
    assert torch.equal(only[0].cpu(), raw)


def _corrupt_files():
    """a corpus file with its stream damaged: {case: (file bytes, the code the emulation gives)}; the chunks stay whole"""
    data = CORPUS["filter_heur"][0]
    p = png_ref.parse(data)
    raw = bytearray(zlib.decompress(p["stream"]))
    stream = p["stream"]
    head = png_ref.ihdr(p["width"], p["height"], p["depth"], p["color"])
    flipped = bytearray(stream)
    flipped[len(stream) // 2] ^= 0x10
    raw[1 + p["rowbytes"]] = 7
    cases = {"flipped": bytes(flipped), "short": stream[:-6], "adler": stream[:-1] + bytes([stream[-1] ^ 1]),
             "long": zlib.compress(bytes(raw[:-1]) + b"\x00\x00"), "filter": zlib.compress(bytes(raw)),
             "far": png_ref.BitWriter().bits(1, 1).bits(1, 2).fixed(0).fixed(257).code(1, 5).fixed(256).done()}
    out = {}
    for case, s in cases.items():
        rc, _, status = png.inflate_host(s, p["raw_bytes"], p["rowbytes"])
        assert -300 < rc <= -200, case  # only what the emulation has decoded to a code goes to the device
        out[case] = (png_ref.build(head, png_ref.chunk(b"IDAT", s)), rc, status)
    return out


@pytest.mark.parametrize("route", ["host", "device"])
def test_a_corrupt_file_raises_naming_the_image_and_returns_nothing(route):
    good = [CORPUS["rgb8"][0], CORPUS["gray4_w5"][0]]
    dec = decoder(route)
    for case, (data, code, status) in _corrupt_files().items():
        out = None
        with pytest.raises(png.CorruptPng, match=r"image 1: ") as e:
            out = dec([good[0], data, good[1]])
        assert out is None, case
        if route == "device":
            assert f"code {code}" in str(e.value), case
            assert np.array_equal(dec.last_status[1], status), (case, dec.last_status[1], status)
            assert dec.last_status[0][0] == 0 and dec.last_status[2][0] == 0  # the neighbours decoded
    outs = dec(good)  # and the decoder goes on
    assert torch.equal(outs[0].cpu(), pixels("rgb8")) and torch.equal(outs[1].cpu(), pixels("gray4_w5"))


def test_image_pipeline_on_the_result_equals_the_pipeline_on_pillows_arrays():
    names = NAMES[::6] + ["mid_150x210"]
    items = [CORPUS[n][0] for n in names]
    pipe = preprocess.ImagePipeline(384, "stretch")
    want = pipe([CORPUS[n][1] for n in names])
    for route in ("host", "device"):
        got = pipe(decoder(route)(items))
        assert got.shape == (len(items), 3, 384, 384) and torch.equal(got, want), route
    then = functools.partial(preprocess.ImagePipeline, 384)
    batch = png.collate([(png.read(d), i) for i, d in enumerate(items)], then=then)
    assert torch.equal(batch[0].to("cuda", non_blocking=True), want) and batch[1].tolist() == list(range(len(items)))
