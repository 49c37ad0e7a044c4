"""CPU side of the image pipeline (madtp_amd/preprocess.py, include/madtp_image.h): the host-made coefficient tables against
Pillow (live where it imports, and always against the recorded tests/golden/imgprep_pil.npz), the normalisation table, the
refusals that need no GPU and the exported symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from madtp_amd import abi, hip, preprocess
from tests import image_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "imgprep_pil.npz")

# one axis, in -> out: ratios below 1, equal to 1, in (1, 2) and above 2, non-integer ratios, in == 1
PAIRS = [(1, 1), (1, 5), (1, 32), (2, 1), (2, 7), (3, 3), (3, 10), (5, 2), (7, 7), (7, 8), (7, 13), (8, 7), (9, 4), (10, 3), (11, 32),
         (13, 40), (16, 16), (16, 32), (17, 5), (19, 96), (23, 7), (31, 32), (32, 31), (33, 32), (37, 11), (40, 32), (41, 40), (47, 32),
         (50, 33), (63, 32), (64, 32), (65, 32), (70, 9), (81, 40), (96, 32), (97, 40), (100, 7), (127, 96), (128, 5), (131, 40),
         (150, 32), (190, 96), (200, 13), (250, 40), (257, 17), (300, 96), (640, 384), (500, 40), (1024, 64)]


def apply_tables(img, axis, out_size, box=None):
    """one pass of preprocess.resample_tables' arrays over `axis` of a uint8 [h, w, 3] array, with image_ref's integer arithmetic"""
    k, bounds = preprocess.resample_tables(img.shape[axis], out_size, box)
    assert k.dtype == np.int32 and bounds.dtype == np.int32 and k.shape[0] == out_size and bounds.shape == (out_size, 2)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        assert not k[xx, n:].any()
        acc = (1 << 21) + (src[xmin:xmin + n] * k[xx, :n].reshape(-1, 1, 1)).sum(axis=0, dtype=np.int32)
        out[xx] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def table_resize(img, W, H):
    return apply_tables(apply_tables(img, 1, W), 0, H)


def test_pairs_cover_what_the_issue_asks():
    ratios = [n / m for n, m in PAIRS]
    assert len(PAIRS) >= 40 and any(r < 1 for r in ratios) and any(r == 1 for r in ratios) and any(1 < r < 2 for r in ratios)
    assert any(r > 2 for r in ratios) and any(r != int(r) for r in ratios) and any(n == 1 for n, _ in PAIRS)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_tables_equal_live_pillow(pair):
    Image = pytest.importorskip("PIL.Image")
    n, m = pair
    img = image_ref.random_image(n * 1000 + m, 3, n)
    img[0] = (np.arange(n) % 2 * 255).astype(np.uint8)[:, None]  # a 0 / 255 row: both clamps
    want = np.asarray(Image.fromarray(img, "RGB").resize((m, 3), Image.BICUBIC))
    assert np.array_equal(apply_tables(img, 1, m), want)
    assert np.array_equal(image_ref.resample_axis(img, 1, m), want)
    # the same pair down the other axis, and through both passes
    want_t = np.asarray(Image.fromarray(np.ascontiguousarray(img.transpose(1, 0, 2)), "RGB").resize((3, m), Image.BICUBIC))
    assert np.array_equal(apply_tables(np.ascontiguousarray(img.transpose(1, 0, 2)), 0, m), want_t)


def test_two_pass_resize_crop_and_box_equal_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    img = image_ref.random_image(77, 131, 97)
    img[40:90, 20:70] = image_ref.checkerboard(50, 50)
    pil = Image.fromarray(img, "RGB")
    for W, H in ((32, 32), (40, 96), (200, 150), (97, 40)):
        want = np.asarray(pil.resize((W, H), Image.BICUBIC))
        assert np.array_equal(table_resize(img, W, H), want) and np.array_equal(image_ref.resize(img, W, H), want)
    box = (5, 7, 90, 100)
    want = np.asarray(pil.crop(box).resize((40, 32), Image.BICUBIC))
    assert np.array_equal(table_resize(img[7:100, 5:90], 40, 32), want)
    # Image.resize(box=...) reads the pixels around the box: resample_tables' box argument
    want = np.asarray(pil.resize((40, 32), Image.BICUBIC, box=(5.5, 7.25, 90.0, 100.5)))
    got = apply_tables(apply_tables(img, 1, 40, (5.5, 90.0)), 0, 32, (7.25, 100.5))
    assert np.array_equal(got, want)
    assert np.array_equal(image_ref.short_side_crop(img, 40), np.asarray(pil.resize((40, 54), Image.BICUBIC).crop((0, 7, 40, 47))))


def _golden():
    return np.load(GOLDEN)


def test_tables_equal_recorded_pillow():
    g = _golden()
    assert os.path.getsize(GOLDEN) <= 300_000 and str(g["pillow_version"])
    seen = 0
    for key in g.files:
        parts = key.split("_")
        if parts[0] == "sweep" and parts[1] != "in":
            n, m = int(parts[1]), int(parts[2])
            img = g[f"sweep_in_{n}"]
            assert np.array_equal(apply_tables(img, 1, m), g[key]), key
            assert np.array_equal(image_ref.resample_axis(img, 1, m), g[key]), key
        elif parts[0] in ("resize", "flip"):
            W, H = map(int, parts[-1].split("x"))
            img = g["in_" + "_".join(parts[1:-1])]
            got = table_resize(img, W, H)
            assert np.array_equal(got[:, ::-1] if parts[0] == "flip" else got, g[key]), key
            assert np.array_equal(image_ref.resize(img, W, H), g["resize_" + "_".join(parts[1:])]), key
        elif parts[0] == "crop":
            W, H = map(int, parts[-1].split("x"))
            l, u, r, d = map(int, parts[-5:-1])
            img = g["in_" + "_".join(parts[1:-5])]
            assert np.array_equal(table_resize(img[u:d, l:r], W, H), g[key]), key
        elif parts[0] == "ssc":
            S = int(parts[-1])
            img = g["in_" + "_".join(parts[1:-1])]
            h, w = img.shape[:2]
            nw, nh, left, top = preprocess.short_side_geometry(w, h, S)
            assert np.array_equal(table_resize(img, nw, nh)[top:top + S, left:left + S], g[key]), key
            assert np.array_equal(image_ref.short_side_crop(img, S), g[key]), key
        else:
            continue
        seen += 1
    assert seen >= 80


def test_tables_are_cached_and_read_only():
    a = preprocess.resample_tables(250, 96)
    assert preprocess.resample_tables(250, 96)[0] is a[0] and preprocess.resample_tables(250, 96, (0.0, 250.0))[0] is not a[0]
    assert np.array_equal(preprocess.resample_tables(250, 96, (0.0, 250.0))[0], a[0])
    with pytest.raises(ValueError):
        a[0][0, 0] = 1
    assert a[0].shape[1] == 2 * int(np.ceil(2.0 * 250 / 96)) + 1
    with pytest.raises(ValueError):
        preprocess.resample_tables(0, 4)


def test_normalize_table_is_totensor_plus_normalize():
    for mean, std in ((preprocess.MEAN, preprocess.STD), ((0.5, 0.25, 0.125), (0.5, 0.3, 0.7))):
        table = preprocess.normalize_table(mean, std)
        assert table.shape == (3, 256) and table.dtype == torch.float32
        img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
        want = image_ref.to_tensor_normalize(img, mean, std)
        got = torch.stack([table[c][torch.from_numpy(img[:, :, c].astype(np.int64))] for c in range(3)])
        assert torch.equal(got, want)
    assert preprocess.MEAN == (0.48145466, 0.4578275, 0.40821073) and preprocess.STD == (0.26862954, 0.26130258, 0.27577711)


def test_short_side_geometry():
    assert preprocess.short_side_geometry(500, 375, 336) == (448, 336, 56, 0)
    assert preprocess.short_side_geometry(375, 500, 336) == (336, 448, 0, 56)
    assert preprocess.short_side_geometry(97, 131, 40) == (40, 54, 0, 7) and preprocess.short_side_geometry(40, 40, 40) == (40, 40, 0, 0)


def test_entry_point_refuses_before_any_launch():
    lib = preprocess.lib()
    E_BADARG, E_SHAPE = abi.DEFINES["MADTP_E_BADARG"], abi.DEFINES["MADTP_E_SHAPE"]
    ok = dict(src=16, table=16, lut=16, out=16, B=1, Sh=32, Sw=32, n_blocks=1, max_ksize=5)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.madtp_image_resize_batch(a["src"], a["table"], a["lut"], a["out"], a["B"], a["Sh"], a["Sw"], a["n_blocks"],
                                            a["max_ksize"], 0)
    for name in ("src", "table", "lut", "out"):
        assert call(**{name: 0}) == E_BADARG, name
    assert call(B=0) == E_BADARG and call(B=-3) == E_BADARG and call(n_blocks=0) == E_BADARG
    assert call(Sh=0) == E_SHAPE and call(Sw=0) == E_SHAPE and call(Sw=-1) == E_SHAPE
    assert call(max_ksize=preprocess.MAX_KSIZE + 2) == E_SHAPE and call(max_ksize=0) == E_SHAPE  # a ratio beyond 16
    assert lib.madtp_strerror(E_SHAPE) == b"unsupported shape"
    # the planner: tile heights whose source rows fit the LDS rows, workgroups per image
    rows = preprocess.DEFINES["MADTP_IMAGE_LDS_ROWS"]
    assert lib.madtp_image_tile_rows(1.25, 7) == 32 and lib.madtp_image_tile_rows(0.1, 5) == 32
    assert lib.madtp_image_tile_rows(16.0, 65) == 4 and lib.madtp_image_tile_rows(16.0, 67) == 0 and lib.madtp_image_tile_rows(0.0, 5) == 0
    for ratio, ksize in ((1.0, 5), (2.6, 13), (5.0, 21), (9.5, 39), (16.0, 65)):
        t = lib.madtp_image_tile_rows(ratio, ksize)
        assert t >= 1 and (t - 1) * ratio + ksize <= rows and (t == 32 or (2 * t - 1) * ratio + ksize > rows)
    assert lib.madtp_image_blocks(96, 96, 32) == 6 and lib.madtp_image_blocks(40, 65, 32) == 4 and lib.madtp_image_blocks(0, 8, 8) == 0


def test_tile_rule_bounds_the_rows_of_every_tile():
    """the planner's bound (T - 1) * ratio + ksize against the exact row span of every tile, from the tables themselves"""
    lib = preprocess.lib()
    rows = preprocess.DEFINES["MADTP_IMAGE_LDS_ROWS"]
    for n, m in PAIRS + [(8192, 512), (4000, 251), (512, 32), (639, 40)]:
        k, bounds = preprocess.resample_tables(n, m)
        t = lib.madtp_image_tile_rows(n / m, k.shape[1])
        assert (t >= 1) == (k.shape[1] <= preprocess.MAX_KSIZE)
        if t < 1:
            continue
        for y0 in range(0, m, t):
            y1 = min(y0 + t, m) - 1
            assert 0 < bounds[y1, 0] + bounds[y1, 1] - bounds[y0, 0] <= rows
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(axis=1)) >= 0).all() and bounds.sum(axis=1).max() <= n


def test_pipeline_refuses_unsupported_images():
    pipe = preprocess.ImagePipeline(32)
    good = image_ref.random_image(1, 20, 30)
    with pytest.raises(ValueError, match="image 1.*float32"):
        pipe([good, good.astype(np.float32)])
    with pytest.raises(ValueError, match="image 0.*float32"):
        pipe([torch.zeros(8, 8, 3)])
    with pytest.raises(ValueError, match=r"image 1.*\(20, 30, 4\)"):
        pipe([good, np.zeros((20, 30, 4), dtype=np.uint8)])
    with pytest.raises(ValueError, match="image 0"):
        pipe([np.zeros((20, 30), dtype=np.uint8)])
    with pytest.raises(ValueError, match="image 2.*ratio"):
        pipe([good, good, np.zeros((8, 32 * 16 + 40, 3), dtype=np.uint8)])
    with pytest.raises(ValueError, match="image 0.*crop box"):
        pipe([good], boxes=[(0, 0, 31, 20)])
    with pytest.raises(ValueError):
        preprocess.ImagePipeline(32, mode="letterbox")
    with pytest.raises(ValueError):
        preprocess.ImagePipeline((32, 40), mode="short_side_crop")


def test_pipeline_needs_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    good = image_ref.random_image(1, 20, 30)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        preprocess.ImagePipeline(32)([good])
    batch = preprocess.collate([torch.from_numpy(good)], size=32)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        batch.to("cuda", non_blocking=True)


def test_cpu_device_is_refused_everywhere():
    good = image_ref.random_image(1, 20, 30)
    with pytest.raises(RuntimeError, match="no CPU / eager fallback"):
        preprocess.ImagePipeline(32, device="cpu")([good])


def test_collate_keeps_raw_images():
    a, b = torch.from_numpy(image_ref.random_image(1, 20, 30)), torch.from_numpy(image_ref.random_image(2, 9, 50))
    batch = preprocess.collate([a, b], size=32)
    assert isinstance(batch, preprocess.RawImageBatch) and len(batch) == 2 and batch.images[1] is b and batch.size == 32
    image, caption, idx = preprocess.collate([(a, "one", 3), (b, "two", 5)], size=(32, 40), mode="stretch")
    assert isinstance(image, preprocess.RawImageBatch) and caption == ["one", "two"] and torch.equal(idx, torch.tensor([3, 5]))
    Image = pytest.importorskip("PIL.Image")
    raw = preprocess.raw_image(Image.fromarray(a.numpy(), "RGB").convert("L"))
    assert raw.dtype == torch.uint8 and raw.shape == (20, 30, 3)
    assert torch.equal(preprocess.raw_image(Image.fromarray(a.numpy(), "RGB")), a)


def _image_header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "madtp_image.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))


def test_image_symbols_are_exported_and_the_model_abi_is_unchanged():
    from madtp_amd import build
    raw = ctypes.CDLL(build.build(verbose=False))
    syms = _image_header_symbols()
    assert syms == sorted(preprocess.SIGNATURES) and "madtp_image_resize_batch" in syms and "madtp_image_abi_version" in syms
    assert all(s.startswith("madtp_image_") for s in syms)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/madtp_image.h but not exported"
    lib = preprocess.lib()
    assert lib.madtp_image_abi_version() == preprocess.ABI_VERSION == 1
    for name, (res, args) in preprocess.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    assert preprocess.SIGNATURES["madtp_image_resize_batch"] == (c_int, [c_void_p] * 4 + [c_int] * 5 + [c_void_p])
    assert len(abi.SIGNATURES) == 97 and not set(abi.SIGNATURES) & set(syms) and hip.ABI_VERSION == 31
    assert preprocess.FIELDS == 16 and sorted(preprocess._F.values()) == list(range(13))
