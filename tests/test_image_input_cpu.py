"""What the image input path shares on the host, without a GPU: the binder of the side headers (madtp_amd/abi.py), the staging ring
and the pool (madtp_amd/staging.py), and the layout of a JPEG batch for both decoders (jpeg.plan_batch).  Whether the planned
layout decodes to the right pixels is the GPU tests' matter (test_jpeg_gpu.py, test_jpeg_device_gpu.py)."""
import functools
import threading

import numpy as np
import pytest
import torch

from madtp_amd import abi, hip, jpeg, jpeg_device, preprocess, staging
from tests.jpeg_device_cases import by_prefix

CODED = ("1x1_444", "1x1_420", "8x9_420", "17x4_422", "33x31_gray", "37x53_420_q85_restart")
RAW = ((1, 1, 3), (5, 4, 3))
ROUTES = ("host", "device")


# ---- the binder ------------------------------------------------------------------------------------------------------------------------
def test_binding_twice_gives_the_one_handle_from_any_thread():
    handles = [m.lib() for m in (preprocess, jpeg, jpeg_device, preprocess, jpeg_device)]
    assert all(h is hip.load() for h in handles)
    again = abi.binder(jpeg.SIGNATURES, jpeg.DEFINES, "madtp_jpeg_abi_version")  # a fresh one, first called from threads
    got = []
    threads = [threading.Thread(target=lambda: got.append(again())) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(got) == 8 and all(h is hip.load() for h in got)
    # a module that needs another's entry points binds them too; a prefix keeps a header's own family
    assert hip.load().madtp_jpeg_inspect.argtypes == jpeg.SIGNATURES["madtp_jpeg_inspect"][1]
    assert jpeg_device.SIGNATURES and all(k.startswith("madtp_jhuff_") for k in jpeg_device.SIGNATURES)


def test_a_header_of_another_version_asks_for_a_rebuild():
    with open(jpeg.HEADER) as f:
        text = f.read()
    assert "#define MADTP_JPEG_ABI_VERSION 1\n" in text
    sigs, _, defines = abi.parse(text.replace("#define MADTP_JPEG_ABI_VERSION 1\n", "#define MADTP_JPEG_ABI_VERSION 2\n"), "madtp_jpeg.h")
    lib = abi.binder(sigs, defines, "madtp_jpeg_abi_version")
    for _ in range(2):  # and it stays unbound
        with pytest.raises(RuntimeError, match="libmadtp_hip jpeg ABI 1 != binding 2; rebuild"):
            lib()


def test_a_parse_error_names_the_header_it_was_given():
    with pytest.raises(ValueError, match=r"^madtp_other\.h: unknown type 'long double'"):
        abi.parse("int madtp_bad(long double x, void* stream);", "madtp_other.h")
    with pytest.raises(ValueError, match=r"^madtp_other\.h: cannot split"):
        abi.parse("int madtp_bad(int);", "madtp_other.h")
    with pytest.raises(ValueError, match=r"^madtp_hip\.h: "):
        abi.parse("int madtp_bad(int);")


# ---- the staging ring and the pool -----------------------------------------------------------------------------------------------------
def test_ring_alternates_and_grows_by_the_rule():
    assert staging.grown(1) == staging.grown(1 << 20) == (1 << 20) * 5 // 4 and staging.grown(4 << 20) == 5 << 20
    assert [staging.align(n, 16) for n in (0, 1, 16, 17)] == [0, 16, 16, 32] and staging.align(257, 256) == 512
    ring = staging.StagingRing()
    assert [ring._next(10) for _ in range(4)] == [(0, 1310720), (1, 1310720), (0, 1310720), (1, 1310720)]
    ring._stage[0] = torch.empty(1000, dtype=torch.uint8)  # (pageable here: the pinned allocation is the GPU tests')
    assert ring._next(1000) == (0, 0) and ring._next(1000) == (1, 1310720)  # a buffer that holds the batch is kept
    assert ring._next(1001) == (0, 1310720) and ring._next(3 << 20) == (1, (3 << 20) * 5 // 4)


def test_pool_is_bounded_and_waits_for_every_job_before_it_raises():
    assert staging.MAX_WORKERS == jpeg.MAX_WORKERS == jpeg_device.MAX_WORKERS == 16
    assert [staging.Pool(w, "t").workers for w in (0, 1, 8, 100)] == [1, 1, 8, 16]
    pool = staging.Pool(4, "madtp-test")
    assert pool.map(lambda j: j * j, list(range(9))) == [j * j for j in range(9)] and pool._pool._max_workers == 4
    done = []

    def job(j):
        if j == 0:
            raise KeyError("job 0")
        done.append(j)

    with pytest.raises(KeyError):
        pool.map(job, list(range(8)))
    assert sorted(done) == list(range(1, 8))  # no thread is still writing when the error surfaces
    assert staging.Pool(1, "t").map(lambda j: j + 1, [1, 2]) == [2, 3] and staging.Pool(8, "t").map(lambda j: j, [5]) == [5]


# ---- the plan of a JPEG batch ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan(prefix):
    return jpeg_device.prepare_scan(by_prefix(prefix))


@functools.lru_cache(maxsize=None)
def entropy(prefix):
    return jpeg.entropy_decode(by_prefix(prefix))


def facts(kinds, route):
    """plan_batch's items for a batch of corpus prefixes and raw shapes, as the route's decoder states them"""
    out = []
    for k in kinds:
        if isinstance(k, tuple):
            out.append(("raw", k))
        elif route == "host":
            out.append(("coded", entropy(k), int(entropy(k).coef.shape[0]), None))
        else:
            s = scan(k)
            out.append(("coded", s, s.blocks, (s.data.size, s.scan_begin, s.tables.size)))
    return out


def plan(kinds, route):
    return jpeg.plan_batch(facts(kinds, route), None if route == "host" else jpeg_device._SCANS)


BATCHES = {"mixed": (RAW[0],) + CODED[:3] + (RAW[1],) + CODED[3:], "one": ("8x9_420",), "one_restart": (CODED[5],), "raw_only": RAW}


def regions(p, kinds, route):
    """-> [(name, begin, bytes, alignment, staged)] of everything that lies in the packed buffer"""
    lib, F, HF, B = jpeg.lib(), jpeg._F, jpeg_device._F, len(kinds)
    out = [("table", 0, B * 8 * jpeg.FIELDS, 16, True), ("qtables", p.qtable_at, B * 384, 16, True)]
    if route == "device":
        out.append(("htable", p.htable_at, len(p.coded) * 8 * jpeg_device.FIELDS, 8, True))
    for n, i in enumerate(p.coded):
        head = scan(kinds[i])
        coef = p.coef_at + int(p.table[i, F["COEF"]])
        assert int(p.table[i, F["COEF"]]) % 16 == 0 and int(p.table[i, F["QTABLE"]]) == 384 * i
        out.append((f"coef {i}", coef, 128 * p.blocks[n], 4, route == "host"))
        if route == "device":
            row = p.htable[n]
            assert int(row[HF["COEF"]]) == int(p.table[i, F["COEF"]]) and int(row[HF["SIZE"]]) == head.data.size
            out.append((f"record {i}", int(row[HF["RECORD"]]), jpeg_device.RECORD_BYTES, 4, True))
            out.append((f"file {i}", int(row[HF["FILE"]]), head.data.size, 16, True))
        (hh, ww), o = p.shapes[i]
        assert (hh, ww) == (head.height, head.width) and int(p.table[i, F["OUT"]]) == o - p.out_at
        out.append((f"out {i}", o, int(lib.madtp_jpeg_out_bytes(ww, hh)), 16, False))
    for i, k in enumerate(kinds):
        if isinstance(k, tuple):
            assert p.shapes[i][0] == k[:2]
            out.append((f"raw {i}", p.shapes[i][1], k[0] * k[1] * 3, 16, True))
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_regions_lie_inside_the_buffer_aligned_and_apart(batch, route):
    kinds = BATCHES[batch]
    p = plan(kinds, route)
    rs = regions(p, kinds, route)
    assert p.B == len(kinds) and p.table_bytes == p.qtable_at == 8 * jpeg.FIELDS * p.B and p.head.size == (p.htable_at if route == "host" else
                                                                                                        p.htable_at + p.htable.nbytes)
    assert p.coded == [i for i, k in enumerate(kinds) if not isinstance(k, tuple)]
    for name, at, size, a, staged in rs:
        assert at % a == 0 and 0 <= at and at + size <= p.total, name
        assert at + size <= p.copy_bytes if staged else at >= p.copy_bytes, name
    ordered = sorted(rs, key=lambda r: r[1])
    for (n0, a0, s0, _, _), (n1, a1, _, _, _) in zip(ordered, ordered[1:]):
        assert a0 + s0 <= a1, (n0, n1)
    assert p.copy_bytes == max(at + size for _, at, size, _, staged in rs if staged)  # nothing is copied that nobody reads
    assert p.out_at % 256 == 0 and p.copy_bytes <= p.out_at <= p.total and (route == "host" or p.coef_at % 256 == 0)
    # the head as it is staged: the rows, then the tables column-major
    assert np.array_equal(p.head[:p.table_bytes].view(np.int64).reshape(p.B, -1), p.table)
    q = p.head[p.qtable_at:p.htable_at].view(np.uint16).reshape(p.B, 3, 8, 8)
    for i, k in enumerate(kinds):
        want = np.zeros((3, 64), np.uint16) if isinstance(k, tuple) else scan(k).qtables
        assert np.array_equal(q[i].transpose(0, 2, 1).reshape(3, 64), want), i


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_grids_and_planes_are_the_librarys_sums(batch, route):
    kinds = BATCHES[batch]
    p = plan(kinds, route)
    lib, F = jpeg.lib(), jpeg._F
    n_idct = n_rgb = plane_sum = plane_end = 0
    for i, k in enumerate(kinds):
        row = p.table[i]
        assert (int(row[F["FIRST_IDCT"]]), int(row[F["FIRST_RGB"]])) == (n_idct, n_rgb), i  # prefix sums over every row, raw ones too
        if isinstance(k, tuple):
            continue
        s = scan(k)
        geometry = (s.components, s.hs, s.vs, s.blocks_x, s.blocks_y)
        assert p.blocks[p.coded.index(i)] == lib.madtp_jpeg_blocks(*geometry) == s.blocks
        assert tuple(int(row[F[f]]) for f in ("W", "H", "COMPONENTS", "HS", "VS", "BLOCKS_X", "BLOCKS_Y")) == (s.width, s.height) + geometry
        n_idct += lib.madtp_jpeg_idct_groups(s.blocks)
        n_rgb += lib.madtp_jpeg_rgb_groups(s.width, s.height)
        planes = int(row[F["PLANES"]])
        assert planes % 256 == 0 and planes >= plane_end
        plane_end = planes + lib.madtp_jpeg_plane_bytes(*geometry)
        plane_sum += lib.madtp_jpeg_plane_bytes(*geometry)
    assert (p.n_idct, p.n_rgb, p.plane_bytes) == (n_idct, n_rgb, plane_sum)
    assert p.workspace == lib.madtp_jpeg_workspace(p.B, plane_sum) and plane_end <= max(p.workspace, 0)
    if batch == "raw_only":
        assert (p.n_idct, p.n_rgb, p.plane_bytes, p.coded, p.blocks) == (0, 0, 0, [], [])
    if batch == "one_restart" and route == "device":
        assert int(p.htable[0, jpeg_device._F["RESTART"]]) == scan(kinds[0]).restart_interval > 0


@pytest.mark.parametrize("batch", list(BATCHES))
def test_both_routes_share_the_rows_of_the_idct_and_colour_kernels(batch):
    host, device = plan(BATCHES[batch], "host"), plan(BATCHES[batch], "device")
    assert np.array_equal(host.table, device.table) and np.array_equal(host.head, device.head[:host.head.size])
    assert (host.n_idct, host.n_rgb, host.plane_bytes, host.workspace, host.blocks) == \
        (device.n_idct, device.n_rgb, device.plane_bytes, device.workspace, device.blocks)
    assert [s for s, _ in host.shapes] == [s for s, _ in device.shapes]


class Fields:
    """an item's header with one field replaced"""

    def __init__(self, image, **changed):
        for k in ("width", "height", "components", "hs", "vs", "blocks_x", "blocks_y", "restart_interval", "qtables"):
            setattr(self, k, changed.get(k, getattr(image, k)))


@pytest.mark.parametrize("changed", [dict(width=8 * 4 + 1), dict(width=0), dict(height=8 * 5 + 1), dict(blocks_x=3), dict(components=2),
                                     dict(hs=1), dict(claimed=19), dict(claimed=-1)], ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_an_entropy_image_with_one_contradictory_field_is_refused(changed):
    e = entropy("33x31_gray")  # 33 rows of 31 pixels: 4 x 5 blocks, 20 in all
    assert (e.blocks_x, e.blocks_y, e.coef.shape[0]) == (4, 5, 20)
    good = ("coded", e, 20, None)
    jpeg.plan_batch([good, ("coded", e, None, None)])
    changed = dict(changed)
    claimed = changed.pop("claimed", 20)
    if changed.get("hs"):
        e, claimed = entropy("8x9_420"), int(entropy("8x9_420").coef.shape[0])
    with pytest.raises(ValueError, match="^image 1: an EntropyImage whose fields contradict each other$"):
        jpeg.plan_batch([good, ("coded", Fields(e, **changed), claimed, None)])


@pytest.mark.parametrize("changed", [dict(width=8 * 2 + 1), dict(blocks_y=3), dict(claimed=5), dict(scan_begin=-1), dict(scan_begin=10 ** 6),
                                     dict(file_bytes=jpeg_device.MAX_BYTES + 1), dict(record_bytes=jpeg_device.RECORD_BYTES - 4)],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_a_scan_image_with_one_contradictory_field_is_refused(changed):
    s = scan("8x9_420")  # 2 x 2 luma blocks and one of each chroma: 6 in all
    assert (s.blocks_x, s.blocks_y, s.blocks) == (2, 2, 6)
    sizes = dict(file_bytes=s.data.size, scan_begin=s.scan_begin, record_bytes=s.tables.size)
    good = ("coded", s, s.blocks, tuple(sizes.values()))
    jpeg.plan_batch([good], jpeg_device._SCANS)
    changed = dict(changed)
    claimed = changed.pop("claimed", s.blocks)
    sizes.update({k: changed.pop(k) for k in list(changed) if k in sizes})
    with pytest.raises(ValueError, match="^image 2: a ScanImage whose fields contradict each other$"):
        jpeg.plan_batch([good, ("raw", (2, 2, 3)), ("coded", Fields(s, **changed), claimed, tuple(sizes.values()))], jpeg_device._SCANS)
