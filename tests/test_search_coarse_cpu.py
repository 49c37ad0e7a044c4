"""CPU side of the certified bf16 shortlist (madtp_amd/search.py, include/madtp_csearch.h): the exported symbols, the binding
against the header, the refusals that come back before any launch, the workspace size and the host restatement of the bound."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from madtp_amd import abi, augment, build, hip, preprocess, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"madtp_csearch_abi_version", "madtp_coarse_prepare", "madtp_coarse_summary", "madtp_ctopk_workspace", "madtp_ctopk_embeds"}


def _header_symbols(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src))


def test_symbols_are_exported_and_the_other_abis_are_unchanged():
    raw = ctypes.CDLL(build.build(verbose=False))
    assert _header_symbols("madtp_csearch.h") == SYMBOLS == set(search.CSIGNATURES)
    for s in SYMBOLS:
        assert hasattr(raw, s), f"{s} declared in include/madtp_csearch.h but not exported"
    lib = search.clib()
    assert lib.madtp_csearch_abi_version() == search.COARSE_ABI_VERSION == 1
    assert search.COARSE_MAX_K == 128 and search.SHORTLISTS == (64, 128, 256)
    for name, (res, args) in search.CSIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert search.CSIGNATURES["madtp_ctopk_workspace"] == (c_size_t, [c_int] * 5)
    assert search.CSIGNATURES["madtp_coarse_prepare"] == (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p])
    assert search.CSIGNATURES["madtp_coarse_summary"] == (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p])
    assert search.CSIGNATURES["madtp_ctopk_embeds"] == (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p] + [c_int] * 5 +
                                                        [c_void_p] * 6 + [c_size_t, c_void_p])
    # the six other headers: their versions, and the symbol set of madtp_search.h
    assert len(abi.SIGNATURES) == 97 and hip.ABI_VERSION == 31
    assert lib.madtp_search_abi_version() == search.ABI_VERSION == 1 and search.MAX_K == 256
    assert lib.madtp_image_abi_version() == preprocess.ABI_VERSION == 1 and augment.lib().madtp_augment_abi_version() == 1
    versions = {}
    for header in ("madtp_jpeg.h", "madtp_jhuff.h"):
        versions.update({k: v for k, v in abi.parse(open(os.path.join(ROOT, "include", header)).read(), header)[2].items()
                         if k.endswith("_ABI_VERSION")})
    assert versions == {"MADTP_JPEG_ABI_VERSION": 1, "MADTP_JHUFF_ABI_VERSION": 1}, versions
    assert _header_symbols("madtp_search.h") == {"madtp_search_abi_version", "madtp_topk_workspace", "madtp_topk_embeds",
                                                 "madtp_topk_scores"} == set(search.SIGNATURES)
    for other in (abi.SIGNATURES, preprocess.SIGNATURES, augment.SIGNATURES, search.SIGNATURES):
        assert not set(other) & SYMBOLS
    assert "search_coarse.hip" in build.SOURCES and "search_device.h" in build.HEADERS
    assert any(h.endswith("madtp_csearch.h") for h in build.HEADERS)


def test_entry_points_refuse_before_any_launch():
    lib = search.clib()
    E_BADARG, E_SHAPE = abi.DEFINES["MADTP_E_BADARG"], abi.DEFINES["MADTP_E_SHAPE"]
    ok = dict(q=16, ldq=64, keys=32, ldk=64, keys16=48, summary=64, nq=3, nk=700, D=64, k=5, m=64, values=16, indices=16, info=16,
              sl_idx=None, sl_coarse=None, ws=16, ws_bytes=None)

    def embeds(**kw):
        a = dict(ok, **kw)
        if a["ws_bytes"] is None:
            a["ws_bytes"] = max(int(lib.madtp_ctopk_workspace(a["nq"], a["nk"], a["D"], a["k"], a["m"])), 8)
        return lib.madtp_ctopk_embeds(a["q"], a["ldq"], a["keys"], a["ldk"], a["keys16"], a["summary"], a["nq"], a["nk"], a["D"], a["k"],
                                      a["m"], a["values"], a["indices"], a["info"], a["sl_idx"], a["sl_coarse"], a["ws"], a["ws_bytes"], 0)
    for name in ("q", "keys", "keys16", "summary", "values", "indices", "info", "ws"):
        assert embeds(**{name: 0}) == E_BADARG, name
    assert embeds(sl_idx=16) == E_BADARG and embeds(sl_coarse=16) == E_BADARG  # one without the other
    for k, m in ((0, 64), (-1, 64), (129, 256), (33, 64), (65, 128), (5, 96), (5, 32), (5, 512), (5, 0)):
        assert embeds(k=k, m=m) == E_BADARG, (k, m)
    for D in (32, 96, 1088, 0):
        assert embeds(D=D, ldq=1088, ldk=1088) == E_SHAPE, D
    assert embeds(ldq=60) == E_SHAPE and embeds(ldk=60) == E_SHAPE and embeds(ldq=66) == E_SHAPE and embeds(ldk=70) == E_SHAPE
    assert embeds(nq=0) == E_SHAPE and embeds(nk=0) == E_SHAPE and embeds(nq=-3) == E_SHAPE
    for name in ("q", "keys", "keys16", "summary", "ws"):
        assert embeds(**{name: 24}) == E_BADARG, name  # off the 16-byte grid
    need = int(lib.madtp_ctopk_workspace(3, 700, 64, 5, 64))
    assert embeds(ws_bytes=need - 1) == E_BADARG and embeds(ws_bytes=0) == E_BADARG

    prep = lambda x=16, ldx=64, n=3, D=64, x16=32, stats=48: lib.madtp_coarse_prepare(x, ldx, n, D, x16, stats, 0)
    assert prep(x=0) == prep(x16=0) == prep(stats=0) == prep(x=8) == prep(x16=8) == E_BADARG
    assert prep(n=0) == prep(D=32) == prep(D=1088, ldx=1088) == prep(ldx=60) == prep(ldx=66) == E_SHAPE
    summ = lambda stats=16, n=3, out=32: lib.madtp_coarse_summary(stats, n, out, 0, 0)
    assert summ(stats=0) == summ(out=0) == E_BADARG and summ(n=0) == E_SHAPE


def test_workspace_is_monotone_and_zero_for_refused_arguments():
    ws = search.clib().madtp_ctopk_workspace
    for bad in ((0, 5, 64, 1, 64), (5, 0, 64, 1, 64), (5, 5, 32, 1, 64), (5, 5, 1088, 1, 64), (5, 5, 64, 0, 64), (5, 5, 64, 129, 256),
                (5, 5, 64, 33, 64), (5, 5, 64, 5, 96), (5, 5, 64, 5, 512)):
        assert ws(*bad) == 0, bad
    nqs = [1, 31, 32, 33, 64, 127, 128, 129, 1000, 1024, 5000, 25010, 32768, 32769, 100000]
    nks = [1, 63, 64, 65, 255, 256, 257, 1285, 5000, 16384, 25010, 65536, 65537, 1000000]
    for m in (64, 128, 256):
        ks = [k for k in (1, 2, 16, 32, 33, 64, 65, 128) if 2 * k <= m]
        for nq, nk, k in itertools.product(nqs, nks, ks):
            # the exact route's lists for the fallback, one list of m words per row, the rows' bf16 copy
            assert ws(nq, nk, 256, k, m) >= search.lib().madtp_topk_workspace(nq, nk, 256, k) + nq * m * 8 + nq * 256 * 2
        for nk, k in itertools.product(nks, ks):
            sizes = [ws(nq, nk, 256, k, m) for nq in range(1, 1100)] + [ws(nq, nk, 256, k, m) for nq in nqs if nq >= 1100]
            assert sizes == sorted(sizes), (nk, k, m)
        for nq, k in itertools.product(nqs, ks):
            sizes = [ws(nq, nk, 256, k, m) for nk in sorted(set(nks) | set(range(1, 3000, 7)))]
            assert sizes == sorted(sizes), (nq, k, m)
        for nq, nk in itertools.product(nqs, nks):
            sizes = [ws(nq, nk, 256, k, m) for k in range(1, m // 2 + 1)]
            assert sizes == sorted(sizes), (nq, nk, m)


def test_python_refusals_without_a_gpu():
    q, keys = torch.zeros(3, 64), torch.zeros(500, 64)
    with pytest.raises(ValueError, match="k = 129"):
        search.topk_embeds(q, keys, 129, coarse="bf16")
    with pytest.raises(ValueError, match="k = 0"):
        search.topk_embeds(q, keys, 0, coarse="bf16")
    with pytest.raises(ValueError, match="shortlist = 64"):   # m < 2 k
        search.topk_embeds(q, keys, 40, coarse="bf16", shortlist=64)
    with pytest.raises(ValueError, match="shortlist = 96"):
        search.topk_embeds(q, keys, 5, coarse="bf16", shortlist=96)
    with pytest.raises(ValueError, match="coarse = 'fp8'"):
        search.topk_embeds(q, keys, 5, coarse="fp8")
    with pytest.raises(ValueError, match="coarse='bf16'"):
        search.topk_embeds(q, keys, 5, shortlist=64)
    with pytest.raises(ValueError, match="coarse='bf16'"):
        search.topk_embeds(q, keys, 5, return_info=True)
    with pytest.raises(RuntimeError, match="GPU"):
        search.topk_embeds(q, keys, 5, coarse="bf16")
    with pytest.raises(RuntimeError, match="GPU"):
        search.EmbeddingIndex(keys, coarse="bf16")
    with pytest.raises(ValueError, match="coarse = 'fp8'"):
        search.EmbeddingIndex(keys, coarse="fp8")
    with pytest.raises(RuntimeError, match="GPU"):
        search.prepare(keys)
    from madtp_amd import blip_retrieval
    with pytest.raises(ValueError, match="k = 129"):
        blip_retrieval.evaluate(None, None, "cpu", {"k_test": 129}, candidates="device", coarse="bf16")
    with pytest.raises(ValueError, match="candidates='device'"):
        blip_retrieval.evaluate(None, None, "cpu", {"k_test": 4}, coarse="bf16")


def _families():
    rng = np.random.default_rng(31)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    f32 = lambda x: torch.from_numpy(x.astype(np.float32))
    q, keys = f32(unit(rng.standard_normal((24, 256)))), f32(unit(rng.standard_normal((600, 256))))
    yield "unit", q, keys
    heavy = lambda n: f32(rng.choice([-1.0, 1.0], (n, 1024)) * rng.uniform(1, 2, (n, 1024)))
    yield "cancellation", heavy(12), heavy(300)
    yield "x 1e4", q * 1e4, keys * 1e4
    yield "x 1e-30", q * 1e-30, keys * 1e-30


def _f32_chain(q, keys):
    """<q_r, y_j> as an f32 fmaf chain over the features in index order (numpy has no fmaf: the product is formed in float64,
    where it is exact, and the sum is rounded to f32 once - which is what fmaf does, up to a double rounding no bound here feels)"""
    acc = np.zeros((q.shape[0], keys.shape[0]), np.float32)
    q64, k64 = q.double().numpy(), keys.double().numpy()
    for i in range(q.shape[1]):
        acc = (acc.astype(np.float64) + np.outer(q64[:, i], k64[:, i])).astype(np.float32)
    return acc.astype(np.float64)


def test_coarse_bound_against_float64_brute_force():
    """E_r bounds, for every pair, the distance between an f32 fmaf chain over the f32 rows (the exact route's arithmetic) and
    the real product of the bf16 rows (torch's CPU rounding, the coarse stage without its accumulation error); the operand terms
    alone bound the distance of the two real products."""
    for name, q, keys in _families():
        D = q.shape[1]
        E = search.coarse_bound(q, keys)
        assert E.dtype == torch.float64 and E.shape == (q.shape[0],)
        real = (q.double() @ keys.double().t()).numpy()
        q16, k16 = q.bfloat16().double(), keys.bfloat16().double()
        real16 = (q16 @ k16.t()).numpy()
        chain = _f32_chain(q, keys)
        third = (search.COARSE_ACC_FACTOR * D * 2.0 ** -24 * q16.norm(dim=1) * k16.norm(dim=1).max()).numpy()
        assert (np.abs(chain - real16) <= (E.numpy() - third)[:, None]).all(), name
        operand = ((q.double() - q16).norm(dim=1) * keys.double().norm(dim=1).max()
                   + q16.norm(dim=1) * (keys.double() - k16).norm(dim=1).max()).numpy()
        assert (np.abs(real - real16) <= operand[:, None] * (1 + 1e-12)).all(), name
        assert (operand <= E.numpy()).all(), name
        ratio = float((np.abs(chain - real16) / E.numpy()[:, None]).max())
        print(f"{name}: max |chain - <q16, y16>| / E = {ratio:.3g}")
        assert ratio > 1e-3 or name == "x 1e-30"  # the bound is a bound, not an ocean
