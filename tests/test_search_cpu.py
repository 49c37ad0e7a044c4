"""CPU side of the retrieval search (madtp_amd/search.py, include/madtp_search.h): the exported symbols, the binding against the
header, the refusals that come back before any launch, the workspace size and evaluate()'s keyword."""
import ctypes
import itertools
import os
import re

import pytest

from madtp_amd import abi, augment, build, hip, preprocess, search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "madtp_search.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))


def test_symbols_are_exported_and_the_other_abis_are_unchanged():
    raw = ctypes.CDLL(build.build(verbose=False))
    syms = _header_symbols()
    assert syms == sorted(search.SIGNATURES)
    assert set(syms) == {"madtp_search_abi_version", "madtp_topk_workspace", "madtp_topk_embeds", "madtp_topk_scores"}
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/madtp_search.h but not exported"
    lib = search.lib()
    assert lib.madtp_search_abi_version() == search.ABI_VERSION == 1 and search.MAX_K == 256
    for name, (res, args) in search.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    assert search.SIGNATURES["madtp_topk_workspace"] == (c_size_t, [c_int] * 4)
    assert search.SIGNATURES["madtp_topk_embeds"] == (c_int, [c_void_p, c_int, c_void_p] + [c_int] * 5 + [c_void_p] * 3 + [c_size_t, c_void_p])
    assert search.SIGNATURES["madtp_topk_scores"] == (c_int, [c_void_p] + [c_int] * 4 + [c_void_p] * 3)
    # the other headers and their version numbers
    assert len(abi.SIGNATURES) == 97 and hip.ABI_VERSION == 31
    for other in (abi.SIGNATURES, preprocess.SIGNATURES, augment.SIGNATURES):
        assert not set(other) & set(syms)
    assert lib.madtp_image_abi_version() == preprocess.ABI_VERSION == 1 and augment.lib().madtp_augment_abi_version() == 1
    assert "search.hip" in build.SOURCES and "eval_device.h" in build.HEADERS
    assert any(h.endswith("madtp_search.h") for h in build.HEADERS)


def test_entry_points_refuse_before_any_launch():
    lib = search.lib()
    E_BADARG, E_SHAPE = abi.DEFINES["MADTP_E_BADARG"], abi.DEFINES["MADTP_E_SHAPE"]
    ok = dict(q=16, ldq=64, keys=32, ldk=64, nq=3, nk=70, D=64, k=5, values=16, indices=16, ws=16, ws_bytes=None)

    def embeds(**kw):
        a = dict(ok, **kw)
        if a["ws_bytes"] is None:
            a["ws_bytes"] = max(int(lib.madtp_topk_workspace(a["nq"], a["nk"], a["D"], a["k"])), 8)
        return lib.madtp_topk_embeds(a["q"], a["ldq"], a["keys"], a["ldk"], a["nq"], a["nk"], a["D"], a["k"], a["values"], a["indices"],
                                     a["ws"], a["ws_bytes"], 0)
    for name in ("q", "keys", "values", "indices", "ws"):
        assert embeds(**{name: 0}) == E_BADARG, name
    assert embeds(k=0) == E_BADARG and embeds(k=257) == E_BADARG and embeds(k=-1) == E_BADARG
    for D in (32, 96, 1088, 0):
        assert embeds(D=D, ldq=1088, ldk=1088) == E_SHAPE, D
    assert embeds(ldq=60) == E_SHAPE and embeds(ldk=60) == E_SHAPE            # too small
    assert embeds(ldq=66) == E_SHAPE and embeds(ldk=70) == E_SHAPE            # not a multiple of 4
    assert embeds(D=128, ldq=64) == E_SHAPE and embeds(D=128, ldq=128, ldk=64) == E_SHAPE
    assert embeds(nq=0) == E_SHAPE and embeds(nk=0) == E_SHAPE and embeds(nq=-3) == E_SHAPE
    assert embeds(q=20) == E_BADARG and embeds(keys=8) == E_BADARG            # bases off the 16-byte grid
    need = int(lib.madtp_topk_workspace(3, 70, 64, 5))
    assert need >= 3 * 5 * 8
    assert embeds(ws_bytes=need - 1) == E_BADARG and embeds(ws_bytes=0) == E_BADARG
    # (a call that passes every check would launch: that is the GPU tests' ground)

    ok2 = dict(scores=16, ld=70, nq=3, nk=70, k=5, values=16, indices=16)

    def scores(**kw):
        a = dict(ok2, **kw)
        return lib.madtp_topk_scores(a["scores"], a["ld"], a["nq"], a["nk"], a["k"], a["values"], a["indices"], 0)
    for name in ("scores", "values", "indices"):
        assert scores(**{name: 0}) == E_BADARG, name
    assert scores(k=0) == E_BADARG and scores(k=257) == E_BADARG
    assert scores(ld=69) == E_SHAPE and scores(nq=0) == E_SHAPE and scores(nk=0) == E_SHAPE


def test_workspace_is_monotone_and_zero_for_refused_shapes():
    ws = search.lib().madtp_topk_workspace
    for bad in ((0, 5, 64, 1), (5, 0, 64, 1), (5, 5, 32, 1), (5, 5, 96, 1), (5, 5, 1088, 1), (5, 5, 64, 0), (5, 5, 64, 257)):
        assert ws(*bad) == 0, bad
    nqs = [1, 31, 32, 33, 64, 127, 128, 129, 160, 161, 224, 225, 256, 257, 1000, 1024, 5000, 25010, 32737, 32768, 32769, 100000]
    nks = [1, 63, 64, 65, 255, 256, 257, 1285, 5000, 16384, 25010, 65536, 65537, 1000000]
    ks = [1, 2, 16, 64, 65, 128, 192, 193, 256]
    for nq, nk, k in itertools.product(nqs, nks, ks):
        assert ws(nq, nk, 256, k) >= nq * min(k, 256) * 8  # at least one list of k candidates per row
    for nk, k in itertools.product(nks, ks):
        sizes = [ws(nq, nk, 256, k) for nq in range(1, 2100)] + [ws(nq, nk, 256, k) for nq in nqs if nq >= 2100]
        assert sizes == sorted(sizes), (nk, k)
    for nq, k in itertools.product(nqs, ks):
        sizes = [ws(nq, nk, 256, k) for nk in sorted(set(nks) | set(range(1, 3000, 7)))]
        assert sizes == sorted(sizes), (nq, k)
    for nq, nk in itertools.product(nqs, nks):
        sizes = [ws(nq, nk, 256, k) for k in range(1, 257)]
        assert sizes == sorted(sizes), (nq, nk)
    assert ws(5000, 25010, 256, 256) < 5000 * 25010 * 4 // 4  # COCO: under a quarter of the f32 matrix the call replaces


def test_python_refusals_without_a_gpu():
    import torch
    q, keys = torch.zeros(3, 64), torch.zeros(5, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        search.topk_embeds(q, keys, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        search.topk_scores(torch.zeros(3, 5), 2)
    with pytest.raises(RuntimeError, match="GPU"):
        search.EmbeddingIndex(keys)
    for k in (0, 257):
        with pytest.raises(ValueError, match="k = "):
            search.topk_embeds(q, keys, k)
        with pytest.raises(ValueError, match="k = "):
            search.topk_scores(q, k)


def test_evaluate_refuses_an_unknown_candidate_stage():
    from madtp_amd import blip_retrieval
    with pytest.raises(ValueError, match="nonsense"):
        blip_retrieval.evaluate(None, None, "cpu", {"k_test": 4}, candidates="nonsense")
