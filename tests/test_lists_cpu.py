"""CPU side of the candidate lists (madtp_amd/lists.py, include/madtp_lists.h): the header against the binding and the library's
exports, the ABIs that must not move, every refusal that needs no GPU, the restatement of tests/lists_ref.py against itself, and
all_gather_lists over two gloo ranks."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from madtp_amd import abi
from tests import lists_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "madtp_lists.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))


def test_symbols_are_exported_and_the_other_abis_are_unchanged():
    from madtp_amd import augment, build, hip, lists, preprocess, search
    raw = ctypes.CDLL(build.build(verbose=False))
    syms = _header_symbols()
    assert syms == sorted(lists.SIGNATURES) == ["madtp_lists_abi_version", "madtp_lists_rank", "madtp_lists_sort"]
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/madtp_lists.h but not exported"
    lib = lists.lib()
    assert lib.madtp_lists_abi_version() == lists.ABI_VERSION == 1
    assert lists.MAX_K == 256 == search.MAX_K and lists.MAX_TARGETS == 16
    for name, (res, args) in lists.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    c_int, c_void_p, c_int64, c_float = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert lists.SIGNATURES["madtp_lists_rank"] == (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_float]
                                                    + [c_void_p] * 5)
    assert lists.SIGNATURES["madtp_lists_sort"] == (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int] + [c_void_p] * 3)
    # the seven other headers
    assert len(abi.SIGNATURES) == 97 and not set(abi.SIGNATURES) & set(syms)
    assert hip.ABI_VERSION == 31 == raw.madtp_abi_version()
    versions = {"madtp_image_abi_version": preprocess.ABI_VERSION, "madtp_augment_abi_version": augment.ABI_VERSION,
                "madtp_search_abi_version": search.ABI_VERSION, "madtp_csearch_abi_version": search.COARSE_ABI_VERSION}
    for symbol, bound in versions.items():
        assert getattr(raw, symbol)() == bound == 1, symbol
    for header, define in (("madtp_jpeg.h", "MADTP_JPEG_ABI_VERSION"), ("madtp_jhuff.h", "MADTP_JHUFF_ABI_VERSION")):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert re.search(rf"#define {define} 1\b", text), header
        assert getattr(raw, define.lower())() == 1
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "include"))) == [
        "madtp_augment.h", "madtp_csearch.h", "madtp_hip.h", "madtp_image.h", "madtp_jhuff.h", "madtp_jpeg.h", "madtp_lists.h",
        "madtp_search.h"]
    assert "lists.hip" in build.SOURCES and any(h.endswith("madtp_lists.h") for h in build.HEADERS)


def test_entry_points_refuse_before_any_launch():
    from madtp_amd import build, lists
    build.build(verbose=False)
    lib = lists.lib()
    E_BADARG, E_SHAPE = abi.DEFINES["MADTP_E_BADARG"], abi.DEFINES["MADTP_E_SHAPE"]
    ok = dict(idx=1 << 20, ld_idx=8, val=2 << 20, ld_val=8, n=4, k=8, nk=100, fill=-100.0, tgt_ptr=16, tgt_idx=16, rank_row=16,
              rank_tgt=16, out_idx=3 << 20, out_val=4 << 20)

    def rank(**kw):
        a = dict(ok, **kw)
        return lib.madtp_lists_rank(a["idx"], a["ld_idx"], a["val"], a["ld_val"], a["n"], a["k"], a["nk"], a["fill"], a["tgt_ptr"],
                                    a["tgt_idx"], a["rank_row"], a["rank_tgt"], 0)

    def sort(**kw):
        a = dict(ok, **kw)
        return lib.madtp_lists_sort(a["idx"], a["ld_idx"], a["val"], a["ld_val"], a["n"], a["k"], a["nk"], a["out_idx"], a["out_val"], 0)
    for name in ("idx", "val", "tgt_ptr", "tgt_idx", "rank_row", "rank_tgt"):
        assert rank(**{name: 0}) == E_BADARG, name
    for name in ("idx", "val", "out_idx", "out_val"):
        assert sort(**{name: 0}) == E_BADARG, name
    for call in (rank, sort):
        assert call(k=0) == E_BADARG and call(k=257, ld_idx=300, ld_val=300) == E_BADARG and call(k=-1) == E_BADARG
        assert call(n=0) == E_SHAPE and call(n=-3) == E_SHAPE and call(nk=0) == E_SHAPE and call(nk=-1) == E_SHAPE
        assert call(ld_idx=7) == E_SHAPE and call(ld_val=7) == E_SHAPE
    # an output that overlaps an input (the last input row ends at idx + 8 * (3 * 8 + 8) bytes) or the other output
    assert sort(out_idx=ok["idx"]) == E_BADARG and sort(out_idx=ok["idx"] + 8 * 31) == E_BADARG
    assert sort(out_val=ok["val"] + 4) == E_BADARG and sort(out_val=ok["out_idx"] + 8) == E_BADARG
    assert sort(out_idx=ok["val"] - 8 * 32 + 4) == E_BADARG


def test_python_refusals_name_the_argument():
    from madtp_amd import lists
    idx = torch.zeros(3, 4, dtype=torch.int64)
    val = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="k = 257"):
        lists.CandidateLists(torch.zeros(2, 257, dtype=torch.int64), torch.zeros(2, 257), 1000)
    with pytest.raises(ValueError, match="idx must be an int64"):
        lists.CandidateLists(idx.int(), val, 10)
    with pytest.raises(ValueError, match="val must be a float32"):
        lists.CandidateLists(idx, val.double(), 10)
    with pytest.raises(ValueError, match="one shape"):
        lists.CandidateLists(idx, val[:, :3], 10)
    with pytest.raises(ValueError, match="nk = 2147483648"):
        lists.CandidateLists(idx, val, 2 ** 31)
    with pytest.raises(ValueError, match="nk = 0"):
        lists.CandidateLists(idx, val, 0)
    lists.CandidateLists(idx, val, 2 ** 31 - 1)
    cl = lists.CandidateLists(idx, val, 10)
    assert cl.nbytes == 3 * 4 * 12 and cl.shape == (3, 4) and cl.fill == -100.0 and cl.cpu().device.type == "cpu"
    ptr, tgt = torch.tensor([0, 1, 2, 3], dtype=torch.int32), torch.tensor([1, 2, 3], dtype=torch.int32)
    with pytest.raises(ValueError, match="idx is a CPU tensor"):
        cl.sorted()
    with pytest.raises(ValueError, match="idx is a CPU tensor"):
        cl.top(2)
    with pytest.raises(ValueError, match="tgt_ptr is a CPU tensor"):
        cl.rank(ptr, tgt)
    with pytest.raises(ValueError, match="tgt_ptr must be a contiguous int32"):
        cl.rank(ptr.long(), tgt)
    with pytest.raises(ValueError, match="tgt_ptr has 3 entries for 3 rows"):
        cl.rank(ptr[:3], tgt)
    with pytest.raises(ValueError, match="row 1 has 17 targets, at most 16"):
        cl.rank(torch.tensor([0, 1, 18, 19], dtype=torch.int32), torch.zeros(19, dtype=torch.int32))
    with pytest.raises(ValueError, match="r = 5"):
        cl.top(5)


def test_validate_and_to_dense_on_the_host():
    """validate() and to_dense() are torch operations and run where the lists are"""
    from madtp_amd import lists
    idx = torch.tensor([[3, -1, 0], [1, 2, 4], [-1, -1, -1]])
    val = torch.tensor([[1.0, 9.0, -100.0], [2.0, float("nan"), -200.0], [5.0, 6.0, 7.0]])
    cl = lists.CandidateLists(idx, val, 5, fill=-100.0)
    assert cl.validate() is cl
    dense = cl.to_dense()
    assert dense.shape == (3, 5) and np.array_equal(dense.numpy(), lists_ref.to_dense(idx.numpy(), val.numpy(), 5), equal_nan=True)
    assert dense[0].tolist() == [-100.0, -100.0, -100.0, 1.0, -100.0] and (dense[2] == -100.0).all()
    twice = idx.clone()
    twice[1, 2] = 1
    with pytest.raises(ValueError, match="row 1 holds key 1 twice"):
        lists.CandidateLists(twice, val, 5).validate()
    with pytest.raises(ValueError, match="row 0 holds index 5 outside"):
        lists.CandidateLists(torch.tensor([[3, 5, 0], [1, 1, 4]]), val[:2], 5).validate()
    with pytest.raises(ValueError, match="row 1 holds index -2 outside"):
        lists.CandidateLists(torch.tensor([[3, -1, -1], [1, -2, 4]]), val[:2], 5).validate()


def test_restatement_rank_is_the_stable_argsort_position():
    rng = np.random.RandomState(0)
    for nk in (1, 2, 7, 40):
        row = rng.randint(0, 4, nk).astype(np.float32)
        row[rng.rand(nk) < 0.2] = -100.0
        order = np.argsort(row, kind="stable")[::-1]
        for t in range(nk):
            assert lists_ref.rank_in_row(row, t) == int(np.where(order == t)[0][0])
    idx = np.array([[4, -1, 2, 7, 0]])
    val = np.array([[1.0, 50.0, 1.0, np.nan, -0.0]], dtype=np.float32)
    si, sv = lists_ref.sort(idx, val, 8)
    assert si.tolist() == [[4, 2, 0, 7, -1]] and sv[0, :3].tolist() == [1.0, 1.0, 0.0] and np.isnan(sv[0, 3]) and sv[0, 4] == -np.inf


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _whole_lists(n, k, nk, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randperm(nk, generator=g)[:k] for _ in range(n)])
    return idx, torch.randn(n, k, generator=g)


def _gather_worker(rank, world, port, out_dir):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from madtp_amd import blip_retrieval as br, dist as mdist, lists
    mdist.init("gloo")
    halves = []
    for n, k, nk, seed in ((5, 3, 9, 1), (9, 3, 5, 2)):  # 5 images x 9 texts: the slices are rows [0,3) + [3,5) and [0,5) + [5,9)
        idx, val = _whole_lists(n, k, nk, seed)
        s, e = br.rank_rows(n, rank, world)
        mine = torch.zeros(n, dtype=torch.bool)
        mine[s:e] = True
        halves.append(lists.CandidateLists(torch.where(mine[:, None], idx, torch.full_like(idx, -1)),
                                           torch.where(mine[:, None], val, torch.full_like(val, -100.0)), nk))
    a, b = br.all_gather_lists(*halves)
    torch.save({"i2t": (a.idx, a.val, a.nk, a.fill), "t2i": (b.idx, b.val, b.nk, b.fill)}, os.path.join(out_dir, f"lists{rank}.pt"))
    mdist.barrier()
    torch.distributed.destroy_process_group()


def test_all_gather_lists_merges_two_half_filled_lists(tmp_path):
    from madtp_amd import blip_retrieval as br, lists
    world = 2
    mp.spawn(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [torch.load(os.path.join(str(tmp_path), f"lists{r}.pt")) for r in range(world)]
    for key, (n, k, nk, seed) in (("i2t", (5, 3, 9, 1)), ("t2i", (9, 3, 5, 2))):
        idx, val = _whole_lists(n, k, nk, seed)
        for o in outs:
            assert torch.equal(o[key][0], idx) and torch.equal(o[key][1], val) and o[key][2:] == (nk, -100.0)
    # without a process group: the arguments themselves
    idx, val = _whole_lists(5, 3, 9, 1)
    a, b = lists.CandidateLists(idx, val, 9), lists.CandidateLists(idx, val, 9)
    assert br.all_gather_lists(a, b) == (a, b)


def test_evaluate_refuses_lists_without_device_candidates():
    from madtp_amd import blip_retrieval as br
    for kw in ({}, {"candidates": "dense"}):
        with pytest.raises(ValueError, match="scores = 'lists' needs candidates='device'"):
            br.evaluate(None, None, "cpu", {"k_test": 2}, scores="lists", **kw)
    with pytest.raises(ValueError, match="scores = 'matrix'"):
        br.evaluate(None, None, "cpu", {"k_test": 2}, candidates="device", scores="matrix")
    from madtp_amd import lists, retrieval_eval
    cl = lists.CandidateLists(torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 1), 3)
    with pytest.raises(ValueError, match="one argument is a CandidateLists"):
        retrieval_eval.itm_eval(cl, np.zeros((3, 2), dtype=np.float32), [0, 0, 1], [[0], [2]])
    with pytest.raises(ValueError, match="expected 3 and 2"):
        retrieval_eval.itm_eval(cl, lists.CandidateLists(torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3, 1), 5), [0, 0, 1], [[0], [2]])
