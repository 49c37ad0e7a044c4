"""CPU side of the token maps (madtp_amd/tokenmap.py, csrc/madtp_tokenmap.h): the header against the binding and the exported
symbols, the refusals, the restatement of tests/tokenmap_ref.py against harness.compose_ids on the reference's recorded indices, and
the kernels' lane routines run on the host (madtp_tokenmap_*_host) against the restatement.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tokenmap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CANARY = 64


@pytest.fixture(scope="module")
def tm():
    from madtp_amd import build, tokenmap
    build.build(verbose=False)
    tokenmap.lib()
    return tokenmap


# ---- header and binding ----------------------------------------------------------------------------------------------------------------
NAMES = ("abi_version strerror build push pull agree shade build_host push_host pull_host agree_host shade_host").split()


def test_header_binding_and_exported_symbols(tm):
    from madtp_amd import abi, build, hip
    src = re.sub(r"/\*.*?\*/", "", open(tm.HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(madtp_[a-z0-9_]+)\s*\(", src)))
    assert syms == sorted(tm.SIGNATURES) == sorted("madtp_tokenmap_" + s for s in NAMES)
    raw = ctypes.CDLL(build.build(verbose=False))
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in csrc/madtp_tokenmap.h but not exported"
    lib = tm.lib()
    assert lib.madtp_tokenmap_abi_version() == tm.ABI_VERSION == 1
    for name, (res, args) in tm.SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
    i, p, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert tm.SIGNATURES["madtp_tokenmap_build"] == (i, [p, i, i, i, p, p, p, p, p])
    assert tm.SIGNATURES["madtp_tokenmap_push"] == (i, [p, i64, i64, p, p, i64, p, i, i, i, i, p])
    assert tm.SIGNATURES["madtp_tokenmap_pull"] == (i, [p, p, p, i64, p, i, i, i, i, i, p])
    assert tm.SIGNATURES["madtp_tokenmap_agree"] == (i, [p, p, p, i, i, i, p])
    assert tm.SIGNATURES["madtp_tokenmap_shade"] == (i, [p, p, p, p, i, i, i, i, i, i, p])
    assert (tm.MAX_N, tm.MAX_LAYERS, tm.FIELDS, tm.LAYER_BITS, tm.DEFINES["MADTP_TOKENMAP_LANES"]) == (4096, 48, 8, 6, 256)
    assert sorted(tm._F.values()) == list(range(8))
    assert sorted(tm.E) == ["CHAIN", "K", "RANGE", "REPEAT", "TABLE"] and len(set(tm.E.values())) == 5
    assert all(lib.madtp_tokenmap_strerror(c) for c in tm.E.values())
    for name, code in tm.E.items():
        assert tm.status_fields(-((-code << 6) | 47)) == (code, 47) and tm.status_fields(0) == (0, None)
    # the other headers keep their own declarations, and the build knows the new files
    assert not set(abi.SIGNATURES) & set(syms) and hip.ABI_VERSION == raw.madtp_abi_version()
    assert "tokenmap.hip" in build.SOURCES and "tokenmap_device.h" in build.HEADERS and "madtp_tokenmap.h" in build.HEADERS
    assert not os.path.exists(os.path.join(ROOT, "include", "madtp_tokenmap.h"))


def test_every_entry_point_refuses_bad_arguments_before_any_launch(tm):
    """null, negative and oversized arguments: MADTP_E_BADARG from the argument check, which stands before the launch (no GPU here)"""
    lib, BAD = tm.lib(), -1
    buf = np.zeros(4096, np.int64)
    a = buf.ctypes.data  # any non-null address: a refused call reads nothing
    for host in (False, True):
        s = () if host else (None,)
        sfx = "_host" if host else ""
        build, push, pull = getattr(lib, "madtp_tokenmap_build" + sfx), getattr(lib, "madtp_tokenmap_push" + sfx), getattr(lib, "madtp_tokenmap_pull" + sfx)
        agree, shade = getattr(lib, "madtp_tokenmap_agree" + sfx), getattr(lib, "madtp_tokenmap_shade" + sfx)
        for args in ([None, 1, 1, 8, a, a, a, a], [a, 1, 1, 8, None, a, a, a], [a, 1, 1, 8, a, None, a, a], [a, 1, 1, 8, a, a, None, a],
                     [a, 1, 1, 8, a, a, a, None], [a, 0, 1, 8, a, a, a, a], [a, 49, 1, 8, a, a, a, a], [a, 1, 0, 8, a, a, a, a],
                     [a, 1, -3, 8, a, a, a, a], [a, 1, 65536, 8, a, a, a, a], [a, 1, 1, 0, a, a, a, a], [a, 1, 1, 4097, a, a, a, a]):
            assert build(*args, *s) == BAD, args
        for args in ([None, 8, 1, a, a, 8, a, 1, 8, 4, 1], [a, 8, 1, None, a, 8, a, 1, 8, 4, 1], [a, 8, 1, a, None, 8, a, 1, 8, 4, 1],
                     [a, 8, 1, a, a, 8, None, 1, 8, 4, 1], [a, 8, 1, a, a, 8, a, 0, 8, 4, 1], [a, 8, 1, a, a, 8, a, 1, 0, 4, 1],
                     [a, 8, 1, a, a, 8, a, 1, 4097, 4, 1], [a, 8, 1, a, a, 8, a, 1, 8, 0, 1], [a, 8, 1, a, a, 8, a, 1, 8, 4097, 1],
                     [a, 8, 1, a, a, 8, a, 1, 8, 4, 0], [a, 8, 1, a, a, 8, a, 1, 8, 4, 65537], [a, 8, 2, a, a, 8, a, 1, 8, 4, 3],
                     [a, 8, 1, a, a, 8, a, 2, 8, 4, 2], [a, 16, 2, a, a, 7, a, 2, 8, 4, 2], [a, -16, 2, a, a, 8, a, 2, 8, 4, 2]):
            assert push(*args, *s) == BAD, args
        for args in ([None, a, a, 8, a, 1, 8, 4, 1, 0], [a, None, a, 8, a, 1, 8, 4, 1, 0], [a, a, None, 8, a, 1, 8, 4, 1, 1],
                     [a, a, a, 8, None, 1, 8, 4, 1, 0], [a, a, a, 8, a, 0, 8, 4, 1, 0], [a, a, a, 8, a, 1, 0, 4, 1, 0],
                     [a, a, a, 8, a, 1, 8, 0, 1, 0], [a, a, a, 8, a, 1, 8, 4097, 1, 0], [a, a, a, 8, a, 1, 8, 4, 0, 0],
                     [a, a, a, 8, a, 1, 8, 4, 65537, 0], [a, a, a, 8, a, 1, 8, 4, 1, 2], [a, a, a, 7, a, 2, 8, 4, 1, 0]):
            assert pull(*args, *s) == BAD, args
        for args in ([None, a, a, 1, 8, 2], [a, None, a, 1, 8, 2], [a, a, None, 1, 8, 2], [a, a, a, 0, 8, 2], [a, a, a, 1, 0, 2],
                     [a, a, a, 1, 4097, 2], [a, a, a, 1, 8, 0], [a, a, a, 1, 8, 49]):
            assert agree(*args, *s) == BAD, args
        for args in ([None, a, a, a, 1, 2, 2, 4, 4, 2], [a, None, a, a, 1, 2, 2, 4, 4, 2], [a, a, None, a, 1, 2, 2, 4, 4, 2],
                     [a, a, a, None, 1, 2, 2, 4, 4, 2], [a, a, a, a, 0, 2, 2, 4, 4, 2], [a, a, a, a, 1, 0, 2, 4, 4, 2],
                     [a, a, a, a, 1, 2, 2, 0, 4, 2], [a, a, a, a, 1, 2, 2, 4, 4, 0], [a, a, a, a, 1, 2, 2, 4, 4, 49],
                     [a, a, a, a, 1, 2, 2, 16384, 4, 2], [a, a, a, a, 1, 128, 128, 4, 4, 2]):
            assert shade(*args, *s) == BAD, args
        assert shade(a, a, a, a, 1, 1, 1, 3, 5, 2, *s) == -4  # MADTP_E_ALIGN: 45 bytes per image
        assert shade(a + 4, a, a, a, 1, 2, 2, 4, 4, 2, *s) == -4


def test_python_refusals_name_the_argument(tm):
    recs = ref.records((2, 63, 3))
    with pytest.raises(ValueError, match=r"records\[0\]\['indices'\].*not a tensor"):
        tm.from_records(recs, 63)
    t = [None if r is None else {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in recs]
    with pytest.raises(ValueError, match=r"records\[0\]\['indices'\].*CPU tensor.*no CPU fallback"):
        tm.from_records(t, 63)
    with pytest.raises(ValueError, match=r"records\[0\]: a pruned layer without 'score'"):
        tm.build_host([{"pruned": True, "k": 3, "indices": recs[0]["indices"], "indices_sort": recs[0]["indices_sort"]}], 63)
    np_recs = lambda: [None if r is None else dict(r) for r in recs]
    for n0, what in ((0, "n0 = 0"), (4097, "n0 = 4097")):
        with pytest.raises(ValueError, match=what):
            tm.build_host(np_recs(), n0)
    with pytest.raises(ValueError, match="49 layers"):
        tm.build_host([None] * 46 + np_recs(), 63)
    bad = np_recs()
    bad[2]["score"] = bad[2]["score"][:1]
    with pytest.raises(ValueError, match=r"records\[2\]\['score'\]: 1 samples"):
        tm.build_host(bad, 63)
    bad = np_recs()
    bad[0]["indices_sort"] = bad[0]["indices_sort"][:, :50].copy()
    with pytest.raises(ValueError, match=r"records\[0\]\['indices_sort'\]: 50 columns, the layer reads 63"):
        tm.build_host(bad, 63)
    bad = np_recs()
    bad[0]["score"] = bad[0]["score"].astype(np.float64)
    with pytest.raises(ValueError, match=r"records\[0\]\['score'\]: must be a numpy float32"):
        tm.build_host(bad, 63)
    # a map of CPU tensors: every method refuses and names its argument
    c = ref.compose(recs, 63)
    m = tm.TokenMap(torch.from_numpy(c["slot"].astype(np.int32)), torch.from_numpy(c["coef"].astype(np.float32)),
                    torch.from_numpy(c["depth"].astype(np.int32)), c["n_out"], c["pruned"])
    assert (m.B, m.L, m.n0) == (2, 3, 63) and m.kept(1).shape == (2, 63)
    with pytest.raises(ValueError, match="x is a CPU tensor.*no CPU fallback"):
        m.push(torch.zeros(2, 63, 4), 0)
    with pytest.raises(ValueError, match="v is a CPU tensor"):
        m.pull(torch.zeros(2, 41, 4), 0)
    with pytest.raises(ValueError, match=r"x \(2, 62, 4\) must be \[2, 63\]"):
        m.push(torch.zeros(2, 62, 4), 0)
    with pytest.raises(ValueError, match="x must be a float32 tensor"):
        m.push(torch.zeros(2, 63, 4, dtype=torch.float64), 0)
    with pytest.raises(ValueError, match=r"l = 3 is not a layer in \[0, 3\)"):
        m.kept(3)
    with pytest.raises(ValueError, match="b must be a TokenMap"):
        tm.agreement(m, c["depth"])
    with pytest.raises(ValueError, match="images is a CPU tensor"):
        tm.shade(torch.zeros(2, 36, 28, 3, dtype=torch.uint8), m, (9, 7))
    with pytest.raises(ValueError, match="images must be a uint8"):
        tm.shade(torch.zeros(2, 36, 28, 3), m, (9, 7))


# ---- the restatement against the code the kept-set match rests on -------------------------------------------------------------------
@pytest.mark.parametrize("case,key,n0_of", [("nlvr_b2_T5", "vit", lambda g: 196), ("nlvr_b2_T5", "txt", lambda g: int(g["L"]) - 1),
                                            ("clip_vit_b2", "vit", lambda g: 196), ("med_text_b3", "txt", lambda g: int(g["L"]) - 1)])
def test_restatement_equals_compose_ids_on_the_reference_traces(case, key, n0_of):
    from madtp_amd import harness
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    n0, lens = n0_of(g), g[key + "_lens"].reshape(-1)[-12:].tolist()
    # the first lens[l] - 2 columns of a recorded index tensor count (the text side records one column more under padding)
    trace = [{"pruned": True, "indices": g[f"{key}{l}_idx"][:, :lens[l] - 2], "k": lens[l] - 2} if f"{key}{l}_idx" in g.files else None
             for l in range(12)]
    want = harness.compose_ids(trace, n0)
    if all(t is None for t in trace):
        assert lens == [n0 + 1] * 12
        return
    c = ref.compose(trace, n0)
    assert [n + 1 for n in c["n_out"]] == lens
    seen = 0
    for l in range(12):
        if want[l] is None:
            assert not c["pruned"][l]
            continue
        seen += 1
        want[l] = [{i for i in s if i < harness.MERGED_BASE} for s in want[l]]  # (a kept merged token is no original position)
        assert ref.kept_sets(c["depth"], l) == want[l], f"{case} {key} layer {l}"
        # the slots of the kept positions are where compose_ids' bookkeeping has them
        for b, kept in enumerate(want[l]):
            assert sorted(c["slot"][b, l, sorted(kept)].tolist()) == sorted(set(c["slot"][b, l, sorted(kept)].tolist()))
            assert np.all(c["coef"][b, l, sorted(kept)] == 1.0)
    assert seen >= 1


# ---- the host emulation against the restatement ----------------------------------------------------------------------------------------
def coef_bound(L, n_max, coef64):
    """a sequential f32 sum of up to n_max terms, the + 1e-8, one division and L products: (n_max + 3) roundings per layer at the most"""
    return L * (n_max + 3) * 2.0 ** -24 * np.abs(coef64)


@pytest.mark.parametrize("shape", ref.SHAPES, ids=[f"B{b}_n{n}_L{l}" for b, n, l in ref.SHAPES])
def test_host_emulation_equals_the_restatement(tm, shape):
    B, n0, L = shape
    recs = ref.records(shape)
    c = ref.compose(recs, n0)
    slot, coef, depth, status = tm.build_host(recs, n0)
    assert status.tolist() == [0] * B
    assert np.array_equal(slot, c["slot"]) and np.array_equal(depth, c["depth"])
    assert slot.min() >= 0 and all(slot[:, l].max() < c["n_out"][l] for l in range(L))
    err, bound = np.abs(coef - c["coef"]), coef_bound(L, n0, c["coef"])
    print(f"{shape}: max |coef - coef64| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound) and np.all(coef[depth[:, None, :] > np.arange(L)[None, :, None]] == 1.0)
    if shape in ref.ZERO_LAYER:
        l = ref.ZERO_LAYER[shape]
        merged = slot[:, l] == c["n_out"][l] - 1
        assert merged.sum() >= 2 * B and np.all(coef[:, l][merged] == 0.0) and not np.isnan(coef).any()
    # push, pull, agree on the map: layer by layer for the small shapes, the last layer for the long ones
    rng = np.random.default_rng(n0)
    for C in (1, 4, 6):
        x = rng.standard_normal((B, n0, C), dtype=np.float32)
        for l in (range(L) if n0 < 100 else [L - 1]):
            n_out = c["n_out"][l]
            y = tm.push_host(x, slot[:, l], coef[:, l], n_out)
            tot, cells = ref.push_abs(x, slot[:, l], coef[:, l].astype(np.float64), n_out)
            want = ref.push(x, slot[:, l], coef[:, l].astype(np.float64), n_out)
            assert np.all(np.abs(y - want) <= (cells[:, :, None] + 1) * 2.0 ** -24 * tot), (C, l)  # one rounding per fused cell
            v = rng.standard_normal((B, n_out, C), dtype=np.float32)
            assert np.array_equal(tm.pull_host(v, slot[:, l], coef[:, l]), ref.pull(v, slot[:, l]))
            assert np.array_equal(tm.pull_host(v, slot[:, l], coef[:, l], weighted=True), ref.pull(v, slot[:, l], coef[:, l]))
    other = depth.copy()
    other[:, ::3] = np.minimum(other[:, ::3], 1)  # a second run that diverges at layer 1
    for a, b in ((depth, depth), (depth, other), (other, depth)):
        got = tm.agree_host(a, b, L)
        assert np.array_equal(got, ref.agree(a, b, L))
    same = tm.agree_host(depth, depth, L)
    assert np.array_equal(same[..., 0], same[..., 1]) and same[:, 0, 0].tolist() == [c["n_out"][0] - 1 if c["pruned"][0] else n0] * B


def test_push_host_drops_a_slot_out_of_range_and_reads_strided_rows(tm):
    B, n0, C, n_out = 2, 70, 8, 9
    rng = np.random.default_rng(5)
    slot = rng.integers(0, n_out - 1, (B, n0)).astype(np.int32)  # slot n_out - 1 stays empty: a row of zeros
    slot[0, 3], slot[1, 69] = -1, n_out
    coef = rng.random((B, n0), dtype=np.float32)
    x = rng.standard_normal((B, n0, C), dtype=np.float32)
    y = tm.push_host(x, slot, coef, n_out)
    ok = (slot >= 0) & (slot < n_out)
    want = ref.push(x * ok[:, :, None], np.where(ok, slot, 0), coef.astype(np.float64), n_out)
    assert np.allclose(y, want, rtol=0, atol=1e-5) and np.all(y[:, n_out - 1] == 0)
    assert np.array_equal(tm.pull_host(y, slot, coef)[~ok], np.zeros((2, C), np.float32))


def test_shade_host_equals_the_integer_formula(tm):
    rng = np.random.default_rng(7)
    for B, gh, gw, ph, pw, L in ((2, 3, 4, 4, 4, 3), (1, 2, 5, 8, 3, 12), (3, 1, 1, 4, 4, 1)):
        images = rng.integers(0, 256, (B, gh * ph, gw * pw, 3), dtype=np.uint8)
        images[0, 0, 0] = (255, 0, 1)
        depth = rng.integers(0, L + 1, (B, gh * gw)).astype(np.int32)
        levels = [0] + sorted(rng.integers(1, 255, L - 1).tolist()) + [255] if L > 1 else [7, 255]
        got = tm.shade_host(images, depth, (gh, gw), levels)
        assert np.array_equal(got, ref.shade(images, depth, (gh, gw), levels))
        assert np.array_equal(tm.shade_host(images, np.full_like(depth, L), (gh, gw), levels), images)  # level 255 is the identity


# ---- damaged records -------------------------------------------------------------------------------------------------------------------
def _build_with_canaries(tm, recs, n0):
    """madtp_tokenmap_build_host into buffers with canaries on both sides -> (slot, coef, depth, status); the canaries must be intact"""
    table, B, n_out, _ = tm._table(recs, n0, lambda t: t.ctypes.data, tm._np_ok)
    L = len(table)
    bufs = []
    for count, dtype, fill in ((B * L * n0, np.int32, -7), (B * L * n0, np.float32, -7), (B * n0, np.int32, -7), (B, np.int32, 1)):
        buf = np.full(count + 2 * CANARY, 0x5a5a5a5a if dtype == np.int32 else 1234.5, dtype)
        buf[CANARY:CANARY + count] = fill
        bufs.append(buf)
    rc = tm.lib().madtp_tokenmap_build_host(table.ctypes.data, L, B, n0, *(b.ctypes.data + CANARY * 4 for b in bufs))
    assert rc == 0
    for buf in bufs:
        edge = np.concatenate([buf[:CANARY], buf[-CANARY:]])
        assert np.all(edge == edge[0]), "a write outside the outputs"
    slot, coef, depth, status = (b[CANARY:-CANARY] for b in bufs)
    return slot.reshape(B, L, n0), coef.reshape(B, L, n0), depth.reshape(B, n0), status


def _damage(recs, layer, what, n0):
    recs = [None if r is None else {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in recs]
    r = recs[layer]
    k, n_in = r["k"], n0
    for q in recs[:layer]:
        n_in = n_in if q is None else q["k"] + 1
    if what == "index == n_in":
        r["indices"][1, k // 2] = n_in
    elif what == "index == n_in in the merged part":
        r["indices_sort"][1, k] = n_in
    elif what == "negative index":
        r["indices"][1, 0] = -1
    elif what == "far index":
        r["indices"][1, k - 1] = 1 << 40
    elif what == "repeat":
        r["indices"][1, 0] = r["indices"][1, k - 1]
    elif what == "repeat in the merged part":
        r["indices_sort"][1, k] = r["indices_sort"][1, k + 1]
    elif what == "k > n_in":
        r["k"] = n_in + 1
    elif what == "k == n_in":
        r["k"] = n_in
    elif what == "k == 0":
        r["k"] = 0
    return recs


@pytest.mark.parametrize("what,code", [("index == n_in", "RANGE"), ("index == n_in in the merged part", "RANGE"), ("negative index", "RANGE"),
                                       ("far index", "RANGE"), ("repeat", "REPEAT"), ("repeat in the merged part", "REPEAT"),
                                       ("k > n_in", "K"), ("k == n_in", "K"), ("k == 0", "K")])
def test_damaged_records_give_their_code_and_write_nothing_else(tm, what, code):
    shape, layer = (2, 196, 12), 5  # wide buffers, so that a k above n_in still has columns to (not) read
    B, n0, L = shape
    good = ref.records(shape)
    clean = _build_with_canaries(tm, good, n0)
    assert clean[3].tolist() == [0, 0]
    slot, coef, depth, status = _build_with_canaries(tm, _damage(good, layer, what, n0), n0)
    per_sample = code != "K"  # k belongs to the whole layer
    assert tm.status_fields(status[1]) == (tm.E[code], layer)
    assert np.all(slot[1] == -7) and np.all(coef[1] == -7) and np.all(depth[1] == -7), "a damaged sample's outputs are left alone"
    if per_sample:
        assert status[0] == 0 and np.array_equal(slot[0], clean[0][0]) and np.array_equal(coef[0], clean[1][0]) and np.array_equal(depth[0], clean[2][0])
    else:
        assert tm.status_fields(status[0]) == (tm.E[code], layer) and np.all(slot[0] == -7)
    with pytest.raises(ValueError, match=rf"sample {0 if not per_sample else 1}, layer {layer}: .*\(code {tm.E[code]}\)"):
        tm._raise_status(status)


def test_a_broken_chain_or_table_row_gives_its_code(tm):
    shape = (2, 63, 3)
    recs = ref.records(shape)
    table, B, _, _ = tm._table(recs, 63, lambda t: t.ctypes.data, tm._np_ok)
    out = [np.zeros(B * 3 * 63, np.int32), np.zeros(B * 3 * 63, np.float32), np.zeros(B * 63, np.int32), np.zeros(B, np.int32)]
    run = lambda t: (tm.lib().madtp_tokenmap_build_host(t.ctypes.data, 3, B, 63, *(o.ctypes.data for o in out)), out[3].tolist())
    assert run(table) == (0, [0, 0])
    for row, field, value, code in ((1, "N_IN", 40, "CHAIN"), (0, "N_IN", 62, "CHAIN"), (0, "SCORE", 0, "TABLE"), (0, "SORT_STRIDE", 62, "TABLE"),
                                    (0, "INDICES_STRIDE", 39, "TABLE"), (2, "K", 41, "K"), (2, "K", -2, "K"), (2, "K", 0, "K")):
        t = table.copy()
        t[row, tm._F[field]] = value
        rc, status = run(t)
        assert rc == 0 and [tm.status_fields(s) for s in status] == [(tm.E[code], row)] * B, (field, value)
