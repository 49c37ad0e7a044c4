"""The attention dispatch policy against the decisions recorded from the commit before the planner existed (no GPU).

tests/golden/attn_plan_parent.npz holds, one row per column, the inputs of ~190 k madtp_i_attention_launch / madtp_i_attention_pair
calls (the launchers behind every madtp_attention* entry point) and what the old dispatch decided for each: kernel family and
instantiation, grid, workgroup size, LDS bytes, the scratch areas it fetched, or the status it returned; `launches` is how many
kernels the call started.  Every one of them is replayed through hip.attention_plan() and must come out field for field the same.
Rows are stored by environment setting; the library reads its switches once, so every setting is replayed in a fresh child process.

A pair that does not run as one launch is planned as the launcher runs it: problem 0, then problem 1, as single launches; the
recorded fields are those of the first kernel started, the status is the call's."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_plan_parent.npz")
F32, BF16, F16S, F16 = 0, 1, 2, 3
ARGS = ("B", "H", "Nq", "Nk", "ldq", "ldk", "ldv", "ldo", "io_dtype", "ld_mask_qk", "kv_block_rows", "split_req", "flags", "res")
INSTANCE = ("family", "nt", "storage", "scores", "f16", "hs", "rb", "hv")  # what names a kernel instantiation


@pytest.fixture(scope="module")
def golden():
    from madtp_amd import build
    build.build(verbose=False)
    z = np.load(GOLDEN)
    inputs = dict(zip([str(c) for c in z["input_cols"]], z["inputs"]))
    plans = dict(zip([str(c) for c in z["plan_cols"]], z["plans"]))
    return z, inputs, plans


def _plan_call(hip, r, at, buf):
    """(plan fields, kernels started) of one recorded call: a single launch, or a pair as madtp_attention_pair runs it"""
    a = [r[at[c]] for c in ARGS]
    got = list(hip.attention_plan(*a, out=buf))
    if got[0] != hip.ATTN_PAIR_TWO_LAUNCHES:
        return got, int(got[0] == 0)
    assert r[at["entry"]] == 1 and got[1:] == [-1] + [0] * (len(got) - 2)
    fl = r[at["flags"]]
    single = fl & ~(hip.ATTN_PLAN_PAIR | hip.ATTN_PLAN_PAIR_UNALIGNED | hip.ATTN_PLAN_PAIR_MASKS_DIFFER | hip.ATTN_PLAN_DEV_Q_ONLY)
    if fl & hip.ATTN_PLAN_N_DEV:
        single |= hip.ATTN_PLAN_DEV_Q_ONLY
    second = single & ~(hip.ATTN_PLAN_QKV_UNALIGNED | hip.ATTN_PLAN_NULL_PTR)  # the second problem's own pointers
    if fl & hip.ATTN_PLAN_PAIR_UNALIGNED:
        second |= hip.ATTN_PLAN_QKV_UNALIGNED
    if fl & hip.ATTN_PLAN_PAIR_MASKS_DIFFER:
        second ^= hip.ATTN_PLAN_ADD_MASK
    a[ARGS.index("flags")] = single
    first = list(hip.attention_plan(*a, out=buf))
    if first[0]:
        return first, 0
    a[ARGS.index("flags")] = second
    status = hip.attention_plan(*a, out=buf)[0]
    first[0] = status
    return first, 1 if status else 2


def _replay(path, env_index, out_path):
    """child process: every row of environment `env_index` through hip.attention_plan(), results to out_path"""
    import ctypes
    sys.path.insert(0, ROOT)
    from madtp_amd import hip
    z = np.load(path)
    cols = [str(c) for c in z["input_cols"]]
    rows = z["inputs"][:, z["inputs"][cols.index("env")] == env_index].T
    assert list(z["plan_cols"]) == list(hip.ATTN_PLAN_FIELDS)
    at = {c: cols.index(c) for c in cols}
    out = np.zeros((len(rows), len(hip.ATTN_PLAN_FIELDS) + 1), dtype=np.int32)
    buf = (ctypes.c_int32 * len(hip.ATTN_PLAN_FIELDS))()
    for i, r in enumerate(rows.tolist()):
        got, launches = _plan_call(hip, r, at, buf)
        out[i] = got + [launches]
    np.save(out_path, out)


def test_every_recorded_decision_is_reproduced(golden, tmp_path):
    z, inputs, plans = golden
    envs = [str(e) for e in z["envs"]]
    assert sorted(set(inputs["env"].tolist())) == list(range(len(envs))) and len(envs) <= 16
    procs = []
    for e, setting in enumerate(envs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MADTP_ATTN_")}
        env["OMP_NUM_THREADS"] = "1"  # (all children at once: none of them needs a thread pool)
        if setting:
            k, v = setting.split("=")
            env[k] = v
        out = str(tmp_path / f"plan{e}.npy")
        code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_attn_plan_cpu import _replay; _replay({GOLDEN!r}, {e}, {out!r})"
        procs.append((setting, out, subprocess.Popen([sys.executable, "-c", code], env=env, cwd=ROOT)))
    want_all = np.concatenate([z["plans"].T, z["launches"].astype(np.int32)[:, None]], axis=1)
    fields = [str(c) for c in z["plan_cols"]] + ["launches"]
    try:
        for e, (setting, out, p) in enumerate(procs):
            assert p.wait(timeout=300) == 0, f"replay of {setting or 'the default environment'} failed"
            got, want = np.load(out), want_all[inputs["env"] == e]
            assert got.shape == want.shape
            bad = np.nonzero((got != want).any(axis=1))[0]
            rows = z["inputs"].T[inputs["env"] == e]
            assert len(bad) == 0, (f"{len(bad)} of {len(want)} decisions differ under {setting or 'the default environment'}; first: inputs "
                                   f"{dict(zip(inputs, rows[bad[0]].tolist()))} recorded {dict(zip(fields, want[bad[0]].tolist()))} "
                                   f"planned {dict(zip(fields, got[bad[0]].tolist()))}")
    finally:
        for _, _, p in procs:  # (a child that outlived its time limit, or the ones behind a failed one)
            if p.poll() is None:
                p.kill()


# Every kernel instantiation of the parent's attention code object, as INSTANCE tuples: the key-tile ladders per family, with and
# without scores; attn_bf16_kernel's HS / RB follow from (scores, NT); attn_large_kernel exists for both storage types; the
# three-sweep order is one more instantiation of the 8-chunk attn_bf16_large_kernel with scores, per operand format.
def _parent_instances():
    inst = set()
    for s in (0, 1):
        inst |= {(0, nt, 0, s, 0, 1, 1, 1) for nt in (2, 4, 6, 8, 10, 12, 13, 16)}
        inst |= {(1, nt, 0, s, 0, 1, 1, 1) for nt in (2, 4, 6, 8, 10, 13, 16)}
        inst |= {(2, nt, 0, s, f, 2 if s and nt <= 8 else 1, 2 if s and nt > 8 else 1, 1) for nt in (4, 6, 8, 10, 12, 13, 16) for f in (0, 1)}
        inst |= {(4, nch, st, s, 0, 1, 1, 1) for nch in (5, 8) for st in (0, 1)}
        inst |= {(5, nch, 0, s, 0, 1, 1, 1) for nch in (5, 8)}
        inst |= {(6, nch, 0, s, f, 1, 1, 1) for nch in (3, 5, 8) for f in (0, 1)}
    inst |= {(3, 0, 0, 1, f, 1, 1, 1) for f in (0, 1)}
    inst |= {(6, 8, 0, 1, f, 1, 1, 2) for f in (0, 1)}
    return inst


def test_fixture_covers_the_policy(golden):
    """a thinned fixture must not pass: the sweep, every kernel instantiation and every kind of decision are in it"""
    from madtp_amd import hip
    z, i, p = golden
    ok = p["status"] == 0
    envs = [str(e) for e in z["envs"]]
    assert envs[0] == ""
    for s in ("MADTP_ATTN_HEAD_SPLIT=0", "MADTP_ATTN_HV=0", "MADTP_ATTN_HEAD_GROUPS=2", "MADTP_ATTN_HEAD_GROUPS=3", "MADTP_ATTN_HEAD_GROUPS=4",
              "MADTP_ATTN_F16S=0", "MADTP_ATTN_LARGE_F32=1", "MADTP_ATTN_PAIR=0"):
        assert (i["env"] == envs.index(s)).sum() >= 1000, s
    assert (i["env"] == 0).sum() >= 1000
    fl = i["flags"]
    has = lambda bit: (fl & bit) != 0
    scores, pair = has(hip.ATTN_PLAN_SCORES), has(hip.ATTN_PLAN_PAIR)
    assert ((pair == 1) == (i["entry"] == 1)).all()
    for res in (0, 1, 2, 3):  # the resource flags, each false with the other true and both false
        assert (i["res"] == res).sum() >= 100, res
    assert (ok & (i["res"] == 0) & scores & (p["gz"] == 1)).any()
    for dt in (F32, BF16, F16S, F16):
        for s in (False, True):
            assert (ok & (i["io_dtype"] == dt) & (scores == s)).sum() >= 1000, (dt, s)
    # every key count, self-attention with scores and cross-attention at 20 queries, plain calls of the default environment
    plain = (i["env"] == 0) & (i["entry"] == 0) & (i["res"] == 3) & (i["B"] == 2) & (i["H"] == 12) & (i["kv_block_rows"] == 0) & (i["split_req"] == 0)
    for dt in (F32, BF16, F16S, F16):
        self_sc = plain & (fl == hip.ATTN_PLAN_SCORES) & (i["io_dtype"] == dt) & (i["Nq"] == i["Nk"])
        cross = plain & (fl == 0) & (i["io_dtype"] == dt) & (i["Nq"] == 20)
        assert set(range(1, 1026)) <= set(i["Nk"][self_sc].tolist()), dt
        assert set(range(1, 1026)) <= set(i["Nk"][cross].tolist()), dt
    # row blocks of the launch on both sides of each threshold of the head spread and the head split
    wgs = i["B"] * ((i["Nq"] + 63) // 64)
    for thr in (128, 384, 512):
        for s in (False, True):
            for w in (thr - 1, thr, thr + 1):
                assert (ok & (i["env"] == 0) & (scores == s) & (wgs == w)).any(), (thr, s, w)
    assert {1, 2, 3, 12, 16, 20} <= set(i["H"][ok].tolist())
    for H in (1, 2, 3, 12, 16, 20):
        assert (ok & scores & (i["H"] == H) & (i["Nk"] > 640)).any() and (ok & ~scores & (i["H"] == H)).any(), H
    assert (ok & has(hip.ATTN_PLAN_MASK_QK)).any() and (has(hip.ATTN_PLAN_MASK_QK) & (p["status"] == -2)).any()
    ndev = has(hip.ATTN_PLAN_N_DEV)
    assert (ok & ndev & has(hip.ATTN_PLAN_DEV_Q_ONLY)).any() and (ok & ndev & ~has(hip.ATTN_PLAN_DEV_Q_ONLY)).any()
    assert (ok & ndev & scores & (i["Nk"] <= 32) & (i["io_dtype"] == BF16) & (p["family"] == 2)).any()  # the small kernel's exclusion
    assert (ok & (i["kv_block_rows"] > i["Nk"])).any() and ((i["kv_block_rows"] > 0) & (p["status"] == -2)).any()
    assert (ok & has(hip.ATTN_PLAN_KV_INDEX)).any() and (ok & has(hip.ATTN_PLAN_ADD_MASK)).any()
    split = i["split_req"] > 0
    f16s_off = i["env"] == envs.index("MADTP_ATTN_F16S=0")
    assert (ok & split & ~f16s_off & (p["split_dim"] > 0) & (p["family"] == 1)).any() and (ok & split & (p["family"] == 5)).any()
    assert (split & f16s_off & (i["io_dtype"] == F16S) & (p["status"] == -1)).any() and (i["split_req"] < 0).any()
    assert (ok & f16s_off & (i["io_dtype"] == F16S) & (p["family"] == 0)).any()
    one = pair & ok & (z["launches"] == 1)
    assert one.any() and (p["gy"][one] == 2 * i["B"][one]).all() and (pair & ok & (z["launches"] == 2)).any()
    assert (pair & (p["status"] != 0) & (z["launches"] == 1)).any()  # (the second of two launches refused)
    for bit in (hip.ATTN_PLAN_QKV_UNALIGNED, hip.ATTN_PLAN_OUT_UNALIGNED16, hip.ATTN_PLAN_OUT_UNALIGNED8, hip.ATTN_PLAN_PAIR_UNALIGNED,
                hip.ATTN_PLAN_PAIR_MASKS_DIFFER, hip.ATTN_PLAN_NULL_PTR, hip.ATTN_PLAN_NO_P0, hip.ATTN_PLAN_NO_ONORM):
        assert has(bit).sum() >= 16, bit
    assert (ok & has(hip.ATTN_PLAN_OUT_UNALIGNED16) & (i["io_dtype"] == F16S) & (p["family"] == 0)).any()  # f16x3 falls back to the exact kernel
    assert (has(hip.ATTN_PLAN_OUT_UNALIGNED8) & split & (p["status"] == -4)).any()
    assert {-1, -2, -3, -4} == set(p["status"][p["status"] < 0].tolist())
    # head split, the minimisation's three outcomes, the three-sweep order and its fallbacks
    assert (ok & (p["family"] == 0) & (p["need_hm"] == 1)).any() and (ok & (p["family"] == 1) & (p["need_hm"] == 1)).any()
    assert {2, 3, 4} <= set(p["gz"][ok & (i["env"] == 0) & (p["family"] == 6) & (p["need_hm"] == 1)].tolist())
    assert (ok & (p["hv"] == 2) & (p["need_opart"] == 1)).any() and (ok & (i["res"] == 1) & (p["family"] == 6) & (p["nt"] == 8) & (p["hv"] == 1)).any()
    assert (ok & (p["family"] == 2) & (p["lds"] * 2 == p["lds_optin"])).any()  # the half ring of the one-head-per-workgroup cross launch
    seen = set(zip(*[p[c][ok].tolist() for c in INSTANCE]))
    assert seen == _parent_instances(), (sorted(_parent_instances() - seen), sorted(seen - _parent_instances()))


def test_plan_query_argument_check(golden):
    from madtp_amd import hip
    lib = hip.load()
    assert lib.madtp_attention_plan(2, 12, 197, 197, 2304, 2304, 2304, 768, 1, 0, 0, 0, 2, 3, None, len(hip.ATTN_PLAN_FIELDS) - 1) == -1
    plan = dict(zip(hip.ATTN_PLAN_FIELDS, hip.attention_plan(2, 12, 197, 197, 2304, 2304, 2304, 768, hip.BF16, flags=hip.ATTN_PLAN_SCORES)))
    assert len(plan) == len(hip.ATTN_PLAN_FIELDS) and plan["status"] == 0 and hip.ATTN_FAMILIES[plan["family"]] == "attn_bf16_kernel"


# ---- what the GPU attention tests reach ----------------------------------------------------------------------------------------------
def _params(fn, names):
    """the value lists of a test's parametrize marks, by argument names"""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == names:
            return list(m.args[1])
    raise KeyError(names)


def _gpu_test_plans(hip):
    """(test, case, plan) of every launch shape of the GPU attention tests of tests/test_kernels_gpu.py, planned as those tests call"""
    from tests import test_kernels_gpu as t
    esz = {F32: 4, BF16: 2, F16S: 4, F16: 2}
    out = []

    def plan(test, case, B, H, Nq, Nk, io, ld, flags, ldm=0):
        # (torch allocations are 256-byte aligned and every column slice of these tests starts at a multiple of 64 elements)
        assert all((l * esz[io]) % 16 == 0 for l in ld)
        r = dict(zip(hip.ATTN_PLAN_FIELDS, hip.attention_plan(B, H, Nq, Nk, *ld, H * 64, io, ld_mask_qk=ldm, flags=flags)))
        if r["status"] == hip.ATTN_PAIR_TWO_LAUNCHES:
            r = dict(zip(hip.ATTN_PLAN_FIELDS, hip.attention_plan(B, H, Nq, Nk, *ld, H * 64, io, flags=flags & ~hip.ATTN_PLAN_PAIR)))
        assert r["status"] == 0, (test, case, r)
        out.append((test, case, r))

    dts = {"f32": F32, "bf16": BF16, "f16": F16, "f16x3": F16S}
    sc = hip.ATTN_PLAN_SCORES
    for B, N, H in _params(t.test_self_attention_with_scores, "B,N,H"):
        for d in _params(t.test_self_attention_with_scores, "dtype"):
            for m in (0, hip.ATTN_PLAN_ADD_MASK):
                plan("self_attention_with_scores", (B, N, H, d), B, H, N, N, dts[d], [3 * H * 64] * 3, sc | m)
    for B, L, Nk in _params(t.test_cross_attention, "B,L,Nk"):
        for d in _params(t.test_cross_attention, "dtype"):
            plan("cross_attention", (B, L, Nk, d), B, 12, L, Nk, dts[d], [768, 1536, 1536], 0)
    for d, Nq, Nk in _params(t.test_attention_pair, "dtype,Nq,Nk"):
        for fl in (hip.ATTN_PLAN_PAIR, 0):  # the pair and the two plain calls it is compared with
            plan("attention_pair", (d, Nq, Nk), 5, 12, Nq, Nk, dts[d], [1536] * 3, fl | hip.ATTN_PLAN_ADD_MASK)
    for B, N, H in _params(t.test_attention_f16_split_products, "B,N,H"):
        for io in (F32, F16S):
            for fl, ldm in ((0, 0), (hip.ATTN_PLAN_ADD_MASK, 0)) + (((hip.ATTN_PLAN_MASK_QK, N),) if N <= 256 else ()):
                plan("attention_f16_split_products", (B, N, H), B, H, N, N, io, [3 * H * 64] * 3, sc | fl, ldm)
    for B, N, H in _params(t.test_self_attention_f16_operands, "B,N,H"):
        plan("self_attention_f16_operands", (B, N, H), B, H, N, N, F16, [3 * H * 64] * 3, sc)
    return out


def _reachable_by_default(hip):
    """every kernel instantiation the exported entries can start in the default environment: all key counts, formats, with and
    without scores, one and many row blocks, even and odd and more than 16 heads"""
    seen = set()
    buf = None
    for io in (F32, BF16, F16S, F16):
        for flags in (0, hip.ATTN_PLAN_SCORES, hip.ATTN_PLAN_PAIR, hip.ATTN_PLAN_SCORES | hip.ATTN_PLAN_MASK_QK):
            for Nk in range(1, 1025):
                if flags & hip.ATTN_PLAN_MASK_QK and Nk > 256:
                    continue
                for B, H in ((1, 12), (1, 20), (600, 3)):
                    r = hip.attention_plan(B, H, Nk if flags & hip.ATTN_PLAN_SCORES else 20, Nk, 3 * H * 64, 3 * H * 64, 3 * H * 64, H * 64, io, ld_mask_qk=Nk,
                                           flags=flags)
                    if r[0] == 0:
                        seen.add(tuple(r[hip.ATTN_PLAN_FIELDS.index(c)] for c in INSTANCE))
    return seen


def test_gpu_attention_tests_reach_every_default_instantiation(golden):
    """The shape lists of the GPU attention tests, planned on the CPU: together they start every kernel instantiation that
    madtp_attention, madtp_attention_qk_mask and madtp_attention_pair can start in the default environment - and the launches that
    the comments in those lists name are the ones the planner gives."""
    from madtp_amd import hip
    assert not any(k.startswith("MADTP_ATTN_") for k in os.environ)
    plans = _gpu_test_plans(hip)
    hit = {tuple(r[c] for c in INSTANCE) for _, _, r in plans}
    reachable = _reachable_by_default(hip)
    assert reachable == {x for x in _parent_instances() if x[:3] != (4, 5, 1) and x[:3] != (4, 8, 1)}  # (bf16 storage on the exact kernel: a switch)
    missing = sorted(reachable - hit)
    assert not missing, [dict(zip(INSTANCE, m), family=hip.ATTN_FAMILIES[m[0]]) for m in missing]
    # the comments of test_self_attention_with_scores' list
    by_case = {(t, c): r for t, c, r in plans}
    for d in ("f32", "bf16"):
        for case in ((2, 700, 12), (1, 901, 12)):  # 641..1024 keys, all heads: the three-sweep order (bf16 storage)
            r = by_case["self_attention_with_scores", case + (d,)]
            assert (hip.ATTN_FAMILIES[r["family"]], r["nt"], r["hv"], r["need_opart"]) == (("attn_bf16_large_kernel", 8, 2, 1) if d == "bf16" else
                                                                                          ("attn_large_kernel", 8, 1, 0)), (case, d)
        for case, gz in (((16, 320, 12), 4 if d == "bf16" else 1), ((24, 96, 12), 1 if d == "bf16" else 2), ((4, 300, 3), 1)):
            r = by_case["self_attention_with_scores", case + (d,)]  # head split on many row blocks; an odd head count: no split
            assert (r["gz"], r["need_hm"]) == (gz, int(gz > 1)), (case, d, r)
