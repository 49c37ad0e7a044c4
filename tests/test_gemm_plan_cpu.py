"""The GEMM dispatch policy against the decisions recorded from the commit before the planner existed (no GPU).

tests/golden/gemm_plan_parent.npz holds, one row per column, the inputs of ~330 k madtp_gemm / madtp_gemm_pair / madtp_gemm_splitk
calls and what the old gemm_launch decided for each: kernel, tile, grid, tile order, stream-K tail, descriptor and epilogue
flags, or the status it returned.  Every one of them is replayed through hip.gemm_plan() and must come out field for field the
same.  Rows are stored in replay order: by environment setting, and within one the rows that leave madtp_gemm_set_config alone
first.  The library reads its environment switches once, so every setting is replayed in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plan_parent.npz")
PAIR = 1  # flags bit (hip.PLAN_PAIR)


@pytest.fixture(scope="module")
def golden():
    from madtp_amd import build
    build.build(verbose=False)
    z = np.load(GOLDEN)
    inputs = dict(zip([str(c) for c in z["input_cols"]], z["inputs"]))
    plans = dict(zip([str(c) for c in z["plan_cols"]], z["plans"]))
    return z, inputs, plans


def _replay(path, env_index, out_path):
    """child process: every row of environment `env_index` through hip.gemm_plan(), results to out_path"""
    import ctypes
    sys.path.insert(0, ROOT)
    from madtp_amd import hip
    z = np.load(path)
    cols = [str(c) for c in z["input_cols"]]
    rows = z["inputs"][:, z["inputs"][cols.index("env")] == env_index].T
    assert list(z["plan_cols"]) == list(hip.PLAN_FIELDS)
    lib = hip.load()
    out = np.zeros((len(rows), len(hip.PLAN_FIELDS)), dtype=np.int32)
    bufs = (ctypes.c_int32 * out.shape[1] * len(rows)).from_buffer(out)
    at = {c: cols.index(c) for c in cols}
    args = [at[c] for c in ("M", "N", "K", "lda", "ldw", "ldc", "ldr", "ab", "c", "splitk", "flags")]
    streams, forced = {}, None
    for i, r in enumerate(rows.tolist()):
        force = r[at["force"]]
        assert force >= 0 or forced is None
        if force >= 0 and force != forced:
            forced = force
            lib.madtp_gemm_set_config(forced)
        stream = None
        if r[at["stream"]]:  # a made-up stream pointer that carries the recorded attributes
            key = (r[at["cus"]], r[at["cost_milli"]], r[at["small"]])
            if key not in streams:
                streams[key] = 0x1000 + 0x100 * len(streams)
                assert lib.madtp_stream_set_sched(streams[key], key[0], key[1] / 1000.0, key[2]) == 0
            stream = streams[key]
        hip.gemm_plan(*[r[j] for j in args], stream, out=bufs[i])
    np.save(out_path, out)


def test_every_recorded_decision_is_reproduced(golden, tmp_path):
    z, inputs, plans = golden
    envs = [str(e) for e in z["envs"]]
    assert sorted(set(inputs["env"].tolist())) == list(range(len(envs)))
    procs = []
    for e, setting in enumerate(envs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("MADTP_GEMM_")}
        env["OMP_NUM_THREADS"] = "1"  # (sixteen children at once: none of them needs a thread pool)
        if setting:
            k, v = setting.split("=")
            env[k] = v
        out = str(tmp_path / f"plan{e}.npy")
        code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gemm_plan_cpu import _replay; _replay({GOLDEN!r}, {e}, {out!r})"
        procs.append((setting, out, subprocess.Popen([sys.executable, "-c", code], env=env, cwd=ROOT)))
    want_all = z["plans"].T
    try:
        for e, (setting, out, p) in enumerate(procs):
            assert p.wait(timeout=300) == 0, f"replay of {setting or 'the default environment'} failed"
            got, want = np.load(out), want_all[inputs["env"] == e]
            assert got.shape == want.shape
            bad = np.nonzero((got != want).any(axis=1))[0]
            rows = z["inputs"].T[inputs["env"] == e]
            assert len(bad) == 0, (f"{len(bad)} of {len(want)} decisions differ under {setting or 'the default environment'}; first: inputs "
                                   f"{dict(zip(inputs, rows[bad[0]].tolist()))} recorded {want[bad[0]].tolist()} planned {got[bad[0]].tolist()}")
    finally:
        for _, _, p in procs:  # (a child that outlived its time limit, or the ones behind a failed one)
            if p.poll() is None:
                p.kill()


def test_fixture_covers_the_policy(golden):
    """a thinned fixture must not pass: the sweep, every kernel and every kind of decision are in it"""
    z, i, p = golden
    ok = p["status"] == 0
    envs = [str(e) for e in z["envs"]]
    for s in ("MADTP_GEMM_TABLE=0", "MADTP_GEMM_TABLE=2", "MADTP_GEMM_PP=0", "MADTP_GEMM_SQ=0", "MADTP_GEMM_SK=1", "MADTP_GEMM_PAIR=0",
              "MADTP_GEMM_NGRP=0", "MADTP_GEMM_NGRP=3", "MADTP_GEMM_BIG_MIN_M=1024", "MADTP_GEMM_BIG_MIN_TILES=100",
              "MADTP_GEMM_WG_PER_XCD=64", "MADTP_GEMM_DESC=0", "MADTP_GEMM_SQ_COST=0.9", "MADTP_GEMM_SMALL_CFG=0", "MADTP_GEMM_CFG=6"):
        assert (i["env"] == envs.index(s)).sum() >= 1000, s
    plain = (i["env"] == 0) & (i["entry"] == 0) & (i["flags"] == 0) & (i["force"] < 0) & (i["stream"] == 0)
    plain &= (i["lda"] == np.where(i["ab"] == 2, 2, 1) * i["K"]) & (i["ldw"] == i["lda"]) & (i["ldc"] == np.where(i["c"] == 2, 2, 1) * i["N"])
    m_sweep = {1, 64, 197, 300, 1280, 3000, 4095, 4096, 4097, 4480} | {64 * k for k in range(63, 513)} | {64 * k + 1 for k in range(63, 513)}
    nk = [(2304, 768), (768, 768), (3072, 768), (768, 3072), (1536, 768), (3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096), (1024, 640),
          (776, 768), (1100, 1024), (100, 768), (768, 192), (768, 64), (18432, 768), (8192, 8192)]
    for ab, c in ((1, 1), (1, 0), (3, 3), (3, 0), (2, 2), (2, 0), (0, 0), (0, 1)):  # operand -> output classes
        cls = plain & (i["ab"] == ab) & (i["c"] == c)
        for N, K in nk:
            sel = cls & (i["N"] == N) & (i["K"] == K)
            assert m_sweep <= set(i["M"][sel].tolist()), (ab, c, N, K)
    assert set(range(11)) <= set(i["force"].tolist())
    assert {(32, -1000, -2), (32, 900, 0), (16, -1000, -2), (8, 900, 0)} <= set(zip(i["cus"][i["stream"] == 1].tolist(), i["cost_milli"][i["stream"] == 1].tolist(),
                                                                                   i["small"][i["stream"] == 1].tolist()))
    assert {1, 2, 4} <= set(i["splitk"][i["entry"] == 2].tolist())
    mdev = (i["flags"] & 8) != 0
    assert (mdev & (i["M"] < 4096) & ok).any() and (mdev & (i["M"] == 4096) & (p["status"] == -2)).any()
    # every kernel, every small-tile variant, both ping-pong tile heights
    assert set(p["kernel"][ok].tolist()) == {0, 1, 2, 3}
    assert set(p["variant"][ok & (p["kernel"] == 0)].tolist()) == {0, 1, 2, 3}
    assert set(p["rows"][ok & (p["kernel"] == 3)].tolist()) == {192, 256}
    # table hits (a table shape with the default environment picks per 64-row bucket) and cost-model decisions (beyond the table / off it)
    auto_big = plain & ok & (i["M"] >= 4096) & (i["ab"] == 1) & (i["c"] == 1)
    tab = auto_big & (i["N"] == 2304) & (i["K"] == 768) & (i["M"] <= 32768)
    assert set(p["kernel"][tab].tolist()) == {3} and set(p["rows"][tab].tolist()) == {192, 256} and tab.sum() >= 800
    model = auto_big & (i["N"] == 3072) & (i["K"] == 1024)
    assert model.sum() >= 800 and len(set(p["kernel"][model].tolist())) >= 2
    assert (ok & (i["env"] == envs.index("MADTP_GEMM_TABLE=0")) & (p["kernel"] >= 1)).any()
    for k in (1, 3):  # column groups on both big kernels
        assert (ok & (p["kernel"] == k) & (p["ngrp"] > 0)).any(), k
    pair = (i["flags"] & PAIR) != 0
    assert (pair & ok & (p["kernel"] == 1)).any() and (pair & (p["status"] == 1000)).any()
    assert (ok & (p["sk"] == 1)).any()
    assert {-1, -2, -3, -4} <= set(p["status"].tolist())
    assert (ok & (p["desc"] == 0)).any() and (ok & (p["fast_epi"] == 0)).any() and (ok & (p["fast_epi"] == 1)).any()


def test_plan_query_argument_check(golden):
    from madtp_amd import hip
    lib = hip.load()
    assert lib.madtp_gemm_plan(64, 64, 64, 64, 64, 64, 0, 1, 1, 1, 0, None, None, 15) == -1
    plan = hip.gemm_plan(1280, 768, 768, 768, 768, 768, 0, hip.BF16, hip.BF16)
    assert len(plan) == len(hip.PLAN_FIELDS) and dict(zip(hip.PLAN_FIELDS, plan))["status"] == 0
