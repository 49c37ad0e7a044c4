"""What tests/test_gemm_small_gpu.py reaches, checked on the planner (no GPU): every launch of tests/gemm_small_cases.py is planned
with hip.gemm_plan() exactly as the GPU test launches it - same leading dimensions, flags, forced configuration and stream
attributes (on a made-up stream pointer) - and the table as a whole must reach every gemm_kernel instantiation the planner can
reach, each with the vector and with the scalar epilogue, with workgroups that walk several tiles and uneven XCD shares."""
import pytest

from tests import gemm_small_cases as C

STREAM = 0x7A5000  # a made-up stream pointer that carries the attributes of the GPU test's stream


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    lib = h.load()
    assert lib.madtp_stream_set_sched(STREAM, *C.STREAM_SCHED) == 0
    return h


def _plan(hip, cfg, args, sched):
    with hip.gemm_config(cfg):
        return C.plan(args, STREAM if sched == "stream" else None)


@pytest.fixture(scope="module")
def plans(hip):
    return [(c, _plan(hip, c.cfg, C.plan_args(c), c.sched)) for c in C.cases()]


def test_every_case_plans_to_its_variant(plans):
    assert len(plans) == len(C.PAIRS) * len(C.CONFIGS) * (len(C.SHAPES) * 2 + 2 * (len(C.EPILOGUES) - 1))
    for c, p in plans:
        assert p["status"] == 0 and p["kernel"] == 0, (c, p)
        v = C.variant_of(c.operand, c.cfg)
        assert p["variant"] == v and (p["rows"], p["cols"]) == C.TILES[v][:2], (c, p)
        assert p["mode"] == C.MODE[c.operand] and p["om"] == C.OM[c.output] and p["desc"] == 1, (c, p)


def test_table_has_every_shape_pair_and_configuration(plans):
    """(a thinned table must not pass)"""
    assert set(C.SHAPES) == {(328, 840, 192), (328, 844, 64), (70, 200, 128)} and C.WALKED == C.SHAPES[:2]
    assert set(C.PAIRS) == {("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"), ("f16", "f32"), ("f16", "f16"),
                            ("f16s", "f32"), ("f16s", "f16s")}
    assert C.CONFIGS == (1, 2, 3, 4) and C.SCHEDS == ("chip", "stream") and C.STREAM_SCHED == (1, 0.0, -2)
    assert set(C.EPILOGUES) == {"linear", "nobias", "gelu", "relu", "quick_gelu", "out_scale", "residual", "lda", "nan_tail", "strided", "ldc_odd"}
    for pair in C.PAIRS:
        for cfg in C.CONFIGS:
            mine = [c for c, _ in plans if (c.operand, c.output, c.cfg) == (*pair, cfg)]
            assert {(c.shape, c.sched) for c in mine if c.epi == "linear"} == {(s, k) for s in C.SHAPES for k in C.SCHEDS}
            assert {(c.shape, c.epi) for c in mine if c.sched == "stream"} >= {(s, e) for s in C.WALKED for e in C.EPILOGUES}
    e = {n: C.epi(C.Case("f32", "f32", 1, C.SHAPES[0], "stream", n)) for n in C.EPILOGUES}
    assert not e["nobias"]["bias"] and e["out_scale"]["out_scale"] == 0.5 and e["residual"]["residual"]
    assert [e[n]["act"] for n in C.ACTS] == list(C.ACTS) and e["lda"]["a"] == "slice" and e["nan_tail"]["a"] == "nan_tail"
    assert e["strided"]["out"] == e["ldc_odd"]["out"] == "strided" and (e["strided"]["pad_cols"], e["ldc_odd"]["pad_cols"]) == (24, 20)


def test_every_reachable_instantiation_is_reached_with_both_epilogues(hip, plans):
    reachable = set()
    for a, o in C.PAIRS:
        for cfg in C.CONFIGS:
            for M, N, K in C.SHAPES:
                p = _plan(hip, cfg, C.plan_args(C.Case(a, o, cfg, (M, N, K), "chip", "linear")), "chip")
                assert p["status"] == 0 and p["kernel"] == 0
                reachable.add((p["mode"], p["om"], p["variant"]))
    # 4 operand formats x 2 outputs x 4 variants, minus the two 128x128 f16-split instantiations (gemm_plan: x3 && cfg == 0 -> 1)
    assert len(reachable) == 30
    assert {(m, om, v) for m, om, v in ((2, 0, 0), (2, 2, 0))}.isdisjoint(reachable)
    for fast in (1, 0):
        got = {(p["mode"], p["om"], p["variant"]) for _, p in plans if p["fast_epi"] == fast}
        assert got == reachable, (fast, sorted(reachable - got))
    # a residual next to a 2-byte output: the scalar epilogue (the vector one adds a residual to f32 outputs only; the launch sends
    # an f16-split output with a residual to the scalar epilogue as well, whatever the plan says: gemm_launch)
    for c, p in plans:
        if c.epi == "residual":
            assert p["fast_epi"] == (1 if c.output in ("f32", "f16s") and c.shape[1] % 8 == 0 else 0), (c, p)
        elif c.epi == "strided":
            assert p["fast_epi"] == (1 if c.shape[1] % 8 == 0 else 0), (c, p)  # (the padded leading dimension stays a multiple of 8)
        elif c.epi == "ldc_odd":
            assert p["fast_epi"] == 0 and (C.plan_args(c)["ldc"] % 8 == 4 or c.shape[1] % 8), (c, p)  # the vector epilogue's shape too


def test_stream_cases_walk_tiles_with_uneven_xcd_shares(plans):
    seen = set()
    for c, p in plans:
        tiles = p["ntm"] * p["ntn"]
        if c.sched == "stream" and c.shape in C.WALKED:
            assert tiles > p["grid"] and tiles % 8 != 0 and p["grid"] in (16, 24), (c, p)
            assert 2 <= -(-tiles // p["grid"]) <= 4, (c, p)
            seen.add((c.operand, c.output, p["variant"]))
        if c.sched == "chip":
            assert p["grid"] == 8 * ((tiles + 7) // 8), (c, p)  # one tile per workgroup at the most
        if c.shape == C.SHAPES[2]:
            assert tiles < 8 or p["variant"] == 3, (c, p)  # XCDs without a tile (the 64x64 variant has 8 tiles for 8 XCDs: one each)
    assert len(seen) == 30


def test_slab_counts(plans):
    """K = 64 / 128 / 192: 1, 2 and 3 slabs of 2-byte operands, 2, 4 and 6 of f32 operands and f16-split steps.  The shortest tile is
    no longer than the 3-stage ring's two prefetches (its prologue reaches into the next tile); the longest stream is longer than every
    ring, except the 3-stage ring on plain 2-byte operands, which it fills exactly."""
    for operand in C.OPERANDS:
        steps = sorted(K * C.ESZ[operand] // 128 * (2 if operand == "f16s" else 1) for _, _, K in C.SHAPES)
        assert steps == ([1, 2, 3] if operand in ("bf16", "f16") else [2, 4, 6]), operand
        assert steps[0] <= max(stages for _, _, stages in C.TILES) - 1
        for rows, cols, stages in C.TILES:
            assert steps[-1] >= stages
            assert steps[-1] >= stages + 1 or (operand in ("bf16", "f16") and stages == 3)


def test_small_tile_hint_plans_the_forced_variant(hip):
    """test_small_tile_hint_equals_forced_configuration on the GPU compares a hinted launch with a forced one: the same plan"""
    lib = hip.load()
    for v in range(4):
        hinted = STREAM + 0x100 * (v + 1)
        assert lib.madtp_stream_set_sched(hinted, C.STREAM_SCHED[0], C.STREAM_SCHED[1], v) == 0
        for shape in C.WALKED:
            args = C.plan_args(C.Case("bf16", "f32", 0, shape, "stream", "linear"))
            with hip.gemm_config(0):
                p = C.plan(args, hinted)
            assert p["variant"] == v and p == _plan(hip, v + 1, args, "stream"), (v, shape, p)


def _splitk_variant(c):
    if c.cfg:
        return C.variant_of(c.operand, c.cfg)
    if c.operand == "f32":
        return 0
    # automatic: the smallest tile whose slots fit one round of three workgroups per CU - 768 on the chip, 24 on the stream
    if c.sched == "chip" or c.shape == C.SPLITK_SHAPES[0]:
        return 3
    return 1 if c.operand == "f16s" else 0


def test_splitk_cases(hip):
    cases = C.splitk_cases()
    assert len(cases) == 4 * 5 * 2 * 2 and set(C.SPLITK_SHAPES) == {(70, 200, 256, 2), (130, 264, 512, 4)}
    assert C.SPLITK_CONFIGS == (0, 1, 2, 3, 4) and C.SPLITK_WALKED == (130, 264, 512, 4)
    variants = set()
    for c in cases:
        p = _plan(hip, c.cfg, C.splitk_plan_args(c), c.sched)
        assert p["status"] == 0 and p["kernel"] == 0 and p["fast_epi"] == 1 and p["om"] == 0 and p["mode"] == C.MODE[c.operand], (c, p)
        assert p["variant"] == _splitk_variant(c), (c, p)
        variants.add((p["mode"], p["variant"]))
        M, N, K, S = c.shape
        assert (K * C.ESZ[c.operand] // 128) % S == 0
        slots = p["ntm"] * p["ntn"] * S
        if c.sched == "stream" and c.shape == C.SPLITK_WALKED:
            assert slots >= 24 and slots > p["grid"] and p["grid"] in (16, 24), (c, p)
    assert len(variants) == 15  # 4 operand formats x 4 variants minus f16-split 128x128
