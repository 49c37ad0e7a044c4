"""What tests/test_gemm_big_gpu.py reaches, checked on the planner (no GPU): every launch of tests/gemm_big_cases.py is planned with
hip.gemm_plan() exactly as the GPU test launches it - same leading dimensions, flags, forced configuration and stream attributes (on
a made-up stream pointer) - and the table as a whole must reach every instantiation of the three big-tile kernels outside the
ablation build, each with the vector and with the scalar epilogue, with workgroups that walk several tiles, the column-group tile
order on both tile widths, the shortest K loops and a stream-K tail of at least two uneven pieces."""
import pytest

from tests import gemm_big_cases as C

STREAM = 0x7B6000  # a made-up stream pointer that carries the attributes of the GPU test's stream


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


def _tiles(p):
    return p["ntm"] * p["ntn"]


def test_every_case_plans_to_its_kernel_tile_and_epilogue(plans):
    n_epi = len(C.EPILOGUES)
    per_id = {7: 4 * 2 + 2 * (n_epi - 1) + 2, 6: 4 * 2 + 2 * (n_epi - 1) + 2, 9: 3 * 2 + 2 * (n_epi - 1) + 2, 5: 2 * 2 + 2 * (n_epi - 1)}
    per_id[10] = per_id[9]
    assert len(plans) == sum(per_id[cfg] for cfg, _ in C.IDS) + 2 * n_epi
    for c, p in plans:
        M, N, K = c.shape
        rows, cols = C.TILE[c.cfg]
        assert p["status"] == 0 and p["kernel"] == C.KERNEL[c.cfg] and (p["rows"], p["cols"]) == (rows, cols), (c, p)
        assert (p["ntm"], p["ntn"]) == (-(-M // rows), -(-N // cols)), (c, p)
        assert p["mode"] == C.MODE[c.operand] and p["om"] == C.OM[c.output], (c, p)
        assert p["fast_epi"] == C.planned_fast_epi(c), (c, p)
        assert p["sk"] == (1 if c.shape == C.SK_SHAPE else 0), (c, p)
        want_ngrp = {C.GROUPED_256: 8, C.GROUPED_WS: 4}.get(c.shape, 0)
        assert p["ngrp"] == want_ngrp, (c, p)
        # the grid: one workgroup per XCD on the stream, on the chip one per tile up to 32 per XCD
        assert p["grid"] == 8 * min(-(-_tiles(p) // 8), 1 if c.sched == "stream" else 32), (c, p)
        assert p["lds"] == (3 * (256 + 128) * 128 if p["kernel"] == C.WS else 2 * (256 + 256) * 128), (c, p)
        # the leading dimensions the GPU test passes (it asserts its tensors' strides against the same plan_args)
        a = C.plan_args(c)
        ka, cn = (2 if c.operand == "f16s" else 1) * K, (2 if c.output == "f16s" else 1) * N
        assert a["lda"] == (3 * ka if c.epi == "lda" else ka) and a["ldw"] == ka, (c, a)
        assert a["ldc"] == cn + {"strided": 24, "ldc_odd": 20}.get(c.epi, 0) and a["ldr"] == (N if "residual" in c.epi else 0), (c, a)


def test_table_has_every_id_shape_epilogue_and_schedule(plans):
    """(a thinned table must not pass)"""
    assert C.CONFIGS == (7, 5, 6, 9, 10) and C.SCHEDS == ("chip", "stream") and C.STREAM_SCHED == (1, 0.0, -2)
    six = {("bf16", "f32"), ("bf16", "bf16"), ("f16", "f32"), ("f16", "f16"), ("f16s", "f32"), ("f16s", "f16s")}
    two = {("bf16", "f32"), ("bf16", "bf16")}
    assert {cfg: set(p) for cfg, p in C.PAIRS.items()} == {7: six, 9: six, 10: six, 6: two, 5: two}
    assert len(C.IDS) == 22 and set(C.IDS) == {(cfg, pr) for cfg in C.CONFIGS for pr in C.PAIRS[cfg]}
    assert C.SHAPES == ((1100, 776, 256), (1100, 780, 128), (300, 100, 64)) and C.WALKED == C.SHAPES[:2]
    assert C.GROUPED == {7: (300, 2056, 2304), 6: (300, 4104, 128), 9: (300, 4104, 128), 10: (300, 4104, 128)}
    assert list(C.EPILOGUES) == ["linear", "nobias", "gelu", "relu", "quick_gelu", "out_scale", "residual", "lda", "nan_tail", "strided", "ldc_odd",
                                 "scale_residual"]
    e = {n: C.epi(C.Case("bf16", "f32", 7, C.SHAPES[0], "stream", n)) for n in C.EPILOGUES}
    assert not e["nobias"]["bias"] and e["out_scale"]["out_scale"] == 0.5 and e["residual"]["residual"] and not e["out_scale"]["residual"]
    assert e["scale_residual"]["out_scale"] == 0.5 and e["scale_residual"]["residual"] and e["scale_residual"]["act"] is None
    assert [e[n]["act"] for n in C.ACTS] == list(C.ACTS) and e["lda"]["a"] == "slice" and e["nan_tail"]["a"] == "nan_tail"
    assert e["strided"]["out"] == e["ldc_odd"]["out"] == "strided" and (e["strided"]["pad_cols"], e["ldc_odd"]["pad_cols"]) == (24, 20)
    assert C.PAD_ROWS == 64 and C.NAN_ROWS == 40  # rows below M: sentinels below the output, NaN below A
    for cfg, pair in C.IDS:
        mine = [c for c, _ in plans if (c.cfg, c.operand, c.output) == (cfg, *pair) and c.shape != C.SK_SHAPE]
        shapes = set(C.WALKED) | ({C.ONE_SLAB} if cfg in (7, 6) else set()) | ({C.GROUPED[cfg]} if cfg in C.GROUPED else set())
        assert {(c.shape, c.sched) for c in mine if c.epi == "linear"} == {(s, k) for s in shapes for k in C.SCHEDS}, (cfg, pair)
        assert {(c.shape, c.epi) for c in mine if c.sched == "stream"} >= {(s, e) for s in C.WALKED for e in C.EPILOGUES}, (cfg, pair)
        if cfg in C.GROUPED:
            assert {(c.sched, c.epi) for c in mine if c.shape == C.GROUPED[cfg]} == {(k, e) for k in C.SCHEDS for e in ("linear", "residual")}
    for out in ("f32", "bf16"):
        assert {(c.epi, c.sched) for c, _ in plans if c.shape == C.SK_SHAPE and c.output == out} == {(e, "chip") for e in C.EPILOGUES}


def test_every_instantiation_is_reached_with_both_epilogues(plans):
    """gemm_launch_ws: 3 operand formats x 2 outputs; gemm_launch_sq: bf16 operands x 2 outputs; madtp_gemm_pp_launch: 3 x 2 on each of
    the two tile heights - 20 instantiations, each run with the vector and with the scalar epilogue, on the stream among others"""
    want = {(C.WS, 256, C.MODE[a], C.OM[o]) for a, o in C.PAIRS_ALL} | {(C.SQ, 256, C.MODE[a], C.OM[o]) for a, o in C.PAIRS_BF16}
    want |= {(C.PP, rows, C.MODE[a], C.OM[o]) for rows in (256, 192) for a, o in C.PAIRS_ALL}
    assert len(want) == 20
    for fast in (1, 0):
        for scheds in (C.SCHEDS, ("stream",)):
            got = {(p["kernel"], p["rows"], p["mode"], p["om"]) for c, p in plans if p["fast_epi"] == fast and c.sched in scheds}
            assert got == want, (fast, scheds, sorted(want - got))
    for c, p in plans:
        e = C.epi(c)
        # what the table means by the scalar epilogue: N % 8 != 0, a leading dimension of C that is no multiple of 8 at a vector
        # shape, a residual next to a 2-byte output - and, by the launch rather than the plan, next to an f16-split output
        scalar = c.shape[1] % 8 != 0 or c.epi == "ldc_odd" or (e["residual"] and c.output in ("bf16", "f16", "f16s"))
        assert C.scalar_epilogue(c) == scalar, c
        assert p["fast_epi"] == (0 if scalar and not (e["residual"] and c.output == "f16s" and C.planned_fast_epi(c)) else 1), (c, p)
        if c.epi == "ldc_odd":
            assert C.plan_args(c)["ldc"] % 8 == 4 or c.shape[1] % 8, c  # the vector epilogue's shape too
    # every combination the old tests never ran on a big tile is in the table, on every kernel and tile height
    for kernel, rows in ((C.WS, 256), (C.SQ, 256), (C.PP, 256), (C.PP, 192)):
        mine = [(c, C.epi(c)) for c, p in plans if (p["kernel"], p["rows"]) == (kernel, rows)]
        assert {(c.output, e["act"]) for c, e in mine} >= {(o, a) for o in ("f32", "bf16") for a in C.ACTS}
        assert {c.output for c, e in mine if e["residual"]} >= {"f32", "bf16"} | (set() if kernel == C.SQ else {"f16", "f16s"})
        assert any(e["residual"] and e["out_scale"] == 0.5 for c, e in mine)
        if kernel != C.SQ:
            assert {c.output for c, e in mine if c.operand == "f16" and e["out"] == "strided"} == {"f32", "f16"}
            assert {(c.operand, e["act"]) for c, e in mine if c.output == "f32"} >= {(a, act) for a in ("bf16", "f16", "f16s") for act in C.ACTS}


def test_stream_cases_walk_tiles(plans):
    """on the stream's grid of 8 every workgroup of the walked shapes gets 2 to 5 tiles, with uneven XCD shares"""
    seen = set()
    for c, p in plans:
        tiles = _tiles(p)
        if c.sched == "stream" and c.shape in C.WALKED:
            assert p["grid"] == 8 and tiles == {(256, 128): 35, (256, 256): 20, (192, 256): 24}[(p["rows"], p["cols"])], (c, p)
            shares = [(x + 1) * tiles // 8 - x * tiles // 8 for x in range(8)]  # xcd_tiles: tiles of the one workgroup of XCD x
            assert 2 <= min(shares) and max(shares) <= 5, (c, shares)
            assert len(set(shares)) == 2 or tiles == 24, (c, shares)
            seen.add((p["kernel"], p["rows"], p["mode"], p["om"]))
        if c.sched == "stream" and c.shape in C.GROUPED.values():
            assert p["grid"] == 8 and tiles == 34, (c, p)  # 2 row tiles x 17 column tiles: 4 or 5 per workgroup across the groups
        if c.sched == "chip" and c.shape != C.SK_SHAPE:
            assert p["grid"] == 8 * ((tiles + 7) // 8), (c, p)  # one tile per workgroup at the most
        if c.shape == C.ONE_SLAB:
            assert tiles == 2 and p["grid"] == 8, (c, p)  # XCDs without a tile
    assert len(seen) == 20


def test_ragged_tiles_and_slab_counts(hip, plans):
    M, N, K = C.SHAPES[0]
    assert (M % 256, M % 192, N % 128, N % 256, N % 8) == (76, 140, 8, 8, 0) and K // 128 == 2  # two slab pairs of the ping-pong kernel
    M, N, K = C.SHAPES[1]
    assert (M, N % 8, K // 128, K // 64) == (1100, 4, 1, 2)  # one slab pair: never steady; 2 slabs < the 3 stages of the wave-specialised ring
    M, N, K = C.ONE_SLAB
    assert K // 64 == 1 and M % 256 and N % 8 == 4
    # the ping-pong kernel needs K % 128 == 0: configurations 9 and 10 run the small-tile kernel at K = 64
    for cfg in (9, 10):
        for a, o in C.PAIRS_ALL:
            p = _plan(hip, cfg, C.plan_args(C.Case(a, o, cfg, C.ONE_SLAB, "chip", "linear")), "chip")
            assert p["status"] == 0 and p["kernel"] == 0, (cfg, a, o, p)
    assert {c.cfg for c, _ in plans if c.shape == C.ONE_SLAB} == {7, 6}
    # the column-group tile order on the 256-column kernels and on the wave-specialised one, both with a ragged last group
    g256 = {(p["kernel"], p["rows"]) for c, p in plans if p["ngrp"] > 0 and p["cols"] == 256}
    assert g256 == {(C.SQ, 256), (C.PP, 256), (C.PP, 192)}
    gws = [(c, p) for c, p in plans if p["ngrp"] > 0 and p["kernel"] == C.WS]
    assert {c.operand for c, _ in gws} == {"bf16", "f16", "f16s"}
    for c, p in plans:
        if p["ngrp"] > 0:
            assert p["ntn"] == 17 and p["ntn"] % p["ngrp"] == 1 and p["ntm"] == 2, (c, p)
            assert p["ngrp"] == (8 if p["cols"] == 256 else 9216 // c.shape[2]), (c, p)  # gemm_plan.h: 8, and G = 12 * 768 / K
    assert {(c.sched, c.epi) for c, p in plans if p["ngrp"] > 0} == {(k, e) for k in C.SCHEDS for e in ("linear", "residual")}


def test_stream_k_shape_is_the_cheapest_with_a_tail_of_uneven_pieces(hip, plans):
    def live(shape):
        p = _plan(hip, 5, C.plan_args(C.Case("bf16", "f32", 5, shape, "chip", "linear")), "chip")
        pieces = C.sk_pieces(shape)
        return p["status"] == 0 and p["sk"] == 1 and pieces and all(len(q) >= 2 and len(set(q)) > 1 for q in pieces)

    found = min((M * K, M, K) for M in range(C.SK_M_MOD, C.SK_M_MAX + 1, 256) for K in range(64, C.SK_K_MAX + 1, 64) if live((M, C.SK_N, K)))
    assert C.SK_SHAPE == (found[1], C.SK_N, found[2])
    M, N, K = C.SK_SHAPE
    assert M % 256 == 45 and N % 128 == 8 and N % 8 == 0
    assert C.sk_pieces(C.SK_SHAPE) == [[2, 3]] * 5  # five XCDs with one tail tile in two pieces of 2 and 3 slabs, three XCDs without
    for c, p in plans:
        if c.shape == C.SK_SHAPE:
            assert p["kernel"] == C.WS and p["sk"] == 1 and p["grid"] == 256 and _tiles(p) == 261, (c, p)
    # the same launches without the tail (configuration 7), which the GPU test compares with
    p7 = _plan(hip, 7, C.plan_args(C.Case("bf16", "f32", 7, C.SK_SHAPE, "chip", "linear")), "chip")
    assert p7["kernel"] == C.WS and p7["sk"] == 0 and p7["grid"] == 256


def test_yardstick_of_the_f16_split_launches_is_the_small_tile_kernel(hip, plans):
    for c, _ in plans:
        if c.operand == "f16s":
            y = C.yardstick(c)
            p = _plan(hip, y.cfg, C.plan_args(y), y.sched)
            assert p["status"] == 0 and p["kernel"] == 0 and p["mode"] == C.MODE["f32"] and p["om"] == 0, (y, p)


def test_splitk_pp_cases():
    assert C.SPLITK_SHAPES == ((300, 264, 256, 2), (600, 520, 1024, 4)) and C.SPLITK_WALKED == C.SPLITK_SHAPES[1]
    for M, N, K, S in C.SPLITK_SHAPES:
        assert K % (128 * S) == 0 and N % 8 == 0 and M % 256 and N % 256 == 8
    M, N, K, S = C.SPLITK_SHAPES[0]
    assert K // S // 128 == 1  # one slab pair per K range
    assert C.splitk_units(C.SPLITK_WALKED) == 36 and C.splitk_grid(C.SPLITK_WALKED, "stream") == 8 and C.splitk_grid(C.SPLITK_WALKED, "chip") == 40
    assert C.splitk_units(C.SPLITK_SHAPES[0]) == 8
    for M, N, K, S in C.SPLITK_REFUSED:
        assert K % (128 * S) != 0 or N % 8 != 0
    assert sum(1 for M, N, K, S in C.SPLITK_REFUSED if K % (128 * S)) == 2 and sum(1 for M, N, K, S in C.SPLITK_REFUSED if N % 8) == 1
