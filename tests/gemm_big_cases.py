"""The launches of tests/test_gemm_big_gpu.py, listed once: the three big-tile GEMM kernels - gemm_ws_kernel (256x128,
wave-specialised, csrc/gemm.hip), gemm_sq_kernel (256x256 lockstep, csrc/gemm.hip) and gemm_pp_kernel (256x256 / 192x256 ping-pong,
csrc/gemm_pp.hip) - under their forced configurations, with their operand -> output pairs, shapes, epilogues and the two schedules,
plus the stream-K launches and the split-K partial launches of the ping-pong kernel.  The GPU test runs them;
tests/test_gemm_big_cpu.py plans every one of them with hip.gemm_plan() and checks what the table as a whole reaches.  Nothing here
needs a GPU."""
import collections

from madtp_amd import hip
from tests.gemm_small_cases import (ACTS, COL0, DT, ESZ, MODE, NAN_ROWS, OM, PAD_COLS, PAD_ROWS, SCHEDS, STREAM_SCHED,  # noqa: F401
                                    EPILOGUES as SMALL_EPILOGUES, plan)

# hip.gemm_config(): 7 wave-specialised, 5 the same with the stream-K tail, 6 lockstep, 9 / 10 ping-pong on 256 / 192 rows
CONFIGS = (7, 5, 6, 9, 10)
WS, SQ, PP = 1, 2, 3  # GemmPlan::kernel
KERNEL = {7: WS, 5: WS, 6: SQ, 9: PP, 10: PP}
TILE = {7: (256, 128), 5: (256, 128), 6: (256, 256), 9: (256, 256), 10: (192, 256)}  # rows, columns

# operand format -> output format, as gemm_launch_ws / gemm_launch_sq / madtp_gemm_pp_launch instantiate them
PAIRS_ALL = (("bf16", "f32"), ("bf16", "bf16"), ("f16", "f32"), ("f16", "f16"), ("f16s", "f32"), ("f16s", "f16s"))
PAIRS_BF16 = PAIRS_ALL[:2]  # the lockstep kernel has bf16 operands only, and the stream-K tail runs on them only
PAIRS = {7: PAIRS_ALL, 9: PAIRS_ALL, 10: PAIRS_ALL, 6: PAIRS_BF16, 5: PAIRS_BF16}
IDS = tuple((cfg, pair) for cfg in CONFIGS for pair in PAIRS[cfg])  # one test id each

# (M, N, K), the smallest at which each mechanism is live (tests/test_gemm_big_cpu.py confirms every claim on the planner):
#   (1100, 776, 256):  ragged last row tile at 256 rows (76 left) and at 192 rows (140 left), last column tile with 8 valid columns at
#                      both tile widths, N % 8 == 0: the vector epilogue; two slab pairs of the ping-pong kernel; on the stream 35
#                      (256x128), 20 (256x256) and 24 (192x256) tiles on 8 workgroups
#   (1100, 780, 128):  N % 8 == 4: the scalar epilogue; one slab pair - the ping-pong loop never becomes steady; two slabs against
#                      the three-stage ring of the wave-specialised kernel
#   (300, 100, 64):    one slab (a ring longer than the loop); 2 tiles: XCDs without a tile.  Configurations 7 and 6 only: the ping-pong
#                      kernel needs K % 128 == 0, and 9 / 10 plan the small-tile kernel here
#   (300, 4104, 128):  6, 9, 10: 17 column tiles of 256, so column groups of 8 with a ragged last group of 1 (tile_mn, ngrp = 8)
#   (300, 2056, 2304): 7: 17 column tiles of 128 against G = 9216 / K = 4, so column groups of 4 (ngrp = 4), ragged last group of 1
SHAPES = ((1100, 776, 256), (1100, 780, 128), (300, 100, 64))
WALKED = SHAPES[:2]  # on the stream schedule (a grid of 8) every workgroup walks 2 to 5 tiles of these
ONE_SLAB = SHAPES[2]
GROUPED_256 = (300, 4104, 128)
GROUPED_WS = (300, 2056, 2304)
GROUPED = {7: GROUPED_WS, 6: GROUPED_256, 9: GROUPED_256, 10: GROUPED_256}
GROUPED_EPILOGUES = ("linear", "residual")

# The stream-K tail (configuration 5, bf16 operands, the whole chip): GemmPlan::sk is 1 only on a grid of 256, and a tail exists only
# when some XCD has more tiles than its 32 workgroups: 257 tiles of 256x128 or more.  K is kept small instead of M.  Found by
# tests/test_gemm_big_cpu.py as the cheapest (least M K) of: N = 1032 (a last column tile of 8), M = 45 mod 256 up to 8237 (a ragged
# last row tile), K a multiple of 64 up to 512, sk == 1, at least 2 pieces on every XCD with a tail, and pieces of uneven length.
# 29 x 9 = 261 tiles: five XCDs have 33 (one tail tile, cut into 2 pieces of 2 and 3 slabs), three have 32 (no tail).
SK_SHAPE = (7213, 1032, 320)
SK_N, SK_M_MOD, SK_M_MAX, SK_K_MAX = 1032, 45, 8237, 512
SK_MAX_PARTS = 8  # csrc/gemm_plan.h


def sk_pieces(shape):
    """per XCD with a stream-K tail on the whole chip: the slab counts of the pieces of one tail tile (csrc/gemm_plan.h sk_parts and
    csrc/gemm.hip gemm_ws_kernel: piece j of p covers slabs [j nk / p, (j + 1) nk / p))"""
    M, N, K = shape
    tiles, nk, gl, out = -(-M // 256) * -(-N // 128), K // 64, 32, []
    for x in range(8):
        nslots = (x + 1) * tiles // 8 - x * tiles // 8  # xcd_tiles (csrc/gemm_device.h)
        rem = nslots - nslots // gl * gl
        p = min(gl // rem, SK_MAX_PARTS, nk // 2) if rem else 0
        if p >= 2:
            out.append([(j + 1) * nk // p - j * nk // p for j in range(p)])
    return out


# epilogues and layouts: those of the small-tile table unchanged, and out_scale together with a residual - the residual is not scaled:
# act(a w^T + bias) * out_scale + residual (hip.gemm).  A residual with a row stride of its own (ldr > N) is NOT in the table:
# hip.gemm takes a contiguous residual only (_req), so such a launch needs a change to the library.
EPILOGUES = collections.OrderedDict(SMALL_EPILOGUES)
EPILOGUES["scale_residual"] = dict(bias=True, out_scale=0.5, residual=True)

Case = collections.namedtuple("Case", "operand output cfg shape sched epi")


def epi(case):
    e = dict(bias=True, act=None, out_scale=1.0, residual=False, a=None, out=None, pad_cols=PAD_COLS)
    e.update(EPILOGUES[case.epi])
    return e


def id_shapes(cfg):
    """the shapes whose linear epilogue runs on both schedules"""
    return WALKED + ((ONE_SLAB,) if cfg in (7, 6) else ()) + ((GROUPED[cfg],) if cfg in GROUPED else ())


def id_cases(operand, output, cfg):
    """every launch of one test id: the linear epilogue on every shape and both schedules, every other epilogue on the stream at the
    two shapes whose tiles the workgroups walk, the residual on both schedules at the shape with column groups"""
    out = [Case(operand, output, cfg, s, sched, "linear") for s in id_shapes(cfg) for sched in SCHEDS]
    out += [Case(operand, output, cfg, s, "stream", e) for s in WALKED for e in EPILOGUES if e != "linear"]
    if cfg in GROUPED:
        out += [Case(operand, output, cfg, GROUPED[cfg], sched, e) for sched in SCHEDS for e in GROUPED_EPILOGUES if e != "linear"]
    return out


def sk_cases(output):
    """the stream-K launches: every epilogue on the whole chip"""
    return [Case("bf16", output, 5, SK_SHAPE, "chip", e) for e in EPILOGUES]


def cases():
    return [c for cfg, (a, o) in IDS for c in id_cases(a, o, cfg)] + [c for _, o in PAIRS_BF16 for c in sk_cases(o)]


def plan_args(case):
    """the arguments of hip.gemm_plan() for this launch, stream left out: leading dimensions in elements as madtp_gemm gets them"""
    M, N, K = case.shape
    e = epi(case)
    ka = (2 if case.operand == "f16s" else 1) * K  # f16-split operands: two planes per row
    cols = (2 if case.output == "f16s" else 1) * N
    return dict(M=M, N=N, K=K, lda=3 * ka if e["a"] == "slice" else ka, ldw=ka, ldc=cols + e["pad_cols"] if e["out"] == "strided" else cols,
                ldr=N if e["residual"] else 0, ab_dtype=DT[case.operand], c_dtype=DT[case.output], splitk=1,
                flags=(hip.PLAN_BIAS if e["bias"] else 0) | (hip.PLAN_RESIDUAL if e["residual"] else 0))


def planned_fast_epi(case):
    """GemmPlan::fast_epi of this launch: the vector epilogue needs N and the leading dimension of C in multiples of 8, and adds a
    residual to f32 outputs only"""
    args, e = plan_args(case), epi(case)
    return int(case.shape[1] % 8 == 0 and args["ldc"] % 8 == 0 and not (e["residual"] and case.output in ("bf16", "f16")))


def scalar_epilogue(case):
    """whether the launch runs the scalar epilogue: where the plan says so, and for a residual next to an f16-split output
    (gemm_launch, csrc/gemm.hip, whatever the plan says)"""
    return not planned_fast_epi(case) or (epi(case)["residual"] and case.output == "f16s")


def yardstick(case):
    """the f32-operand launch of the small-tile kernel (the automatic choice: f32 operands have no big tile) at the shape, schedule and
    epilogue of an f16-split launch: its error is what the f16-split operands are measured against"""
    return case._replace(operand="f32", output="f32", cfg=0)


# ---- split-K partials of the ping-pong kernel (madtp_gemm_splitk_pp): part[s] = A[:, Ks] W[:, Ks]^T, f32, f16-split operands ---------
#   (300, 264, 256, 2):  one slab pair per K range, the shortest loop; 4 tiles x 2 ranges
#   (600, 520, 1024, 4): on the stream 9 tiles x 4 ranges on 8 workgroups
SPLITK_SHAPES = ((300, 264, 256, 2), (600, 520, 1024, 4))  # (M, N, K, splits)
SPLITK_WALKED = SPLITK_SHAPES[1]
SPLITK_REFUSED = ((300, 264, 384, 2), (300, 264, 256, 4), (300, 260, 256, 2))  # K % (128 S) != 0 twice, N % 8 != 0: MADTP_E_SHAPE


def splitk_units(shape):
    """(tile, K range) units of a madtp_gemm_splitk_pp launch"""
    M, N, K, S = shape
    return -(-M // 256) * -(-N // 256) * S


def splitk_grid(shape, sched):
    """its grid (csrc/gemm.hip: gemm_grid over gemm_wg_per_xcd - 32 workgroups per XCD on the chip, 1 on the stream)"""
    return 8 * min(-(-splitk_units(shape) // 8), 32 if sched == "chip" else STREAM_SCHED[0])
