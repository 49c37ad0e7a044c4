"""The launches of tests/test_gemm_small_gpu.py, listed once: shapes, operand -> output pairs, forced tile configurations, epilogues
and the two schedules of the small-tile GEMM (gemm_kernel, csrc/gemm.hip), plus the split-K partial launches.  The GPU test runs
them; tests/test_gemm_small_cpu.py plans every one of them with hip.gemm_plan() and checks what the table as a whole reaches.
Nothing here needs a GPU."""
import collections

from madtp_amd import hip

# (M, N, K).  328 and 840 are 8 mod 64 and 72 mod 128: a ragged last row tile and column tile at every tile size.
#   (328, 840, 192): N % 8 == 0, the vector epilogue; 3 slabs of 2-byte operands, 6 of f32
#   (328, 844, 64):  N % 8 == 4, the scalar epilogue; 1 slab of 2-byte operands, 2 of f32, 2 f16-split steps
#   (70, 200, 128):  fewer tiles than the minimum grid of 8 workgroups: XCDs without a tile
SHAPES = ((328, 840, 192), (328, 844, 64), (70, 200, 128))
WALKED = SHAPES[:2]  # on the stream schedule the workgroups walk 2 to 4 tiles of these

# operand format -> output format, as gemm_launch_small instantiates them
PAIRS = (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"), ("f16", "f32"), ("f16", "f16"), ("f16s", "f32"), ("f16s", "f16s"))
OPERANDS = ("f32", "bf16", "f16", "f16s")
DT = {"f32": hip.F32, "bf16": hip.BF16, "f16": hip.F16, "f16s": hip.F16S}
MODE = {"bf16": 0, "f16": 1, "f16s": 2, "f32": 3}  # GemmPlan::mode
OM = {"f32": 0, "bf16": 1, "f16s": 2, "f16": 3}    # GemmPlan::om
ESZ = {"f32": 4, "bf16": 2, "f16": 2, "f16s": 2}

CONFIGS = (1, 2, 3, 4)  # hip.gemm_config(): variant 0..3 of kGemmSmallTiles (gemm_plan.h)
TILES = ((128, 128, 2), (64, 128, 2), (64, 128, 3), (64, 64, 3))  # rows, columns, ring stages of the variants


def variant_of(operand, cfg):
    """the variant configuration `cfg` runs: f16-split operands have no 128x128 tile, configuration 1 gives them 64x128 (so the two
    128x128 f16-split instantiations cannot be reached, and the table does not try)"""
    return 1 if (operand == "f16s" and cfg == 1) else cfg - 1


# the two schedules: the whole chip on the current stream, and one stream that owns one CU per XCD (hip.stream_set_sched(s, 1, 0.0, -2))
SCHEDS = ("chip", "stream")
STREAM_SCHED = (1, 0.0, -2)

# epilogues and operand / output layouts.  a: "slice" = a column slice of a three times wider matrix, "nan_tail" = the first M rows of
# a buffer whose later rows are NaN; out: "strided" = the view [:M, 8:8+cols] of an (M + 64) x (cols + pad_cols) sentinel buffer.
# pad_cols 24 keeps the leading dimension a multiple of 8; 20 does not, which sends the vector-epilogue shape to the scalar epilogue
EPILOGUES = collections.OrderedDict((
    ("linear", dict(bias=True)),
    ("nobias", dict(bias=False)),
    ("gelu", dict(bias=True, act="gelu")),
    ("relu", dict(bias=True, act="relu")),
    ("quick_gelu", dict(bias=True, act="quick_gelu")),
    ("out_scale", dict(bias=True, out_scale=0.5)),
    ("residual", dict(bias=True, residual=True)),
    ("lda", dict(bias=True, a="slice")),
    ("nan_tail", dict(bias=True, a="nan_tail")),
    ("strided", dict(bias=True, out="strided")),
    ("ldc_odd", dict(bias=True, out="strided", pad_cols=20)),
))
ACTS = ("gelu", "relu", "quick_gelu")
NAN_ROWS, PAD_ROWS, PAD_COLS, COL0 = 40, 64, 24, 8

Case = collections.namedtuple("Case", "operand output cfg shape sched epi")


def epi(case):
    e = dict(bias=True, act=None, out_scale=1.0, residual=False, a=None, out=None, pad_cols=PAD_COLS)
    e.update(EPILOGUES[case.epi])
    return e


def id_cases(operand, output, cfg):
    """every launch of one test id: the linear epilogue on every shape and both schedules, every other epilogue on the stream at the
    two shapes whose tiles the workgroups walk"""
    out = [Case(operand, output, cfg, s, sched, "linear") for s in SHAPES for sched in SCHEDS]
    out += [Case(operand, output, cfg, s, "stream", e) for s in WALKED for e in EPILOGUES if e != "linear"]
    return out


def cases():
    return [c for (a, o) in PAIRS for cfg in CONFIGS for c in id_cases(a, o, cfg)]


def plan_args(case):
    """the arguments of hip.gemm_plan() for this launch, stream left out: leading dimensions in elements as madtp_gemm gets them"""
    M, N, K = case.shape
    e = epi(case)
    ka = (2 if case.operand == "f16s" else 1) * K  # f16-split operands: two planes per row
    cols = (2 if case.output == "f16s" else 1) * N
    return dict(M=M, N=N, K=K, lda=3 * ka if e["a"] == "slice" else ka, ldw=ka, ldc=cols + e["pad_cols"] if e["out"] == "strided" else cols,
                ldr=N if e["residual"] else 0, ab_dtype=DT[case.operand], c_dtype=DT[case.output], splitk=1,
                flags=(hip.PLAN_BIAS if e["bias"] else 0) | (hip.PLAN_RESIDUAL if e["residual"] else 0))


# ---- split-K partials (madtp_gemm_splitk): part[s] = A[:, Ks] W[:, Ks]^T, f32, no epilogue ---------------------------------------------
SPLITK_SHAPES = ((70, 200, 256, 2), (130, 264, 512, 4))  # (M, N, K, splits)
SPLITK_WALKED = SPLITK_SHAPES[1]  # on the stream: 24 or more slots on 16 to 24 workgroups
SPLITK_CONFIGS = (0, 1, 2, 3, 4)  # 0: the automatic choice

SplitKCase = collections.namedtuple("SplitKCase", "operand cfg shape sched")


def splitk_cases():
    return [SplitKCase(a, cfg, s, sched) for a in OPERANDS for cfg in SPLITK_CONFIGS for s in SPLITK_SHAPES for sched in SCHEDS]


def splitk_plan_args(case):
    M, N, K, S = case.shape
    ka = (2 if case.operand == "f16s" else 1) * K
    return dict(M=M, N=N, K=K, lda=ka, ldw=ka, ldc=N, ldr=0, ab_dtype=DT[case.operand], c_dtype=hip.F32, splitk=S, flags=0)


def plan(args, stream=None):
    """hip.gemm_plan() of plan_args() / splitk_plan_args() as a dict of hip.PLAN_FIELDS"""
    return dict(zip(hip.PLAN_FIELDS, hip.gemm_plan(args["M"], args["N"], args["K"], args["lda"], args["ldw"], args["ldc"], args["ldr"],
                                                   args["ab_dtype"], args["c_dtype"], args["splitk"], args["flags"], stream)))
