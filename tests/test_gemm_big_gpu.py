"""The big-tile GEMMs - gemm_ws_kernel (256x128, wave-specialised, optional stream-K tail), gemm_sq_kernel (256x256 lockstep; both
csrc/gemm.hip) and gemm_pp_kernel (256x256 / 192x256 ping-pong and its split-K instantiation, csrc/gemm_pp.hip) - against float64
on a real MI355X: every instantiation of gemm_launch_ws, gemm_launch_sq and madtp_gemm_pp_launch under its forced configuration, with
the vector and the scalar epilogue, on the whole chip and on a stream that owns one CU per XCD.  There the grid is 8 workgroups and
each walks 2 to 5 tiles of a 1100-row problem: the hand-over of the LDS ring from tile to tile, the half-tiles that run ahead during
an epilogue and the phantom loads past the last tile are live.  The launches are the table of tests/gemm_big_cases.py
(tests/test_gemm_big_cpu.py checks on the planner what the table reaches: the shortest K loops, the column-group tile order, ragged
last tiles, a stream-K tail of two uneven pieces).  References are float64 products on the CPU of the operands as the kernel sees
them (rounded to their format), for f16-split operands of the ORIGINAL f32 operands; outputs are compared with them on the device.
Outputs that are views lie in sentinel buffers with 64 rows below row M, A's NaN tail lies below its row M: a ragged last row tile
that stored or loaded past M would show.

Bounds, none of them measured on these kernels; they are the ones tests/test_gemm_small_gpu.py derives.
mag = |A| |W|^T + |bias| + |residual| in float64 (out_scale, a power of two, scales the first two terms exactly):
  no activation, f32 output, bf16 / f16 operands: |out - ref| <= (K + 8) 2^-24 mag elementwise - an f32 dot product of K terms in any
      order (the products of 2-byte operands are exact in f32) plus the few roundings of the epilogue;
  stream-K launches: (K + 16) 2^-24 mag - at most SK_MAX_PARTS = 8 partial sums are added in f32 on top;
  2-byte outputs: that plus one rounding of the result, 2^-8 |ref| (bf16) or 2^-10 |ref| + 2^-24 (f16);
  f16-split operands: max err / mag < max(3 e32, 3e-7), e32 the same figure of the f32-operand launch of the small-tile kernel at the
      same shape, schedule and epilogue (no big tile takes f32 operands; the yardstick of test_gemm_f16x3_pingpong) - that launch
      runs the same epilogue code, so it has to meet the first bound itself before it counts; split output 1e-6 max(mag, 1) after
      joining the planes;
  activations (their f32 forms against float64 erf / exp): f32 output 2e-5 max(1, max|ref|), bf16 1e-2 and f16 1.5e-3 of that
      scale, f16-split operands 1e-6 max(mag, 1);
  stream-K against the same launch without the tail (configuration 7): 2e-5 max(1, max|core|), as test_gemm_stream_k_tail has it;
      for a bf16 output plus the two results' own roundings, which may fall to different sides: 2^-8 |ref| each, 2^-7 |ref|;
  split-K partials: each slab against the float64 product over its own K range, max err / mag < max(3 e32, 3e-7) with e32 from
      hip.gemm_splitk on f32 operands at the same shape and schedule (the criterion of test_splitk_partials).

Bit relations that hold (asserted):
  repeated launches give identical bits (3 repeats per linear case on the stream, 10 of the ping-pong kernels where every workgroup
      walks tiles; the stream-K tail too: its pieces are summed in piece order);
  the stream schedule gives the bits of the whole chip (include/madtp_hip.h: a kernel gives the same bits on any grid);
  A's rows behind row M reach no output, a strided output and the scalar epilogue at a vector shape give the bits of the plain launch;
  configurations 9 and 10 give the bits of configuration 6 on bf16 operands at f32 output (test_gemm_256x256);
  madtp_splitk_sum is the f32 sum of the slabs in slab order.
Printed, not asserted (test_cross_kernel_bits_report), whether configuration 7 and the small tiles give the bits of the 256-column
kernels.  The answer on an MI355X, at both walked shapes on the stream, f32 output, linear epilogue: on bf16 and on f16 operands
yes - configurations 7, 1 and 4 give the bits of configuration 9, not one element differs.  On f16-split operands no: configurations
7, 1 and 4 differ from configuration 9 in 38 to 49 % of the elements (by low-order bits: each of them meets the f16-split bound
above, and test_gemm_f16x3_pingpong holds the two within 3e-7 of mag).  The wave-specialised and small-tile kernels keep the P0
fragments of a k-slab in registers and add its three products in two staged steps, the ping-pong kernel streams them as three slabs;
include/madtp_hip.h therefore promises equal bits across kernel choices for plain 2-byte operands only."""
import pytest
import torch

from tests import gemm_big_cases as C
from tests import gemm_parity as P
from tests.gemm_parity import CONTAINER, SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


@pytest.fixture(scope="module")
def stream(hip):
    """the one stream of this module that carries scheduling attributes: one CU per XCD"""
    s = torch.cuda.Stream()
    hip.stream_set_sched(s, *C.STREAM_SCHED)
    yield s
    hip.stream_set_sched(s, 32, 0.0, -2)  # (torch hands its pooled streams out again: leave it as a whole-chip stream)


@pytest.fixture(scope="module")
def problems(hip):
    """operands and float64 products per (operand format, shape), built once (tests/gemm_parity.py)"""
    return P.problem_cache(hip)


def _dbits(t):
    """the bits of a result, kept on the device (a copy where `t` is a view)"""
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _launch(hip, problems, stream, case):
    """the launch of one table row -> (output view on the device, the whole buffer it lies in)"""
    M, N, K = case.shape
    e, args, p = C.epi(case), C.plan_args(case), problems(case.operand, case.shape)
    a = p.a_as(e["a"])
    cols = (2 if case.output == "f16s" else 1) * N
    if e["out"] == "strided":
        whole = torch.full((M + C.PAD_ROWS, cols + e["pad_cols"]), SENTINEL, device="cuda", dtype=CONTAINER[case.output])
        out = whole[:M, C.COL0:C.COL0 + cols]
    else:
        whole = out = torch.empty((M, cols), device="cuda", dtype=CONTAINER[case.output])
    assert (a.stride(0), p.w.stride(0), out.stride(0)) == (args["lda"], args["ldw"], args["ldc"])  # as tests/test_gemm_big_cpu.py plans it
    assert p.res_d.stride(0) == args["ldr"] or not e["residual"]
    act = {None: hip.ACT_NONE, "gelu": hip.ACT_GELU, "relu": hip.ACT_RELU, "quick_gelu": hip.ACT_QUICK_GELU}[e["act"]]
    with P.lp(hip, case.operand), hip.gemm_config(case.cfg), P.on(stream if case.sched == "stream" else None):
        hip.gemm(a, p.w, p.bias_d if e["bias"] else None, p.res_d if e["residual"] else None, out_dtype=CONTAINER[case.output], act=act,
                 n=N, out=out, out_scale=e["out_scale"])
    return out, whole


_REF = {}  # (operand, shape, bias, act, out_scale, residual) -> (ref, mag): float64, made on the CPU once, kept on the device


def _reference(problems, case):
    e = C.epi(case)
    key = (case.operand, case.shape, e["bias"], e["act"], e["out_scale"], e["residual"])
    if key not in _REF:
        _REF[key] = tuple(t.cuda() for t in P.reference(e, problems(case.operand, case.shape)))
    return _REF[key]


def _err(problems, case, out):
    ref, mag = _reference(problems, case)
    return (P.values(case.output, case.shape[1], out, cpu=False) - ref).abs(), ref, mag


_E32 = {}  # (shape, sched, epilogue) -> max err / mag of the f32-operand launch of the small-tile kernel: the yardstick of f16-split operands


def _e32(hip, problems, stream, case):
    key = (case.shape, case.sched, case.epi)
    if key not in _E32:
        c32 = C.yardstick(case)
        out32 = _launch(hip, problems, stream, c32)[0]
        _check(hip, problems, stream, c32, out32)  # the yardstick shares the epilogue's code: it has to meet its own f32 bound first
        err, _, mag = _err(problems, c32, out32)
        _E32[key] = (err / mag).max().item()
    return _E32[key]


def _check(hip, problems, stream, case, out, tail=False):
    """the bound of the module docstring for this launch (tail: it has a stream-K tail)"""
    M, N, K = case.shape
    e = C.epi(case)
    err, ref, mag = _err(problems, case, out)
    if case.operand == "f16s":
        if case.output == "f32" and e["act"] is None:
            e16, e32 = (err / mag).max().item(), _e32(hip, problems, stream, case)
            print(f"{case}: e16 {e16:.3e} e32 {e32:.3e}")
            assert e16 < max(3.0 * e32, 3e-7), (case, e16, e32)
            return
        bound = 1e-6 * mag.clamp_min(1.0)
    elif e["act"] is None:
        bound = (K + (16 if tail else 8)) * 2.0 ** -24 * mag
        if case.output == "bf16":
            bound = bound + 2.0 ** -8 * ref.abs()
        elif case.output == "f16":
            bound = bound + 2.0 ** -10 * ref.abs() + 2.0 ** -24
    else:
        scale = max(1.0, ref.abs().max().item())
        bound = torch.full_like(ref, {"f32": 2e-5, "bf16": 1e-2, "f16": 1.5e-3}[case.output] * scale)
    ok = err <= bound  # (a NaN fails)
    print(f"{case}: max err / bound {(err / bound).max().item():.3f}")
    assert ok.all(), (case, int((~ok).sum()), (err / bound)[~ok].max().item(), err[~ok].max().item())


def _check_view(case, out, whole, plain):
    """a strided output: the bits of the plain launch, and not a bit outside the view - the rows below M included"""
    assert torch.equal(_dbits(out), plain), case
    want = torch.full_like(whole, SENTINEL)
    want[:out.shape[0], C.COL0:C.COL0 + out.shape[1]] = out
    assert torch.equal(_dbits(whole), _dbits(want)), case


@pytest.mark.parametrize("cfg,pair", C.IDS, ids=[f"cfg{cfg}-{a}-{o}" for cfg, (a, o) in C.IDS])
def test_parity(hip, problems, stream, cfg, pair):
    operand, output = pair
    hip.range_status()
    first = {}  # (shape, sched, epilogue) -> bits of the linear launches and of the residual ones at the shape with column groups
    for case in C.id_cases(operand, output, cfg):
        out, whole = _launch(hip, problems, stream, case)
        _check(hip, problems, stream, case, out)
        if case.epi == "linear" or case.shape not in C.WALKED:
            first[(case.shape, case.sched, case.epi)] = _dbits(out)
            continue
        plain = first[(case.shape, "stream", "linear")]
        if case.epi == "nan_tail":  # the rows behind A's M rows reach no output
            assert torch.equal(_dbits(out), plain), case
        if case.epi in ("strided", "ldc_odd"):
            _check_view(case, out, whole, plain)
    for (shape, sched, epi), got in first.items():
        if sched != "stream":
            continue
        # results do not depend on stream attributes (include/madtp_hip.h), nor on the run: a race in the ring would show
        assert torch.equal(got, first[(shape, "chip", epi)]), (pair, cfg, shape, epi)
        again = C.Case(operand, output, cfg, shape, "stream", epi)
        # where every workgroup of the ping-pong kernel walks tiles with two slab pairs each, the run-ahead DMA stream crosses a tile
        # boundary under the fragment reads of the tile before: ten repeats
        for _ in range(10 if (cfg in (9, 10) and shape == C.SHAPES[0] and epi == "linear") else 3):
            assert torch.equal(_dbits(_launch(hip, problems, stream, again)[0]), got), (pair, cfg, shape, epi)
    if output in ("f16", "f16s"):
        assert hip.range_status() == 0  # O(1) operands: nothing left the f16 range


def test_pingpong_equals_lockstep_bit_for_bit(hip, problems, stream):
    """same k order per accumulator in the ping-pong kernel, on both tile heights, as in the lockstep kernel (test_gemm_256x256)"""
    for shape in C.WALKED + (C.GROUPED_256,):
        for sched in C.SCHEDS:
            for epi in ("linear", "residual"):
                got = {cfg: _dbits(_launch(hip, problems, stream, C.Case("bf16", "f32", cfg, shape, sched, epi))[0]) for cfg in (6, 9, 10)}
                for cfg in (9, 10):
                    assert torch.equal(got[cfg], got[6]), (shape, sched, epi, cfg, int((got[cfg] != got[6]).sum()))


def test_cross_kernel_bits_report(hip, problems, stream):
    """prints (pytest -s) whether the wave-specialised kernel and the small tiles give the bits of the 256-column ping-pong kernel;
    asserts only that each is within the parity bound (test_parity has the big tiles; here the small-tile launches)"""
    for operand in ("bf16", "f16", "f16s"):
        for shape in C.WALKED:
            got = {cfg: _launch(hip, problems, stream, C.Case(operand, "f32", cfg, shape, "stream", "linear"))[0] for cfg in (9, 7, 1, 4)}
            for cfg in (1, 4):
                _check(hip, problems, stream, C.Case(operand, "f32", cfg, shape, "stream", "linear"), got[cfg])
            for cfg in (7, 1, 4):
                differ = int((_dbits(got[cfg]) != _dbits(got[9])).sum())
                print(f"cross-kernel bits: {operand} {shape} configuration {cfg} vs 9: {differ} of {got[9].numel()} elements differ")


# ---- the stream-K tail of the wave-specialised kernel ---------------------------------------------------------------------------
_SK_PLAIN = {}  # output -> bits of the linear stream-K launch


@pytest.mark.parametrize("epi", list(C.EPILOGUES))
@pytest.mark.parametrize("output", [o for _, o in C.PAIRS_BF16])
def test_stream_k_tail(hip, problems, stream, output, epi):
    """configuration 5 where the plan has a tail (one tail tile on five XCDs, cut into pieces of 2 and 3 slabs): the parity bound with
    the partial sums' roundings, bit-equal to a second launch (the tickets reset themselves, the pieces are summed in piece order),
    and within test_gemm_stream_k_tail's distance of the same launch without the tail"""
    case = C.Case("bf16", output, 5, C.SK_SHAPE, "chip", epi)
    assert case in C.sk_cases(output)
    out, whole = _launch(hip, problems, stream, case)
    _check(hip, problems, stream, case, out, tail=True)
    got = _dbits(out)
    assert torch.equal(_dbits(_launch(hip, problems, stream, case)[0]), got), case
    plain, _ = _launch(hip, problems, stream, case._replace(cfg=7))
    _, ref, _ = _err(problems, case, out)
    n = case.shape[1]
    dist = (P.values(output, n, out, cpu=False) - P.values(output, n, plain, cpu=False)).abs()
    bound = 2e-5 * max(1.0, problems("bf16", C.SK_SHAPE).core.abs().max().item()) + (2.0 ** -7 * ref.abs() if output == "bf16" else 0.0)
    assert (dist <= bound).all(), (case, dist.max().item())
    if epi in ("nan_tail", "strided", "ldc_odd"):
        if output not in _SK_PLAIN:
            _SK_PLAIN[output] = _dbits(_launch(hip, problems, stream, case._replace(epi="linear"))[0])
        if epi == "nan_tail":
            assert torch.equal(got, _SK_PLAIN[output]), case
        else:
            _check_view(case, out, whole, _SK_PLAIN[output])


# ---- split-K partials of the ping-pong kernel -----------------------------------------------------------------------------------
def _splitk_pp(hip, problems, stream, shape, sched):
    """madtp_gemm_splitk_pp as backward.wgrad calls it -> (status, [S + 1, M, N] on the device: the S partial slabs and a sentinel slab
    behind them that the launch must leave alone)"""
    M, N, K, S = shape
    p = problems("f16s", (M, N, K))
    buf = torch.full((S + 1, M, N), SENTINEL, device="cuda", dtype=torch.float32)
    assert (p.a.stride(0), p.w.stride(0)) == (2 * K, 2 * K) and p.w.shape[0] % 128 == 0
    with P.on(stream if sched == "stream" else None):
        rc = hip.load().madtp_gemm_splitk_pp(p.a.data_ptr(), p.w.data_ptr(), buf.data_ptr(), M, N, K, 2 * K, 2 * K, S, p.w_scale,
                                             torch.cuda.current_stream().cuda_stream)
    return rc, buf


def _splitk_small(hip, problems, stream, shape, sched):
    """hip.gemm_splitk on f32 operands (the small-tile kernel): the yardstick -> [S, M, N], raw accumulators of logical weights"""
    M, N, K, S = shape
    p = problems("f32", (M, N, K))
    with P.on(stream if sched == "stream" else None):
        return hip.gemm_splitk(p.a, p.w, S, N)


def _splitk_errors(shape, p, part):
    """max over the slabs and elements of err / mag, each slab against the float64 product over its K range"""
    M, N, K, S = shape
    worst = 0.0
    for s in range(S):
        ks = slice(s * K // S, (s + 1) * K // S)
        ref, mag = p.ar[:, ks] @ p.wr[:, ks].t(), p.ar[:, ks].abs() @ p.wr[:, ks].abs().t()
        worst = max(worst, ((part[s].double().cpu() - ref).abs() / mag).max().item())
    return worst


@pytest.mark.parametrize("shape", C.SPLITK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_splitk_pp_partials(hip, problems, stream, shape):
    M, N, K, S = shape
    p = problems("f16s", (M, N, K))
    parts = {}
    for sched in C.SCHEDS:
        rc, buf = _splitk_pp(hip, problems, stream, shape, sched)
        assert rc == 0, (shape, sched, rc)
        parts[sched] = buf
        assert torch.equal(_dbits(buf[S]), _dbits(torch.full_like(buf[S], SENTINEL))), (shape, sched)
        # (the accumulator scale of the weight went into the launch: the slabs are the logical products)
        e16 = _splitk_errors(shape, p, buf)
        e32 = _splitk_errors(shape, problems("f32", (M, N, K)), _splitk_small(hip, problems, stream, shape, sched))
        print(f"split-K {shape} {sched}: e16 {e16:.3e} e32 {e32:.3e}")
        assert e32 <= (K // S + 8) * 2.0 ** -24, (shape, sched, e32)  # the yardstick meets its own bound (test_splitk_partials)
        assert e16 < max(3.0 * e32, 3e-7), (shape, sched, e16, e32)
        # madtp_splitk_sum: the slabs added in slab order in f32
        total = torch.full((M, N), SENTINEL, device="cuda", dtype=torch.float32)
        with P.on(stream if sched == "stream" else None):
            assert hip.load().madtp_splitk_sum(buf.data_ptr(), S, M * N, total.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        want = buf[0].clone()
        for s in range(1, S):
            want = want + buf[s]
        assert torch.equal(_dbits(total), _dbits(want)), (shape, sched)
    assert torch.equal(_dbits(parts["stream"]), _dbits(parts["chip"])), shape


def test_splitk_pp_refuses_bad_shapes(hip, problems, stream):
    """K % (128 S) != 0 and N % 8 != 0: MADTP_E_SHAPE, and nothing is launched"""
    from madtp_amd import abi
    for shape in C.SPLITK_REFUSED:
        rc, buf = _splitk_pp(hip, problems, stream, shape, "chip")
        assert rc == abi.DEFINES["MADTP_E_SHAPE"], (shape, rc)
        torch.cuda.synchronize()
        assert torch.equal(_dbits(buf), _dbits(torch.full_like(buf, SENTINEL))), shape
