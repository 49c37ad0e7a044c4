"""The small-tile GEMM (gemm_kernel, csrc/gemm.hip) against float64 on a real MI355X: every tile variant x operand format x output
mode that the planner can reach, with the vector and the scalar epilogue, on the whole chip and on a stream that owns one CU per
XCD - there the workgroups walk 2 to 4 tiles each with uneven XCD shares, so the LDS ring's hand-over from tile to tile and its
phantom slabs at the tail are live.  The launches are the table of tests/gemm_small_cases.py (tests/test_gemm_small_cpu.py checks on
the planner what the table reaches).  References are float64 products on the CPU of the operands as the kernel sees them (rounded
to their format), for f16-split operands of the ORIGINAL f32 operands.  (The residual next to an f16-split output at N % 8 == 0 is
the launch that used to lose its residual on the vector epilogue: gemm_launch now sends it to the scalar one.)

Bounds, none of them measured on the kernel.  mag = |A| |W|^T + |bias| + |residual| in float64 (out_scale, a power of two, scales
the first two terms exactly):
  no activation, f32 output, f32 / bf16 / f16 operands: |out - ref| <= (K + 8) 2^-24 mag elementwise - an f32 dot product of K
      terms in any order (the products of 2-byte operands are exact in f32) plus the few roundings of the epilogue;
  2-byte outputs: that plus one rounding of the result, 2^-8 |ref| (bf16) or 2^-10 |ref| + 2^-24 (f16);
  f16-split operands: max err / mag < max(3 e32, 3e-7), e32 the same figure of the f32-operand launch of the same variant, shape
      and epilogue (the criterion of test_gemm_f16x3); split output 1e-6 max(mag, 1) after joining the planes;
  activations (their f32 or fast forms against float64 erf / exp), as test_gemm / test_gemm_f16_operands / test_gemm_f16x3 have
      them: f32 output 2e-5 max(1, max|ref|), bf16 1e-2 and f16 1.5e-3 of that scale, f16-split operands 1e-6 max(mag, 1)."""
import pytest
import torch

from tests import gemm_small_cases as C
from tests import gemm_parity as P
from tests.gemm_parity import CONTAINER, SENTINEL, bits as _bits, lp as _lp, on as _on

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
    """the one stream of this module that carries scheduling attributes (64 per process may): one CU per XCD"""
    s = torch.cuda.Stream()
    hip.stream_set_sched(s, *C.STREAM_SCHED)
    yield s
    hip.stream_set_sched(s, 32, 0.0, -2)  # (torch hands its pooled streams out again: leave it as a whole-chip stream)


@pytest.fixture(scope="module")
def problems(hip):
    """operands and float64 products per (operand format, shape), built once (tests/gemm_parity.py)"""
    return P.problem_cache(hip)


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
    assert (a.stride(0), p.w.stride(0), out.stride(0)) == (args["lda"], args["ldw"], args["ldc"])  # as tests/test_gemm_small_cpu.py plans it
    act = {None: hip.ACT_NONE, "gelu": hip.ACT_GELU, "relu": hip.ACT_RELU, "quick_gelu": hip.ACT_QUICK_GELU}[e["act"]]
    with _lp(hip, case.operand), hip.gemm_config(case.cfg), _on(stream if case.sched == "stream" else None):
        hip.gemm(a, p.w, p.bias_d if e["bias"] else None, p.res_d if e["residual"] else None, out_dtype=CONTAINER[case.output], act=act,
                 n=N, out=out, out_scale=e["out_scale"])
    return out, whole


def _values(case, out):
    """the output as float64 [M, N] on the CPU"""
    return P.values(case.output, case.shape[1], out)


def _reference(case, p):
    return P.reference(C.epi(case), p)


_E32 = {}  # (variant, shape, sched, epilogue) -> max err / mag of the f32-operand launch: the yardstick of the f16-split operands


def _e32(hip, problems, stream, case):
    v = C.variant_of(case.operand, case.cfg)
    key = (v, case.shape, case.sched, case.epi)
    if key not in _E32:
        c32 = case._replace(operand="f32", output="f32", cfg=v + 1)
        ref, mag = _reference(c32, problems("f32", case.shape))
        _E32[key] = ((_values(c32, _launch(hip, problems, stream, c32)[0]) - ref).abs() / mag).max().item()
    return _E32[key]


def _check(hip, problems, stream, case, out):
    """the bound of the module docstring for this launch"""
    M, N, K = case.shape
    e, p = C.epi(case), problems(case.operand, case.shape)
    ref, mag = _reference(case, p)
    err = (_values(case, out) - ref).abs()
    if case.operand == "f16s":
        if case.output == "f32" and e["act"] is None:
            e16, e32 = (err / mag).max().item(), _e32(hip, problems, stream, case)
            assert e16 < max(3.0 * e32, 3e-7), (case, e16, e32)
            return
        bound = 1e-6 * mag.clamp_min(1.0)
    elif e["act"] is None:
        bound = (K + 8) * 2.0 ** -24 * mag
        if case.output == "bf16":
            bound = bound + 2.0 ** -8 * ref.abs()
        elif case.output == "f16":
            bound = bound + 2.0 ** -10 * ref.abs() + 2.0 ** -24
    else:
        scale = max(1.0, ref.abs().max().item())
        bound = torch.full_like(ref, {"f32": 2e-5, "bf16": 1e-2, "f16": 1.5e-3}[case.output] * scale)
    ok = err <= bound  # (a NaN fails)
    assert ok.all(), (case, int((~ok).sum()), (err / bound)[~ok].max().item(), err[~ok].max().item())


@pytest.mark.parametrize("cfg", C.CONFIGS)
@pytest.mark.parametrize("pair", C.PAIRS, ids="-".join)
def test_parity(hip, problems, stream, pair, cfg):
    operand, output = pair
    hip.range_status()
    linear = {}
    for case in C.id_cases(operand, output, cfg):
        out, whole = _launch(hip, problems, stream, case)
        _check(hip, problems, stream, case, out)
        if case.epi == "linear":
            linear[(case.shape, case.sched)] = _bits(out)
            continue
        first = linear[(case.shape, "stream")]
        if case.epi == "nan_tail":  # the rows behind A's M rows reach no output
            assert torch.equal(_bits(out), first), case
        if case.epi in ("strided", "ldc_odd"):  # the same values (from the scalar epilogue too), and not a bit outside the view - the rows past M included
            assert torch.equal(_bits(out), first), case
            want = torch.full_like(whole, SENTINEL)
            want[:out.shape[0], C.COL0:C.COL0 + out.shape[1]] = out
            assert torch.equal(_bits(whole), _bits(want)), case
    for shape in C.SHAPES:
        # results do not depend on stream attributes (include/madtp_hip.h), nor on the run: a race in the ring would show
        assert torch.equal(linear[(shape, "stream")], linear[(shape, "chip")]), (pair, cfg, shape)
        again = C.Case(operand, output, cfg, shape, "stream", "linear")
        for _ in range(3):
            assert torch.equal(_bits(_launch(hip, problems, stream, again)[0]), linear[(shape, "stream")]), (pair, cfg, shape)
    if output in ("f16", "f16s"):
        assert hip.range_status() == 0  # O(1) operands: nothing left the f16 range


@pytest.mark.parametrize("operand", ["bf16", "f16", "f16s"])
def test_variants_agree_bit_for_bit(hip, problems, stream, operand):
    """same arithmetic per output element in every kernel choice (include/madtp_hip.h), the tile variant among them: the 2-byte operand
    formats walk K in the same MFMA steps whatever the tile"""
    for shape in C.SHAPES:
        for epi in ("linear", "gelu"):
            for sched in (C.SCHEDS if epi == "linear" else ("stream",)):
                got = [_bits(_launch(hip, problems, stream, C.Case(operand, "f32", cfg, shape, sched, epi))[0]) for cfg in C.CONFIGS]
                for cfg, g in zip(C.CONFIGS[1:], got[1:]):
                    assert torch.equal(g, got[0]), (operand, shape, epi, sched, cfg, int((g != got[0]).sum()))


def test_small_tile_hint_equals_forced_configuration(hip, problems, stream):
    """a stream's small_tile hint v picks the variant that madtp_gemm_set_config(v + 1) forces"""
    for shape in C.WALKED:
        for v in range(4):
            forced = _bits(_launch(hip, problems, stream, C.Case("bf16", "f32", v + 1, shape, "stream", "linear"))[0])
            try:
                hip.stream_set_sched(stream, C.STREAM_SCHED[0], C.STREAM_SCHED[1], v)
                hinted = _launch(hip, problems, stream, C.Case("bf16", "f32", 0, shape, "stream", "linear"))[0]
            finally:
                hip.stream_set_sched(stream, *C.STREAM_SCHED)
            _check(hip, problems, stream, C.Case("bf16", "f32", 0, shape, "stream", "linear"), hinted)
            assert torch.equal(_bits(hinted), forced), (shape, v)


_E32_SPLITK = {}


def _splitk_launch(hip, problems, stream, case):
    """-> part [S + 1, M, N] on the CPU: the S partial slabs, and a sentinel slab behind them that the launch must leave alone"""
    M, N, K, S = case.shape
    p = problems(case.operand, (M, N, K))
    buf = torch.full((S + 1, M, N), SENTINEL, device="cuda", dtype=torch.float32)
    args = C.splitk_plan_args(case)
    assert (p.a.stride(0), p.w.stride(0)) == (args["lda"], args["ldw"])
    with _lp(hip, case.operand), hip.gemm_config(case.cfg), _on(stream if case.sched == "stream" else None):
        part = hip.gemm_splitk(p.a, p.w, S, N, part=buf[:S])
        assert part.data_ptr() == buf.data_ptr()
    return buf.cpu()


def _splitk_errors(case, p, part):
    """max over the slabs and elements of err / mag, each slab against the float64 product over its K range"""
    M, N, K, S = case.shape
    worst = 0.0
    for s in range(S):
        ks = slice(s * K // S, (s + 1) * K // S)
        ref, mag = p.ar[:, ks] @ p.wr[:, ks].t(), p.ar[:, ks].abs() @ p.wr[:, ks].abs().t()
        # the partials are raw accumulators: the logical product over the weight's accumulator scale (a power of two)
        worst = max(worst, ((part[s].double() * p.w_scale - ref).abs() / mag).max().item())
    return worst


@pytest.mark.parametrize("cfg", C.SPLITK_CONFIGS)
@pytest.mark.parametrize("operand", C.OPERANDS)
def test_splitk_partials(hip, problems, stream, operand, cfg):
    for shape in C.SPLITK_SHAPES:
        M, N, K, S = shape
        p = problems(operand, (M, N, K))
        parts = {}
        for sched in C.SCHEDS:
            case = C.SplitKCase(operand, cfg, shape, sched)
            part = parts[sched] = _splitk_launch(hip, problems, stream, case)
            assert torch.equal(_bits(part[S]), _bits(torch.full((M, N), SENTINEL))), case
            e = _splitk_errors(case, p, part)
            if operand == "f16s":
                with hip.gemm_config(cfg):
                    v = C.plan(C.splitk_plan_args(case), stream.cuda_stream if sched == "stream" else None)["variant"]
                key = (v, shape, sched)
                if key not in _E32_SPLITK:
                    c32 = C.SplitKCase("f32", v + 1, shape, sched)
                    _E32_SPLITK[key] = _splitk_errors(c32, problems("f32", (M, N, K)), _splitk_launch(hip, problems, stream, c32))
                assert e < max(3.0 * _E32_SPLITK[key], 3e-7), (case, e, _E32_SPLITK[key])
            else:
                assert e <= (K // S + 8) * 2.0 ** -24, (case, e)
        assert torch.equal(_bits(parts["stream"]), _bits(parts["chip"])), (operand, cfg, shape)
