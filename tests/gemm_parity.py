"""What tests/test_gemm_small_gpu.py and tests/test_gemm_big_gpu.py share: the operands of one (format, shape) with what the kernel
sees of them in float64 on the CPU, the float64 reference of an epilogue, and the plumbing of a launch (element format of the
thread, a side stream ordered against the current one, bit views).  Needs a GPU; the tables of launches (tests/gemm_small_cases.py,
tests/gemm_big_cases.py) do not."""
import contextlib

import torch
import torch.nn.functional as F

from tests.gemm_small_cases import NAN_ROWS

SENTINEL = -1234.5
CONTAINER = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.bfloat16, "f16s": torch.float16}  # (hip.py: 2-byte containers)


@contextlib.contextmanager
def lp(hip, operand):
    """the thread's 2-byte element format for these operands"""
    prev = hip.lp_format()
    hip.set_lp_format(hip.F16 if operand == "f16" else hip.BF16)
    try:
        yield
    finally:
        hip.set_lp_format(prev)


@contextlib.contextmanager
def on(s):
    """launch on `s`, ordered after what the current stream has queued and before what it queues next (None: the current stream)"""
    if s is None:
        yield
        return
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        yield
    torch.cuda.current_stream().wait_stream(s)


def rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def pad128(w):
    pad = -w.shape[0] % 128
    return torch.cat([w, torch.zeros(pad, w.shape[1], dtype=w.dtype)], 0).contiguous() if pad else w.contiguous()


def unsplit(p, n):
    """f16 planes [..., 2n] -> P0 + 2^-11 P1, exact in float64"""
    return p[..., :n].double() + p[..., n:].double() / 2048.0


def bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class Problem:
    """operands of one (format, shape) on the device, and what the kernel sees of them in float64 on the CPU; built once, never written"""

    def __init__(self, hip, operand, shape):
        M, N, K = shape
        a, w = rand(M, K, seed=1), rand(N, K, seed=2, scale=0.05)
        self.bias, self.res = rand(N, seed=3), rand(M, N, seed=4)
        self.bias_d, self.res_d = self.bias.cuda(), self.res.cuda()
        ag, wg = a.cuda(), pad128(w).cuda()
        with lp(hip, operand):
            if operand == "f32":
                self.a, self.w, ar, wr = ag, wg, a, w
            elif operand == "f16s":
                self.a, self.w, ar, wr = hip.split_f16(ag), hip.split_f16_weight(wg), a, w  # (the reference: the f32 originals)
            else:
                self.a, self.w = hip.cast_bf16(ag), hip.cast_lp_weight(wg)
                ar, wr = hip.lp_to_f32(self.a).cpu(), hip.lp_to_f32(self.w)[:N].cpu()
        self.w_scale = hip.w_scale_of(self.w)  # 2^-s of the f16 and f16-split weights (|w| < 0.3: s > 0), applied to the accumulator
        assert (self.w_scale < 1.0) == (operand in ("f16", "f16s"))
        self.ar = ar.double()
        self.wr = wr.double() * (1.0 if operand == "f16s" else self.w_scale)  # the logical weight
        self.core = self.ar @ self.wr.t()
        self.mag = self.ar.abs() @ self.wr.abs().t()
        self.layouts = {None: self.a}

    def a_as(self, layout):
        if layout not in self.layouts:
            M, ka = self.a.shape
            nan = float("nan")  # (the bf16 NaN pattern is a NaN as f16 bits too)
            if layout == "slice":  # the middle third of the columns of a NaN matrix
                wide = torch.full((M, 3 * ka), nan, device="cuda", dtype=self.a.dtype)
                wide[:, ka:2 * ka] = self.a
                self.layouts[layout] = wide[:, ka:2 * ka]
            else:  # the first M rows of a buffer whose later rows are NaN
                buf = torch.full((M + NAN_ROWS, ka), nan, device="cuda", dtype=self.a.dtype)
                buf[:M] = self.a
                self.layouts[layout] = buf[:M]
        return self.layouts[layout]


def problem_cache(hip):
    cache = {}

    def get(operand, shape):
        if (operand, shape) not in cache:
            cache[(operand, shape)] = Problem(hip, operand, shape)
        return cache[(operand, shape)]
    return get


def values(output, n, out, cpu=True):
    """an output of format `output` with n logical columns as float64 [M, n], on the CPU or where it lies (every step is exact)"""
    if cpu:
        out = out.cpu()
    if output == "f16s":
        return unsplit(out, n)
    if output == "f16":
        return out.view(torch.float16).double()
    return out.double()


def reference(e, p):
    """-> (ref, mag) of the epilogue `e` (the dict of a table's epi()) on problem p: act(core + bias) * out_scale + residual in float64,
    and the magnitude |A| |W|^T + |bias| + |residual| its rounding errors are measured against"""
    lin = p.core + p.bias.double() if e["bias"] else p.core
    mag = (p.mag + p.bias.double().abs() if e["bias"] else p.mag) * e["out_scale"]
    fn = {None: lambda t: t, "gelu": F.gelu, "relu": F.relu, "quick_gelu": lambda t: t * torch.sigmoid(1.702 * t)}[e["act"]]
    ref = fn(lin) * e["out_scale"]
    if e["residual"]:
        ref, mag = ref + p.res.double(), mag + p.res.double().abs()
    return ref, mag
