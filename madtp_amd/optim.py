"""AdamW on the HIP path: optimizer.step() of the training drivers (utils.py create_optimizer -> torch.optim.AdamW) as ONE launch
over every parameter of a step (madtp_adamw_step, csrc/optim.hip) instead of torch's dozen multi-tensor passes.

    from madtp_amd import optim
    optimizer = optim.AdamW(params=model.parameters(), lr=..., weight_decay=...)      # the drivers' one changed line

or, to run a driver unchanged, `optim.install()`: torch.optim.AdamW(...) then builds this class wherever it applies.

The arithmetic is torch's single-tensor AdamW (torch/optim/adam.py _single_tensor_adam, decoupled weight decay) element by element
in f32; state (`exp_avg`, `exp_avg_sq`, `step`) has torch's keys, dtypes and placement, so state_dict() / load_state_dict()
interchange with torch.optim.AdamW in both directions.  There is no eager fallback: what the kernel does not cover raises."""
import math
import struct

import torch
from torch.optim.optimizer import Optimizer

from . import hip
from . import runtime as _runtime  # noqa: F401  (registers the optimizer-step post-hook the prepared-weight caches follow)


def _f32(x):
    """a Python double rounded once to f32 (what the kernel receives)"""
    return struct.unpack("f", struct.pack("f", x))[0]


def adamw_scalars(lr, beta1, beta2, eps, weight_decay, step):
    """The kernel's scalars of step number `step` (1, 2, ...), each formed in Python double as torch's single-tensor AdamW forms
    it and rounded once to f32 -> (decay, w1, beta2, w2, step_size, bc2_sqrt, eps).  decay is exactly 1 when weight_decay == 0
    (torch skips the multiplication; p * 1 is exact)."""
    return (_f32(1.0 - lr * weight_decay) if weight_decay != 0 else 1.0, _f32(1.0 - beta1), _f32(beta2), _f32(1.0 - beta2),
            _f32(lr / (1.0 - beta1 ** step)), _f32(math.sqrt(1.0 - beta2 ** step)), _f32(eps))


def plan(numels, steps):
    """Pure planning of one (param group, device): element counts and `step` values (before this step) of the parameters that have
    a gradient -> the launches, one per distinct step value in order of first appearance:
    [{"step": value, "index": positions in the input, "first": first workgroup of each of them, "blocks": total}].
    A zero-element tensor stays in its bucket (its step advances) and owns no workgroup."""
    buckets = {}
    for i, s in enumerate(steps):
        buckets.setdefault(s, []).append(i)
    out = []
    for s, index in buckets.items():
        first, nb = hip.adamw_first_blocks([numels[i] for i in index])
        out.append({"step": s, "index": index, "first": first, "blocks": nb})
    return out


def _refuse(name, value):
    if value:
        raise ValueError(f"madtp_amd.optim.AdamW does not support {name}=True (there is no eager fallback; use torch.optim.AdamW)")


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"madtp_amd.optim.AdamW: parameters must be tensors, got {type(p).__name__}")
    if p.is_complex() or p.is_sparse or p.layout != torch.strided or p.dtype != torch.float32 or not p.is_cuda:
        raise ValueError(f"madtp_amd.optim.AdamW: every parameter must be a dense GPU f32 tensor, got {p.dtype} on {p.device} "
                         f"({p.layout}); there is no eager fallback")


class AdamW(Optimizer):
    """torch.optim.AdamW's signature and defaults; one madtp_adamw_step launch per (param group, device, `step` value) - the
    drivers' case is one launch.

    Supported: dense f32 parameters on a GPU, float `lr`.  amsgrad / maximize / capturable / differentiable = True, a tensor lr,
    complex, sparse, non-f32 or CPU parameters raise (at construction, add_param_group or the first step); `foreach` and `fused`
    are accepted and ignored.  A parameter whose .grad is None is skipped (no state, its `step` does not advance).  A
    step bumps Parameter._version of what it updated, as torch's in-place ops do (torch's fused=True does not).  A
    NON-CONTIGUOUS .grad is copied into a contiguous tensor for the step (rare; the parameter's .grad itself is left as it is);
    parameters and state must be contiguous.  Every group's lr / betas / eps / weight_decay are read at each step().
    torch.amp.GradScaler works through its generic route (unscale_, then step()); the grad_scale / found_inf arguments of torch's
    fused optimizers are not taken."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("madtp_amd.optim.AdamW: a tensor lr is not supported (the scalars of a step are formed on the host)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # (torch's own group keys, so that a state_dict loads into torch.optim.AdamW and back)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=True)
        self._tables = {}
        super().__init__(params, defaults)

    @staticmethod
    def _check_group(group):
        for name in ("amsgrad", "maximize", "capturable", "differentiable"):
            _refuse(name, group.get(name, False))
        if isinstance(group["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
            raise ValueError("madtp_amd.optim.AdamW: tensor lr / betas are not supported")
        if not group.get("decoupled_weight_decay", True):
            raise ValueError("madtp_amd.optim.AdamW: decoupled_weight_decay=False is Adam, not AdamW")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        self._check_group(group)
        for p in group["params"]:
            _check_param(p)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}
        self._normalise_steps()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = {}
        self._normalise_steps()

    def _normalise_steps(self):
        """`step` as torch's default implementations keep it: an f32 scalar tensor on the CPU (a state saved by fused=True holds it
        on the device, an old one as a float)"""
        for group in self.param_groups:
            group.setdefault("decoupled_weight_decay", True)
        for st in self.state.values():
            if "step" in st:
                s = st["step"]
                if not torch.is_tensor(s):
                    st["step"] = torch.tensor(float(s), dtype=torch.float32)
                elif s.is_cuda or s.dtype != torch.float32:
                    st["step"] = s.detach().to("cpu", torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            beta1, beta2 = group["betas"]
            per_device = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise RuntimeError("madtp_amd.optim.AdamW does not support sparse gradients")
                st = self.state[p]
                if len(st) == 0:
                    _check_param(p)
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if not g.is_contiguous():
                    g = g.contiguous()
                per_device.setdefault(p.device, []).append((p, g, st))
            for dev, items in per_device.items():
                steps = torch.stack([st["step"] for _, _, st in items]).tolist()
                for bi, b in enumerate(plan([p.numel() for p, _, _ in items], steps)):
                    quads = [(items[i][0], items[i][1], items[i][2]["exp_avg"], items[i][2]["exp_avg_sq"]) for i in b["index"]]
                    scalars = adamw_scalars(group["lr"], beta1, beta2, group["eps"], group["weight_decay"], b["step"] + 1)
                    # one table per (group, device, bucket position): the drivers' single bucket keeps its table for good, and
                    # a table whose bucket changed members sees other pointers and rebuilds itself
                    table = self._tables.get((gi, dev, bi))
                    if table is None:
                        table = self._tables[(gi, dev, bi)] = hip.AdamWTable()
                    table.step(quads, scalars)
                    torch._foreach_add_([items[i][2]["step"] for i in b["index"]], 1)
                    # the kernel wrote the parameters behind torch's back: bump their version counters as torch's in-place ops
                    # do, so that autograd's saved-tensor check and every cache keyed on Parameter._version see the update
                    ps = [q[0] for q in quads]
                    torch._C._autograd._unsafe_set_version_counter(ps, [p._version + 1 for p in ps])
        return loss

    def tables(self):
        """the live pointer tables (hip.AdamWTable; `rebuilds` counts their uploads)"""
        return list(self._tables.values())


# ---- opt-in replacement of torch.optim.AdamW, for running the reference's drivers unchanged -------------------------------------
_ORIGINAL = None


def _eligible(param_list, kw):
    if any(kw.get(k) for k in ("amsgrad", "maximize", "capturable", "differentiable")):
        return False
    if isinstance(kw.get("lr"), torch.Tensor) or any(isinstance(b, torch.Tensor) for b in kw.get("betas", ())):
        return False
    tensors = []
    for entry in param_list:
        if isinstance(entry, dict):
            if any(entry.get(k) for k in ("amsgrad", "maximize", "capturable", "differentiable")) or isinstance(entry.get("lr"), torch.Tensor):
                return False
            ps = entry["params"]
            tensors += [ps] if isinstance(ps, torch.Tensor) else list(ps)
        else:
            tensors.append(entry)
    return bool(tensors) and all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 and p.layout == torch.strided
                                 for p in tensors)


def install():
    """After this, torch.optim.AdamW(...) returns madtp_amd.optim.AdamW when every parameter is a dense GPU f32 tensor and no
    unsupported flag is set, and torch's own class otherwise.  uninstall() puts the original object back."""
    global _ORIGINAL
    if _ORIGINAL is not None:
        return
    original = torch.optim.AdamW
    names = ("params", "lr", "betas", "eps", "weight_decay", "amsgrad")

    def adamw(*args, **kwargs):
        kw = dict(zip(names, args))
        if len(args) > len(names) or set(kw) & set(kwargs):
            return original(*args, **kwargs)  # (let torch raise its own TypeError)
        kw.update(kwargs)
        if "params" in kw and not isinstance(kw["params"], torch.Tensor):
            kw["params"] = list(kw["params"])  # (a generator is consumed once)
            if _eligible(kw["params"], kw):
                return AdamW(**kw)
        return original(**kw)

    adamw.__wrapped__ = original
    adamw.__doc__ = original.__doc__
    _ORIGINAL = original
    torch.optim.AdamW = adamw


def uninstall():
    global _ORIGINAL
    if _ORIGINAL is not None:
        torch.optim.AdamW = _ORIGINAL
        _ORIGINAL = None
