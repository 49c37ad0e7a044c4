"""madtp_amd.optim without a GPU: scope guards, the pure table planner, the host scalars, the C entry points' argument checks and
install() / uninstall()."""
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from madtp_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def test_constructor_scope_guards_raise():
    from madtp_amd import optim
    cpu = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="GPU f32"):
        optim.AdamW(cpu)                                                     # a CPU parameter: no eager fallback
    with pytest.raises(ValueError, match="GPU f32"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="GPU f32"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.complex64))])
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=flag):
            optim.AdamW(cpu, **{flag: True})
    with pytest.raises(ValueError, match="tensor lr"):
        optim.AdamW(cpu, lr=torch.tensor(1e-3))
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError, match="Invalid"):
            optim.AdamW(cpu, **bad)
    with pytest.raises(ValueError):
        optim.AdamW([])                                                      # torch's own "empty parameter list"


def test_signature_and_defaults_are_torchs():
    import inspect
    from madtp_amd import optim
    ours, theirs = inspect.signature(optim.AdamW.__init__), inspect.signature(torch.optim.AdamW.__init__)
    assert [(n, p.kind) for n, p in ours.parameters.items()] == [(n, p.kind) for n, p in theirs.parameters.items()]
    assert [p.default for p in ours.parameters.values()] == [p.default for p in theirs.parameters.values()]
    assert issubclass(optim.AdamW, torch.optim.Optimizer)


def test_plan_prefix_sums_and_buckets():
    from madtp_amd import hip, optim
    E = hip.ADAMW_PER_BLOCK
    assert [hip.adamw_blocks(n) for n in (0, 1, E - 1, E, E + 1, 2 * E, 2 * E + 5)] == [0, 1, 1, 1, 2, 2, 3]
    numels = [0, 1, E, 0, E + 1, 2 * E + 5, 0]
    (b,) = optim.plan(numels, [3.0] * len(numels))
    assert b["step"] == 3.0 and b["index"] == list(range(len(numels)))
    assert b["first"] == [0, 0, 1, 2, 2, 4, 7] and b["blocks"] == 7
    # two step values -> two launches, each with its own prefix sum; order of first appearance, input order inside a bucket
    got = optim.plan([5, E + 1, 0, 7, 3 * E], [2.0, 0.0, 2.0, 0.0, 2.0])
    assert got == [{"step": 2.0, "index": [0, 2, 4], "first": [0, 1, 1], "blocks": 4},
                   {"step": 0.0, "index": [1, 3], "first": [0, 2], "blocks": 3}]
    assert optim.plan([], []) == []
    assert optim.plan([0, 0], [1.0, 1.0]) == [{"step": 1.0, "index": [0, 1], "first": [0, 0], "blocks": 0}]


@pytest.mark.parametrize("lr,wd,betas,eps", [(1e-3, 1e-2, (0.9, 0.999), 1e-8), (2e-5, 0.05, (0.9, 0.98), 1e-6), (1e-5, 0.0, (0.9, 0.999), 1e-8)])
def test_host_scalars_are_the_double_formulas_rounded_once(lr, wd, betas, eps):
    from madtp_amd import optim
    b1, b2 = betas
    for t in (1, 2, 3, 10, 1000, 100000):
        want = np.array([1.0 - lr * wd, 1.0 - b1, b2, 1.0 - b2, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), eps], dtype=np.float64)
        got = optim.adamw_scalars(lr, b1, b2, eps, wd, t)
        assert len(got) == 7
        for g, w in zip(got, want):
            assert g == float(np.float32(w))           # one rounding, double -> f32
    assert optim.adamw_scalars(1e-3, 0.9, 0.999, 1e-8, 0.0, 1)[0] == 1.0   # no weight decay: p * 1 is exact


def test_c_entry_points_validate_without_gpu(lib):
    from madtp_amd import hip
    E = hip.ADAMW_PER_BLOCK
    assert [lib.madtp_adamw_blocks(n) for n in (0, 1, E - 1, E, E + 1, 2 * E + 5, 2 ** 33)] == [0, 1, 1, 1, 2, 3, 2 ** 33 // E]
    s = (1.0, 0.1, 0.999, 0.001, 1e-3, 0.03, 1e-8)
    table = (hip.ctypes.c_int64 * 6)()
    ptr = hip.ctypes.addressof(table)
    assert lib.madtp_adamw_step(0, 1, 1, *s, 0) == -1          # table == NULL
    assert lib.madtp_adamw_step(ptr, 0, 1, *s, 0) == -1        # n_tensors < 1
    assert lib.madtp_adamw_step(ptr, 1, -1, *s, 0) == -1       # n_blocks < 0
    assert lib.madtp_adamw_step(ptr, 1, 0, *s, 0) == 0         # nothing to do: no launch, success


def test_install_returns_torchs_class_for_cpu_parameters_and_uninstall_restores():
    from madtp_amd import optim
    original = torch.optim.AdamW
    lin = torch.nn.Linear(3, 2)
    try:
        optim.install()
        assert torch.optim.AdamW is not original
        optim.install()                                         # idempotent
        opt = torch.optim.AdamW(lin.parameters(), lr=1e-2, weight_decay=0.05)
        assert type(opt) is original and opt.param_groups[0]["lr"] == 1e-2
        opt = torch.optim.AdamW(params=(p for p in lin.parameters()), lr=1e-2)   # the drivers' keyword form, a generator
        assert type(opt) is original and len(opt.param_groups[0]["params"]) == 2
        lin(torch.ones(1, 3)).sum().backward()
        opt.step()
        assert float(opt.state[lin.weight]["step"]) == 1.0
    finally:
        optim.uninstall()
    assert torch.optim.AdamW is original
    optim.uninstall()                                           # idempotent
    assert torch.optim.AdamW is original
