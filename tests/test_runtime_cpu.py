"""Host logic of madtp_amd.runtime that needs no GPU."""
import pytest
import torch


def test_registration_hooks_count_only_owned_modules():
    """The process-wide torch registration hooks (parameter re-assignment / replaced sub-module -> the layers re-collect their
    parameter lists) ignore modules that are not part of a mirror model which has collected its parameters: building unrelated
    modules elsewhere in the process must not invalidate anything (round-3 advice)."""
    from madtp_amd import runtime, vit
    e0 = runtime.param_epoch()
    torch.nn.Linear(4, 4)
    torch.nn.TransformerEncoderLayer(16, 2, 32)
    assert runtime.param_epoch() == e0, "a foreign module moved the epoch"
    blk = vit.Block(768, 12, qkv_bias=True)
    assert runtime.param_epoch() == e0, "constructing a mirror block is not a re-assignment"
    runtime.own_modules(blk)  # what Block._weights() does when it collects its parameter list
    blk.mlp.fc1.weight = torch.nn.Parameter(torch.zeros(3072, 768))
    assert runtime.param_epoch() == e0 + 1
    blk.mlp.fc2 = torch.nn.Linear(3072, 768)
    assert runtime.param_epoch() == e0 + 2
    other = vit.Block(768, 12, qkv_bias=True)  # never collected: nothing cached, nothing to invalidate
    other.mlp.fc1.weight = torch.nn.Parameter(torch.zeros(3072, 768))
    assert runtime.param_epoch() == e0 + 2


def test_score_fast_follows_the_precision_mode():
    from madtp_amd import hip, runtime
    prev = runtime.get_precision()
    try:
        for mode, want in (("fp32", 0), ("f16", 1), ("f16x3", 0), ("bf16", 1)):
            runtime.set_precision(mode)
            assert hip._score_fast == (want if runtime._SCORE_FAST else 0), mode
    finally:
        runtime.set_precision(prev)


# ---- parameter-change signature (runtime.signature / reusable / note_updated) behind every prepared-weight cache -----------------
# All of the cache logic runs on CPU tensors with fake builders.  torch.optim.AdamW(fused=True) works on CPU tensors and bumps no
# Parameter._version, like its device kernels.

class _Builds:
    """a fake builder that records the previous value each call was handed"""

    def __init__(self):
        self.prevs = []
        self.build = lambda prev=None: self._build(prev)
        self.build._takes_prev = True

    def _build(self, prev):
        self.prevs.append(prev)
        return object()


def _lookups():
    """{name: (lookup(tensors, builds) -> value)} over a fresh runtime.PreparedCache and a fresh key of backward._cached"""
    from madtp_amd import backward, runtime
    cache, key = runtime.PreparedCache(), ("test", object())
    return {"PreparedCache": lambda ts, b: cache.get("k", ts, b.build), "_cached": lambda ts, b: backward._cached(key, ts, b.build)}


def _grads(lin):
    for p in lin.parameters():
        p.grad = torch.ones_like(p)


def _sgd(lin):
    _grads(lin)
    torch.optim.SGD(lin.parameters(), lr=0.1).step()


def _fused(lin):
    _grads(lin)
    before = [p._version for p in lin.parameters()]
    torch.optim.AdamW(lin.parameters(), lr=0.1, fused=True).step()
    assert [p._version for p in lin.parameters()] == [v + 1 for v in before], "a fused step advances _version by exactly one"


def _mul(lin):
    with torch.no_grad():
        lin.weight.mul_(2.0)


def _note(lin):
    from madtp_amd import runtime
    runtime.note_updated(lin.parameters())


def _data_edit(lin):
    lin.weight.data.mul_(2.0)


def _data_edit_told(lin):
    from madtp_amd import runtime
    lin.weight.data.mul_(2.0)
    runtime.parameters_updated()


def _foreign_step(lin):
    _sgd(torch.nn.Linear(4, 4))


def _new_storage(lin):
    lin.weight.data = torch.zeros(8, 8)


# (what happens, then: "hit", or on a miss which previous value the builder gets)
_SCENARIOS = {"nothing": (lambda lin: None, "hit"), "mul_": (_mul, None), "sgd": (_sgd, "old"), "fused": (_fused, "old"),
              "note_updated": (_note, "old"), "data_edit": (_data_edit, "hit"), "data_edit_told": (_data_edit_told, None),
              "foreign_step": (_foreign_step, "hit"), "new_storage": (_new_storage, None)}
_MISSES = [k for k, (_, want) in _SCENARIOS.items() if want != "hit"]

@pytest.mark.parametrize("which", ["PreparedCache", "_cached"])
@pytest.mark.parametrize("scenario", list(_SCENARIOS))
def test_cache_hit_miss_and_reuse(which, scenario):
    act, want = _SCENARIOS[scenario]
    lookup, b = _lookups()[which], _Builds()
    lin = torch.nn.Linear(8, 8)
    params = [lin.weight, lin.bias]
    v0 = lookup(params, b)
    assert lookup(params, b) is v0 and b.prevs == [None]
    act(lin)
    v1 = lookup(params, b)
    if want == "hit":
        assert v1 is v0 and b.prevs == [None]
    else:
        assert v1 is not v0 and len(b.prevs) == 2
        assert b.prevs[1] is (v0 if want == "old" else None)
        assert lookup(params, b) is v1


def test_precision_change_is_a_miss_without_reuse():
    from madtp_amd import runtime
    lookup, b = _lookups()["PreparedCache"], _Builds()
    lin = torch.nn.Linear(8, 8)
    prev = runtime.get_precision()
    try:
        runtime.set_precision("fp32")
        v0 = lookup([lin.weight], b)
        runtime.set_precision("f16x3")
        _sgd(lin)  # (even with a step in between)
        assert lookup([lin.weight], b) is not v0 and b.prevs == [None, None]
    finally:
        runtime.set_precision(prev)


@pytest.mark.parametrize("which", ["PreparedCache", "_cached"])
def test_none_entries_and_aliases(which):
    lookup, b = _lookups()[which], _Builds()
    lin = torch.nn.Linear(8, 8)
    v0 = lookup([lin.weight, None], b)
    assert lookup([lin.weight, None], b) is v0
    assert lookup([None, lin.weight], b) is not v0
    # a Parameter and its detach() alias alternate under one key (the forward and dgrad of the f16x3 training route), step count >= 1
    lookup, b = _lookups()[which], _Builds()
    _sgd(lin)
    vals = [lookup([w], b) for _ in range(3) for w in (lin.weight, lin.weight.detach())]
    assert len(b.prevs) == 1 and all(v is vals[0] for v in vals)
    # an alias sees a fused step, and - its step count is unknown - gets no previous value
    _fused(lin)
    assert lookup([lin.weight.detach()], b) is not vals[0] and b.prevs == [None, None]
    # ... nor does the Parameter get the value an alias built
    _sgd(lin)
    lookup([lin.weight], b)
    assert b.prevs == [None, None, None]


def test_signature_is_shared_by_aliases_and_sees_each_fact():
    from madtp_amd import runtime
    w = torch.nn.Parameter(torch.zeros(8, 8))
    s0 = runtime.signature([w, None])
    assert s0 == runtime.signature([w.detach(), None]) == runtime.signature((w, None))
    assert runtime.signature([w.detach().view(64), None]) != s0          # shape
    assert runtime.signature([w.detach()[1:], None]) != s0               # address
    _sgd_w = torch.optim.SGD([w], lr=0.1)
    w.grad = torch.ones_like(w)
    _sgd_w.step()
    assert runtime.signature([w, None]) != s0 and runtime.param_step_count(w) == 1   # version
    w.data = torch.zeros(4, 4)
    assert runtime.signature([w])[1] == ((w.data_ptr(), w.device, w.shape),)  # the memoised identity follows new storage


class _FakeLayer:
    def __init__(self):
        import ctypes
        self.lin = torch.nn.Linear(8, 8)
        self._madtp_params = [self.lin.weight, self.lin.bias]
        self._weights = lambda: ctypes.c_int(0)


@pytest.mark.parametrize("scenario", _MISSES)
def test_encoder_weights_follow(scenario):
    from madtp_amd import runtime
    layers, ew = [_FakeLayer(), _FakeLayer()], runtime.EncoderWeights()
    v0 = ew.get(layers)
    _foreign_step(None)
    assert ew.get(layers) is v0
    _SCENARIOS[scenario][0](layers[1].lin)
    v1 = ew.get(layers)
    assert v1 is not v0 and ew.get(layers) is v1


@pytest.mark.parametrize("scenario", list(_SCENARIOS))
def test_check_versions(scenario):
    import types
    from madtp_amd import backward
    act, want = _SCENARIOS[scenario]
    lin, ctx = torch.nn.Linear(8, 8), types.SimpleNamespace()
    params = [lin.weight, None, lin.bias]
    backward._note_versions(ctx, params)
    act(lin)
    if want == "hit":
        backward._check_versions(ctx, params, "layer backward")
    else:
        with pytest.raises(RuntimeError, match="modified in place"):
            backward._check_versions(ctx, params, "layer backward")


def test_scaled_value_follows_updates_without_version_bumps():
    """the head-masked value projection of a MED layer (bert._scaled_value) after a fused step, note_updated and a told .data edit"""
    import types
    from madtp_amd import bert, runtime
    layer = types.SimpleNamespace()
    sm = types.SimpleNamespace(value=torch.nn.Linear(8, 8), attention_head_size=2)
    hm = torch.linspace(0.5, 1.5, 4)
    rows = hm.repeat_interleave(2)

    def check():
        h = bert.MedBertLayer._scaled_value(layer, sm, hm)
        assert torch.equal(h.weight, sm.value.weight.detach() * rows[:, None]) and torch.equal(h.bias, sm.value.bias.detach() * rows)
        return h

    h0 = check()
    assert check() is h0
    _fused(sm.value)
    h1 = check()
    assert h1 is not h0
    with torch.no_grad():
        sm.value.weight.data.add_(1.0)      # (stands for a kernel that writes behind torch's back)
    runtime.note_updated([sm.value.weight])
    h2 = check()
    assert h2 is not h1
    sm.value.bias.data.add_(1.0)
    runtime.parameters_updated()
    assert check() is not h2
