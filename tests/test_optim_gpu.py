"""madtp_amd.optim.AdamW (madtp_adamw_step, csrc/optim.hip) on a real MI355X.

Tolerance (derived, not tuned; u = 2^-23): one step from a given f32 state (p0, g, m0, v0) against a float64 restatement of

    p1 = p * decay;  m' = m + w1 (g - m);  v' = v beta2 + w2 g g;  p' = p1 - step_size (m' / (sqrt(v') / bc2_sqrt + eps))

on those same f32 values and the f32-rounded scalars:

    |dm| <= 4u (|m0| + |g|)        |dv| <= 4u v'        |dp| <= 4u (|p0| + step_size (|m0| + |g|) / denom)

(two to six f32 roundings each; m' can cancel, so its error scales with |m0| + |g| and carries into p).  torch's own CPU
single-tensor step stays within 1.16u / 1.35u / 1.25u of those denominators, so 4 leaves a 3x margin for another FMA contraction.
Every parity check also runs torch's CPU single-tensor step from the same state and holds it to the same bounds."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -23
K = 4.0


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


def _hp(group):
    return (group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"])


def _snapshot(opt):
    """the state every parameter with a gradient is about to step from, on the CPU: {param: (p0, g, m0, v0, t, hp)}"""
    snap = {}
    for group in opt.param_groups:
        for p in group["params"]:
            if p.grad is None:
                continue
            st = opt.state.get(p, {})
            m0 = st["exp_avg"].detach().cpu().clone() if "exp_avg" in st else torch.zeros(p.shape)
            v0 = st["exp_avg_sq"].detach().cpu().clone() if "exp_avg_sq" in st else torch.zeros(p.shape)
            t = int(float(st["step"])) + 1 if "step" in st else 1
            snap[p] = (p.detach().cpu().clone(), p.grad.detach().cpu().clone(), m0, v0, t, _hp(group))
    return snap


def _torch_cpu_step(p0, g, m0, v0, t, hp):
    """torch's single-tensor AdamW on the CPU from the given state (flat f32 tensors) -> (p, m, v)"""
    lr, b1, b2, eps, wd = hp
    pc = p0.clone().requires_grad_(True)
    ref = torch.optim.AdamW([pc], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    ref.state[pc] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    pc.grad = g.clone()
    ref.step()
    assert float(ref.state[pc]["step"]) == t
    return pc.detach(), ref.state[pc]["exp_avg"], ref.state[pc]["exp_avg_sq"]


def _worst(got, ref, bound):
    """max of |got - ref| / bound over the elements (0 where both vanish; inf where a zero bound is exceeded)"""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


def _verify(snap, opt, what, extra=None):
    """After opt.step(): every stepped parameter within the bounds of the float64 restatement of its own pre-step state - and
    torch's CPU single-tensor step from that state as well.  Tensors that share (hyper-parameters, step) are checked as one flat
    tensor.  extra: {param: (p, m, v)} results of another implementation to hold to the same bounds."""
    from madtp_amd import optim
    torch.cuda.synchronize()
    buckets = {}
    for p, (p0, g, m0, v0, t, hp) in snap.items():
        buckets.setdefault((hp, t), []).append(p)
    for (hp, t), ps in buckets.items():
        cat = lambda i: torch.cat([snap[p][i].reshape(-1) for p in ps])  # noqa: E731
        p0, g, m0, v0 = cat(0), cat(1), cat(2), cat(3)
        decay, w1, beta2, w2, step_size, bc2_sqrt, eps = optim.adamw_scalars(*hp, t)
        P, G, M, V = p0.double(), g.double(), m0.double(), v0.double()
        m_ref = M + w1 * (G - M)
        v_ref = V * beta2 + w2 * G * G
        denom = v_ref.sqrt() / bc2_sqrt + eps
        p_ref = P * decay - step_size * (m_ref / denom)
        bm = K * U * (M.abs() + G.abs())
        bv = K * U * v_ref
        bp = K * U * (P.abs() + step_size * (M.abs() + G.abs()) / denom)
        results = {"torch CPU single-tensor": _torch_cpu_step(p0, g, m0, v0, t, hp),
                   what: (torch.cat([p.detach().cpu().reshape(-1) for p in ps]),
                          torch.cat([opt.state[p]["exp_avg"].cpu().reshape(-1) for p in ps]),
                          torch.cat([opt.state[p]["exp_avg_sq"].cpu().reshape(-1) for p in ps]))}
        if extra is not None:
            results["other"] = tuple(torch.cat([extra[p][i].detach().cpu().reshape(-1) for p in ps]) for i in range(3))
        for name, (pg, mg, vg) in results.items():
            wm, wv, wp = _worst(mg, m_ref, bm), _worst(vg, v_ref, bv), _worst(pg, p_ref, bp)
            print(f"{name}: step {t} hp {hp}: {p0.numel()} elements, worst error / bound: m {wm:.3f} v {wv:.3f} p {wp:.3f}")
            assert wm <= 1.0 and wv <= 1.0 and wp <= 1.0, (name, t, hp, wm, wv, wp)
        for p in ps:
            assert float(opt.state[p]["step"]) == t and opt.state[p]["step"].dtype == torch.float32 and not opt.state[p]["step"].is_cuda


def _grad_like(p, gen, all_zero=False):
    """four decades of scale, about a fifth exact zeros"""
    if all_zero:
        return torch.zeros_like(p)
    g = torch.randn(p.shape, generator=gen) * 10.0 ** torch.randint(-3, 1, p.shape, generator=gen).float()
    g[torch.rand(p.shape, generator=gen) < 0.2] = 0.0
    return g.to(p.device)


def _params(shapes, seed, view_numel=()):
    """GPU f32 leaf parameters; view_numel: extra 1-D parameters that are views from element 1 of a larger buffer"""
    gen = torch.Generator().manual_seed(seed)
    ps = [(torch.randn(s, generator=gen) * 0.05).cuda().requires_grad_(True) for s in shapes]
    bufs = []
    for n in view_numel:
        buf = (torch.randn(n + 9, generator=gen) * 0.05).cuda()
        v = buf[1:n + 1].detach().requires_grad_(True)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous() and v.numel() == n
        bufs.append(buf)
        ps.append(v)
    return ps, bufs


def _kernel_path_shapes(hip):
    E = hip.ADAMW_PER_BLOCK
    assert E == 4096 and hip.load().madtp_adamw_blocks(E) == 1 and hip.load().madtp_adamw_blocks(E + 1) == 2
    sizes = [0, 1, 3, 4, 5, E - 1, E, E + 1, 2 * E + 5]
    shapes = [(n,) for n in sizes] * 3 + [(3, 5), (64, 65), (7, 0, 2), (2, E // 2 + 1), (1,), (E + 4,), (2 * E,), (13, 17, 3), (E - 4,)]
    return shapes, [E + 5, 3, 2 * E + 6]


def test_kernel_paths_six_steps(hip):
    """~40 tensors in one table: 0, 1, 3, 4, 5 elements, one below / at / one above a workgroup's elements, two workgroups plus a
    tail, 4-byte-aligned views (the element-wise path); the bounds at every step from the test's own state; on the first step
    (m = v = 0) an element with g = 0 moves by the weight decay alone."""
    from madtp_amd import optim
    shapes, views = _kernel_path_shapes(hip)
    ps, bufs = _params(shapes, 0, views)
    guard = [b.clone() for b in bufs]
    assert len(ps) == 39
    opt = optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
    gen = torch.Generator().manual_seed(1)
    zero_first = {5, 7, 36}  # tensors whose first gradient is all zeros (one of them a view)
    for step in range(6):
        for i, p in enumerate(ps):
            p.grad = _grad_like(p, gen, all_zero=(step == 0 and i in zero_first))
        snap = _snapshot(opt)
        opt.step()
        _verify(snap, opt, "madtp_adamw_step")
        if step == 0:
            decay = np.float32(optim.adamw_scalars(1e-3, 0.9, 0.98, 1e-8, 0.05, 1)[0])
            for p, (p0, g, _, _, _, _) in snap.items():
                z = (g == 0).numpy()
                assert np.array_equal(p.detach().cpu().numpy()[z], (p0.numpy() * decay)[z])
                assert float(opt.state[p]["exp_avg"].cpu()[torch.from_numpy(z)].abs().sum()) == 0.0
    assert len(opt.tables()) == 1
    for buf, g0, n in zip(bufs, guard, views):  # nothing outside the views was written
        assert torch.equal(buf[:1], g0[:1]) and torch.equal(buf[n + 1:], g0[n + 1:])


def test_parameters_without_gradient_are_skipped_and_keep_their_own_step(hip):
    from madtp_amd import optim
    ps, _ = _params([(5,), (4097,), (64, 3), (9000,), (17,), (4,)], 2)
    late = [ps[1], ps[4]]
    before = [p.detach().clone() for p in late]
    opt = optim.AdamW(ps, lr=1e-3, weight_decay=0.05)
    gen = torch.Generator().manual_seed(3)
    for step in range(5):
        for p in ps:
            p.grad = None if (step < 2 and any(p is q for q in late)) else _grad_like(p, gen)
        snap = _snapshot(opt)
        opt.step()
        _verify(snap, opt, "madtp_adamw_step")
        if step < 2:
            for p, b in zip(late, before):
                assert torch.equal(p.detach(), b) and p not in opt.state and p not in snap
            assert len(opt.tables()) == 1
        else:
            assert [float(opt.state[p]["step"]) for p in late] == [step - 1.0] * 2
            assert float(opt.state[ps[0]]["step"]) == step + 1.0
            assert len(opt.tables()) == 2  # two buckets: two launches


def test_param_groups_and_lr_reassigned_between_steps(hip):
    """the no_weight_decay split; lr assigned as cosine_lr_schedule does (param_group["lr"] = ...): used on the very next step"""
    from madtp_amd import optim
    ps, _ = _params([(300,), (4100,), (33, 7), (5,), (8200,)], 4)
    opt = optim.AdamW([{"params": ps[:3], "weight_decay": 0.05}, {"params": ps[3:], "weight_decay": 0.0}], lr=1e-3, betas=(0.9, 0.999))
    gen = torch.Generator().manual_seed(5)
    for step, lr in enumerate([1e-3, 5e-4, 5e-4, 1e-5]):
        for group in opt.param_groups:
            group["lr"] = lr
        for i, p in enumerate(ps):
            p.grad = _grad_like(p, gen, all_zero=(step == 0 and i == 4))
        snap = _snapshot(opt)
        assert all(s[5][0] == lr for s in snap.values())
        opt.step()
        _verify(snap, opt, "madtp_adamw_step")  # (the reference uses the new lr: half the old update is far outside 4u)
        if step == 0:
            assert torch.equal(ps[4].detach().cpu(), snap[ps[4]][0])  # no weight decay, g = m = v = 0: bit-unchanged
    assert len(opt.tables()) == 2


def test_table_follows_moving_gradient_addresses(hip):
    from madtp_amd import optim
    ps, _ = _params([(300,), (4100,), (33, 7)], 6)
    opt = optim.AdamW(ps, lr=1e-3, weight_decay=0.05)
    gen = torch.Generator().manual_seed(7)
    kept = []
    for step in range(4):
        old = [p.grad for p in ps]
        kept.append(old)  # the old gradients stay alive: the new ones cannot land at their addresses
        opt.zero_grad()   # set_to_none=True, torch's default
        assert all(p.grad is None for p in ps)
        for p in ps:
            p.grad = _grad_like(p, gen)
        if step:
            assert all(p.grad.data_ptr() != o.data_ptr() for p, o in zip(ps, old))
        snap = _snapshot(opt)
        opt.step()
        _verify(snap, opt, "madtp_adamw_step")
        (table,) = opt.tables()
        assert table.rebuilds == step + 1
    for p in ps:  # gradients rewritten in place: same addresses, no upload
        p.grad.copy_(_grad_like(p, gen))
    snap = _snapshot(opt)
    opt.step()
    _verify(snap, opt, "madtp_adamw_step")
    assert opt.tables()[0].rebuilds == 4


@pytest.mark.parametrize("direction", ["to_torch", "from_torch"])
def test_state_dict_interchanges_with_torch_adamw(hip, direction):
    from madtp_amd import optim
    shapes = [(300,), (4100,), (33, 7), (0,), (5,)]
    hp = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
    ps, _ = _params(shapes, 8)
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    make = {"ours": lambda params: optim.AdamW(params, **hp), "torch": lambda params: torch.optim.AdamW(params, foreach=False, **hp)}
    first, second = ("ours", "torch") if direction == "to_torch" else ("torch", "ours")
    a = make[first](ps)
    gen = torch.Generator().manual_seed(9)
    for _ in range(2):
        for p in ps:
            p.grad = _grad_like(p, gen)
        a.step()
    sd = a.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(sd["param_groups"][0]) == set(make["torch"](qs).state_dict()["param_groups"][0])
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    b = make[second](qs)
    b.load_state_dict(copy.deepcopy(sd))  # (load_state_dict keeps tensors of the right dtype and device by reference)
    if second == "torch":
        for group in b.param_groups:
            group["foreach"] = False  # (the loaded group carried this class's foreach=None)
    for p, q in zip(ps, qs):
        assert torch.equal(a.state[p]["exp_avg"], b.state[q]["exp_avg"]) and a.state[p]["exp_avg"] is not b.state[q]["exp_avg"]
        assert float(b.state[q]["step"]) == 2.0
        p.grad = _grad_like(p, gen)
        q.grad = p.grad.clone()
    ours, theirs, mine, other = (a, b, ps, qs) if first == "ours" else (b, a, qs, ps)
    snap = _snapshot(ours)
    a.step()
    b.step()
    extra = {m: (o.detach(), theirs.state[o]["exp_avg"], theirs.state[o]["exp_avg_sq"]) for m, o in zip(mine, other)}
    _verify(snap, ours, "madtp_adamw_step", extra=extra)
    assert all(float(theirs.state[o]["step"]) == 3.0 for o in other)


def test_identical_calls_give_identical_bits(hip):
    from madtp_amd import optim
    shapes, views = _kernel_path_shapes(hip)

    def run():
        ps, _ = _params(shapes, 10, views)
        opt = optim.AdamW(ps, lr=1e-3, weight_decay=0.05)
        gen = torch.Generator().manual_seed(11)
        for _ in range(6):
            for p in ps:
                p.grad = _grad_like(p, gen)
            opt.step()
        torch.cuda.synchronize()
        return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]

    for x, y in zip(run(), run()):
        assert all(torch.equal(s, t) for s, t in zip(x, y))


def test_prepared_weights_follow_this_optimizer(hip):
    """a mirror Block in the fp32 mode: forward, backward, step() with this class, forward again - the second output differs from
    the first and equals that of a fresh module loaded with the updated parameters (the step ran through torch's hook wrapper,
    runtime._on_optimizer_step bumped the parameters' update counts)"""
    from madtp_amd import optim, runtime, vit
    torch.manual_seed(0)
    blk = vit.Block(768, 12, qkv_bias=True).cuda().eval()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(2, 50, 768, generator=gen).cuda().requires_grad_(True)
    w = torch.randn(2, 50, 768, generator=gen).cuda()
    opt = optim.AdamW(blk.parameters(), lr=1e-2)
    steps0 = [getattr(p, "_madtp_steps", 0) for p in blk.parameters()]
    versions0 = [p._version for p in blk.parameters()]
    with runtime.precision("fp32"):
        y0 = blk(x, temperature=0)
        (y0 * w).sum().backward()
        opt.step()
        assert [getattr(p, "_madtp_steps", 0) for p in blk.parameters()] == [s + 1 for s in steps0]
        assert [p._version for p in blk.parameters()] == [v + 1 for v in versions0]
        with torch.no_grad():
            y1 = blk(x, temperature=0)
            fresh = vit.Block(768, 12, qkv_bias=True).cuda().eval()
            fresh.load_state_dict(blk.state_dict())
            y2 = fresh(x, temperature=0)
    rel = float((y1 - y0.detach()).abs().max()) / float(y0.detach().abs().max())
    assert rel > 1e-2, "the step did not reach the prepared weights"
    assert torch.equal(y1, y2)


def test_nlvr_three_steps_against_torchs_own_two_implementations(hip):
    """trainstep_nlvr_b2's model and batch, f16x3, three steps: the loss after each step with this class against
    torch.optim.AdamW(foreach=False); the yardstick is the difference between torch's own foreach=False and foreach=True legs on
    the same box: within 2x that per step (floor 1e-6).  The loss goes down."""
    from madtp_amd import harness, optim, runtime
    g = np.load(os.path.join(ROOT, "tests", "golden", "trainstep_nlvr_b2.npz"))
    B, size, L, T, seed = int(g["B"]), int(g["size"]), int(g["L"]), float(g["temperature"]), int(g["seed"])
    model = harness.build_nlvr(size, seed, "cuda")
    for p_ in model.parameters():
        p_.requires_grad_(True)
        p_.grad = None
    start = [p_.detach().clone() for p_ in model.parameters()]
    images, text, _ = harness.nlvr_inputs(B, size, L, seed, "cuda", pad_tail=int(g["pad_tail"]))
    targets = (torch.arange(B) % 2).cuda()
    hp = dict(lr=2e-5, weight_decay=0.05)
    legs = {"single": lambda ps: torch.optim.AdamW(ps, foreach=False, **hp), "foreach": lambda ps: torch.optim.AdamW(ps, foreach=True, **hp),
            "madtp": lambda ps: optim.AdamW(ps, **hp),
            "fused": lambda ps: torch.optim.AdamW(ps, fused=True, **hp)}  # (reported in the message only, no part of the bound)
    losses = {}
    with runtime.precision("f16x3"), runtime.training_f16x3():
        for name, make in legs.items():
            with torch.no_grad():
                for p_, s in zip(model.parameters(), start):
                    p_.copy_(s)
            opt = make(model.parameters())
            out = []
            for i in range(4):  # the loss before the first step, then after each of the three
                opt.zero_grad()
                lo, lf = model(images, text, targets, temperature=T, train=True)
                loss = lo + 0.1 * lf
                out.append(float(loss.detach()))
                if i < 3:
                    loss.backward()
                    opt.step()
            losses[name] = out
    msg = "; ".join(f"{k}: {[f'{v:.7f}' for v in vs]}" for k, vs in losses.items())
    print("nlvr three steps, loss before and after steps 1-3:", msg)
    assert all(np.isfinite(v).all() for v in losses.values()), msg
    for i in range(4):
        yard = abs(losses["foreach"][i] - losses["single"][i])
        ours = abs(losses["madtp"][i] - losses["single"][i])
        assert ours <= max(2.0 * yard, 1e-6), f"step {i}: |madtp - single| {ours:.3e} vs |foreach - single| {yard:.3e}; {msg}"
    assert losses["madtp"][-1] < losses["madtp"][0], msg


def test_grad_scaler_generic_route(hip):
    """scale(loss).backward(); step(opt); update() with a power-of-two scale equals the unscaled step bit for bit; one inf in a
    gradient and nothing changes, no step advances"""
    from madtp_amd import optim
    gen = torch.Generator().manual_seed(12)
    a, b = torch.randn(4100, generator=gen).cuda(), torch.randn(33, 7, generator=gen).cuda()

    def setup():
        ps, _ = _params([(4100,), (33, 7)], 13)
        return ps, optim.AdamW(ps, lr=1e-3, weight_decay=0.05)

    def loss_of(ps):
        return (ps[0] * a).sum() + (ps[1] * ps[1] * b).sum()

    plain, opt_p = setup()
    scaled, opt_s = setup()
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    for _ in range(2):
        opt_p.zero_grad()
        loss_of(plain).backward()
        opt_p.step()
        opt_s.zero_grad()
        scaler.scale(loss_of(scaled)).backward()
        scaler.step(opt_s)
        scaler.update()
    assert scaler.get_scale() == 2.0 ** 16
    for p, q in zip(plain, scaled):
        assert torch.equal(p, q) and torch.equal(opt_p.state[p]["exp_avg"], opt_s.state[q]["exp_avg"])
        assert torch.equal(opt_p.state[p]["exp_avg_sq"], opt_s.state[q]["exp_avg_sq"]) and float(opt_s.state[q]["step"]) == 2.0
    keep = [(q.detach().clone(), opt_s.state[q]["exp_avg"].clone(), opt_s.state[q]["exp_avg_sq"].clone()) for q in scaled]
    opt_s.zero_grad()
    scaler.scale(loss_of(scaled)).backward()
    scaled[0].grad[17] = float("inf")
    scaler.step(opt_s)
    scaler.update()
    assert scaler.get_scale() == 2.0 ** 15
    for q, (p0, m0, v0) in zip(scaled, keep):
        assert torch.equal(q, p0) and torch.equal(opt_s.state[q]["exp_avg"], m0) and torch.equal(opt_s.state[q]["exp_avg_sq"], v0)
        assert float(opt_s.state[q]["step"]) == 2.0
