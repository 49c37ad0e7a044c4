"""madtp_itc_loss for wide features (512 < D <= 1024, the exact-f32 MFMA kernel of csrc/retrieval.hip) on a real MI355X:
float64 parity at the tolerances of test_retrieval_train_gpu.py::test_itc_loss_matches_float64 (same feature, duplicate-id and
queue-id recipe), bit repeatability (also across a large call in between: stale workspace), the autograd route and the range
check.  (512, 17, 48) is the last narrow D: both sides of the dispatch boundary sit in one table."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (D, B, Q, alpha, temp)
CASES = [(576, 1, 0, .4, .07),          # the first wide D, one row, no queue
         (768, 3, 12, .4, .07),         # N = 15, under one MFMA tile
         (768, 3, 12, 0., .001),        # large scores
         (768, 16, 48, .4, .07),        # one full row tile, one queue key tile short of full
         (768, 17, 48, .4, .07),        # one row past a 16-row tile
         (1024, 33, 130, 1.0, .07),     # one row past 32; Q % 4 != 0 (the scalar staging of queue tiles)
         (1024, 256, 64, .4, .07),      # the row limit
         (768, 16, 57600, .4, .07),     # the driver's shape
         (1024, 32, 57600, 1.0, .001),  # the largest case
         (512, 17, 48, .4, .07)]        # the narrow kernel next to the boundary


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


def _rel(a, b, floor):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), floor)


def _feats(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(n, D, generator=g), dim=-1)


def _itc_ref(q, qm, kb, queue, idx, idxq, temp, alpha):
    """blip_retrieval.py:116-150 for one direction in float64, with autograd for dq and dtemp of the mean loss."""
    q = q.double().clone().requires_grad_(True)
    t = torch.tensor(float(temp), dtype=torch.float64, requires_grad=True)
    keys = torch.cat([kb.double().t(), queue.double()], 1)
    ids = torch.cat([idx, idxq]).view(1, -1)
    pos = (idx.view(-1, 1) == ids).double()
    with torch.no_grad():
        tgt = alpha * F.softmax(qm.double() @ keys / t, 1) + (1 - alpha) * pos / pos.sum(1, keepdim=True)
    loss = -(F.log_softmax(q @ keys / t, 1) * tgt).sum(1)
    loss.mean().backward()
    return loss.detach(), q.grad, t.grad


def _inputs(D, B, Q, temp):
    q, qm, kb = _feats(B, D, 1), _feats(B, D, 2), _feats(B, D, 3)
    queue = _feats(Q, D, 4).t().contiguous()
    idx = torch.arange(B) % max(1, B - 1) + 5   # duplicates in the batch
    idxq = torch.full((Q,), -100, dtype=torch.long)
    if Q:
        idxq[:: max(1, Q // 7)] = 5                  # queue entries sharing a batch id
        idxq[1] = 6
    return q, qm, kb, queue, idx, idxq, torch.tensor([temp], dtype=torch.float32)


def _cuda(args, alpha):
    return tuple(a.cuda() for a in args) + (alpha,)


@pytest.mark.parametrize("D,B,Q,alpha,temp", CASES)
def test_itc_wide_matches_float64(hip, D, B, Q, alpha, temp):
    cpu = _inputs(D, B, Q, temp)
    l_ref, dq_ref, dt_ref = _itc_ref(*cpu[:6], float(cpu[6]), alpha)
    args = _cuda(cpu, alpha)
    loss, dq, dt = hip.itc_loss(*args)
    tol = 1e-5 if temp >= 0.07 else 1e-4
    e = (_rel(loss.cpu(), l_ref, 1.0), _rel(dq.cpu(), dq_ref, 1e-3), abs(float(dt) - float(dt_ref)) / max(abs(float(dt_ref)), 1e-3))
    print(f"itc_wide D={D} B={B} Q={Q} alpha={alpha} temp={temp}: loss {e[0]:.2e} dq {e[1]:.2e} dtemp {e[2]:.2e} (tol {tol})")
    assert e[0] < tol, e
    assert e[1] < tol, e
    assert e[2] <= tol, (e, float(dt), float(dt_ref))
    loss2, dq2, dt2 = hip.itc_loss(*args)
    assert torch.equal(loss, loss2) and torch.equal(dq, dq2) and torch.equal(dt, dt2)  # fixed-order reductions


def test_itc_wide_same_bits_after_a_large_call(hip):
    small = _cuda(_inputs(768, 3, 12, .07), .4)
    big = _cuda(_inputs(768, 16, 57600, .07), .4)
    first = hip.itc_loss(*small)
    hip.itc_loss(*big)
    again = hip.itc_loss(*small)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_itc_wide_autograd_route(hip):
    from madtp_amd.blip_retrieval import _ItcLoss
    q, qm, kb, queue, idx, idxq, tt, alpha = _cuda(_inputs(768, 3, 12, .07), .4)
    _, dq, dt = hip.itc_loss(q, qm, kb, queue, idx, idxq, tt, alpha)
    qg = q.clone().requires_grad_(True)
    tg = tt.clone().requires_grad_(True)
    (2 * _ItcLoss.apply(qg, tg, qm, kb, queue, idx, idxq, alpha)).backward()
    assert torch.equal(qg.grad, 2 * dq)
    assert torch.equal(tg.grad, (2 * dt).reshape(tg.shape))


def test_itc_above_1024_raises(hip):
    with pytest.raises(RuntimeError):
        hip.itc_loss(*_cuda(_inputs(1088, 3, 12, .07), .4))
