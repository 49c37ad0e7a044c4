"""The retrieval training step on a real MI355X (BLIP_Retrieval(evaluate=False).forward, csrc/retrieval.hip):
  * madtp_itc_loss / madtp_ema_update / madtp_itm_negatives against float64 / torch restatements written here,
  * one training step against the reference's own (tests/golden/trainstep_retr_*.npz, tools/make_golden.py::retr_train_case):
    losses, every gradient, the negatives drawn, momentum parameters, queues, pointer, and the losses of a second step,
  * model.train() dropout behaviour, a few AdamW steps, the full-size step."""
import glob
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "trainstep_retr_*.npz")))
TRAIN_MODES = ["fp32", "f16x3"]


@pytest.fixture(scope="module")
def hip():
    from madtp_amd import build, hip as h
    build.build(verbose=False)
    h.load()
    assert torch.cuda.is_available()
    return h


def _train_mode(mode):
    import contextlib
    from madtp_amd import runtime
    st = contextlib.ExitStack()
    st.enter_context(runtime.precision(mode))
    if mode == "f16x3":
        st.enter_context(runtime.training_f16x3())
    return st


def _rel(a, b, floor=1e-30):
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


ITC_CASES = [(1, 0, 0.4, 0.07), (3, 12, 0.4, 0.07), (3, 12, 0.0, 0.001), (3, 12, 1.0, 0.5), (32, 12, 0.4, 0.5),
             (32, 57600, 0.4, 0.07), (32, 57600, 1.0, 0.001), (32, 57600, 0.0, 0.5), (1, 57600, 0.4, 0.07), (32, 0, 1.0, 0.07)]


@pytest.mark.parametrize("B,Q,alpha,temp", ITC_CASES)
def test_itc_loss_matches_float64(hip, B, Q, alpha, temp):
    D = 256
    q, qm, kb = _feats(B, D, 1), _feats(B, D, 2), _feats(B, D, 3)
    queue = _feats(Q, D, 4).t().contiguous()
    idx = torch.arange(B) % max(1, B - 1) + 5   # duplicates in the batch
    idxq = torch.full((Q,), -100, dtype=torch.long)
    if Q:
        idxq[:: max(1, Q // 7)] = 5                  # queue entries sharing a batch id
        idxq[1] = 6
    tt = torch.tensor([temp], dtype=torch.float32)
    l_ref, dq_ref, dt_ref = _itc_ref(q, qm, kb, queue, idx, idxq, float(tt), alpha)
    args = (q.cuda(), qm.cuda(), kb.cuda(), queue.cuda(), idx.cuda(), idxq.cuda(), tt.cuda(), alpha)
    loss, dq, dt = hip.itc_loss(*args)
    # (B = 1 with an empty queue: the loss and its gradient are exactly 0 - compared against the unit scale of log N instead)
    # temp = 0.001: |s| reaches ~1e3, where the f32 rounding of s alone is ~6e-5 absolute in every exponent - 1e-4 there
    tol = 1e-5 if temp >= 0.07 else 1e-4
    assert _rel(loss.cpu(), l_ref, 1.0) < tol, _rel(loss.cpu(), l_ref, 1.0)
    assert _rel(dq.cpu(), dq_ref, 1e-3) < tol, _rel(dq.cpu(), dq_ref, 1e-3)
    assert abs(float(dt) - float(dt_ref)) <= tol * max(abs(float(dt_ref)), 1e-3), (float(dt), float(dt_ref))
    loss2, dq2, dt2 = hip.itc_loss(*args)
    assert torch.equal(loss, loss2) and torch.equal(dq, dq2) and torch.equal(dt, dt2)  # fixed-order reductions


def _neg_ref(f, g, idx, idx_w, temp, u):
    w = F.softmax(f @ g.t() / temp, dim=1)
    w = w.masked_fill(idx.view(-1, 1) == idx_w.view(1, -1), 0)
    out = []
    for b in range(f.shape[0]):
        c = torch.cumsum(w[b], 0)
        if float(c[-1]) == 0:
            out.append(-1)
            continue
        out.append(int(torch.nonzero(c > u[b] * c[-1])[0, 0]))
    return out


@pytest.mark.parametrize("B,world", [(3, 1), (8, 1), (8, 4), (32, 2)])
def test_itm_negatives_match_inverse_cdf(hip, B, world):
    D, Bw = 256, B * world
    img, txt = _feats(B, D, 11), _feats(B, D, 12)
    img_w = torch.cat([img, _feats(Bw - B, D, 13)]) if world > 1 else img
    txt_w = torch.cat([txt, _feats(Bw - B, D, 14)]) if world > 1 else txt
    idx = torch.arange(B) // 2
    idx_w = torch.cat([idx, torch.arange(Bw - B) // 3])
    u = torch.rand(2, B, generator=torch.Generator().manual_seed(B))
    temp = torch.tensor([0.07])
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    neg = hip.itm_negatives(img.cuda(), txt.cuda(), img_w.cuda(), txt_w.cuda(), idx.cuda(), idx_w.cuda(), temp.cuda(), u.cuda(), flag)
    ref0 = _neg_ref(txt.cuda(), img_w.cuda(), idx.cuda(), idx_w.cuda(), 0.07, u[0].cuda())
    ref1 = _neg_ref(img.cuda(), txt_w.cuda(), idx.cuda(), idx_w.cuda(), 0.07, u[1].cuda())
    assert neg.cpu().tolist() == [ref0, ref1]
    assert int(flag) == 0
    # every column shares the row's id: -1 and the flag
    same = torch.zeros(Bw, dtype=torch.long, device="cuda")
    neg = hip.itm_negatives(img.cuda(), txt.cuda(), img_w.cuda(), txt_w.cuda(), same[:B].contiguous(), same, temp.cuda(), u.cuda(), flag)
    assert bool((neg == -1).all()) and int(flag) == 1


def _fixture_model(g):
    from madtp_amd import synth
    from madtp_amd.blip_retrieval import BLIP_Retrieval
    model = BLIP_Retrieval(image_size=int(g["size"]), queue_size=int(g["queue_size"]), evaluate=False)
    sd = synth.fill_state_dict(model, int(g["seed"]))
    sd["image_queue"] = torch.from_numpy(g["init_image_queue"])
    sd["text_queue"] = torch.from_numpy(g["init_text_queue"])
    sd["idx_queue"] = torch.from_numpy(g["init_idx_queue"])
    sd["ptr_queue"] = torch.tensor([int(g["init_ptr"])])
    sd["temp"] = torch.tensor(float(g["init_temp"]))
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval()


def _fixture_inputs(g):
    from madtp_amd import harness, synth
    B, L, seed = int(g["B"]), int(g["L"]), int(g["seed"])
    images = synth.synth_images(B, int(g["size"]), seed).cuda()
    ids = synth.synth_token_ids(B, L, seed, first_id=101)
    cap = {"input_ids": ids.cuda(), "attention_mask": harness.padded_mask(B, L, int(g["pad_tail"])).cuda()}
    return images, cap, torch.from_numpy(g["idx"]).cuda()


def _lens(layers, n0):
    """sequence length (CLS included) after each layer of the last call, from the layers' last_prune records"""
    out, n = [], n0
    for layer in layers:
        info = layer.last_prune
        if info is not None and info.get("pruned"):
            n = int(info["k"]) + 2
        out.append(n)
    return out


def _check_losses(losses, ref, what):
    l = [float(x.detach()) for x in losses]
    assert abs(l[0] - ref[0]) < 1e-3 * abs(ref[0]), (what, "loss_ita", l[0], ref[0])
    assert abs(l[1] - ref[1]) < 1e-3 * abs(ref[1]), (what, "loss_itm", l[1], ref[1])
    assert abs(l[2] - ref[2]) < 1e-4 * max(1.0, abs(ref[2])), (what, "loss_fdt", l[2], ref[2])
    assert abs(l[3] - ref[3]) < 1e-4 * max(1.0, abs(ref[3])), (what, "loss_fdt_m", l[3], ref[3])


@pytest.mark.parametrize("mode", TRAIN_MODES)
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c)[:-4] for c in CASES])
def test_retrieval_training_step_matches_reference(hip, path, mode):
    from tests import grad_case
    g = np.load(path)
    model = _fixture_model(g)
    images, cap, idx = _fixture_inputs(g)
    model.itm_uniforms = torch.from_numpy(g["u"]).cuda()
    alpha, T = float(g["alpha"]), float(g["temperature"])
    with _train_mode(mode):
        losses = model(images, cap, alpha, idx, temperature=T, train=True)
        _check_losses(losses, g["losses"], mode)
        (losses[0] + losses[1] + 0.1 * losses[2] + 0.1 * losses[3]).backward()
    assert model.last_negatives.cpu().numpy().tolist() == g["neg"].tolist()
    # per-layer lengths of all four towers (the student text encoder's last call is the negatives' multimodal pass)
    n_img, L = (int(g["size"]) // 16) ** 2 + 1, int(g["L"])
    assert _lens(model.visual_encoder.blocks, n_img) == g["vit_lens"].tolist()
    assert _lens(model.visual_encoder_m.blocks, n_img) == g["vit_m_lens"].tolist()
    assert _lens(model.text_encoder_m.encoder.layer, L) == g["txt_m_lens"].tolist()
    assert _lens(model.text_encoder.encoder.layer, L) == g["txt_lens"].tolist()[-len(model.text_encoder.encoder.layer):]
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    missing = [k[2:-7] for k in g.files if k.startswith("g_") and k.endswith("_sample") and k[2:-7] not in grads]
    assert not missing, missing[:5]
    grad_case.check_against_fixture(g, grads, 1e-3, f"HIP retrieval training step ({mode}) vs reference")
    # momentum parameters after the EMA: bit-exact (same f32 inputs, same three roundings)
    params = dict(model.named_parameters())
    for k in g.files:
        if k.startswith("m_"):
            flat = params[k[2:]].detach().reshape(-1).cpu()
            got = flat[torch.from_numpy(grad_case.grad_sample_index(flat.numel(), 16, stride=104729))].numpy()
            assert np.array_equal(got, g[k]), k
    assert _rel(model.image_queue.cpu(), torch.from_numpy(g["image_queue"])) < 1e-4
    assert _rel(model.text_queue.cpu(), torch.from_numpy(g["text_queue"])) < 1e-4
    assert np.array_equal(model.idx_queue.cpu().numpy(), g["idx_queue"]) and int(model.ptr_queue[0]) == int(g["ptr"])
    torch.optim.SGD([p for p in model.parameters() if p.grad is not None], lr=float(g["lr"])).step()
    with _train_mode(mode), torch.no_grad():
        losses2 = model(images, cap, alpha, idx, temperature=T, train=True)
    _check_losses(losses2, g["losses2"], mode + " second step")
    assert model.last_negatives.cpu().numpy().tolist() == g["neg2"].tolist()


def test_ema_update_bit_exact_and_no_stale_cache(hip):
    from madtp_amd import runtime
    g = np.load(CASES[0])
    model = _fixture_model(g)
    with torch.no_grad():
        for p, _ in model.momentum_pairs():
            p.add_(torch.randn_like(p) * 1e-1)
    want = [pm.detach() * model.momentum + p.detach() * (1. - model.momentum) for p, pm in model.momentum_pairs()]
    with torch.no_grad():
        model._momentum_update()
    for (p, pm), w in zip(model.momentum_pairs(), want):
        assert torch.equal(pm.detach(), w)
    # the stale-cache half runs in f16x3, where the momentum towers' prepared weights are real copies (f16 split planes; in
    # fp32 the prepared weight of a 128-row-aligned Linear IS the parameter and nothing could go stale)
    images, _, _ = _fixture_inputs(g)
    fresh = _fixture_model(g)

    def ref_forward():
        fresh.load_state_dict(model.state_dict())
        return fresh.visual_encoder_m(images, space_dict=fresh.space_dict, temperature=0)[0]

    with runtime.precision("f16x3"), torch.no_grad():
        model.visual_encoder_m(images, space_dict=model.space_dict, temperature=0)  # prepares the current weights
        # the kernel alone (no update-epoch bump): the forward reads stale planes - shows this test can see a stale cache
        for p, _ in model.momentum_pairs():
            p.add_(torch.randn_like(p) * 1e-1)
        model._ema.update(model._ema_pairs, model.momentum)
        stale = model.visual_encoder_m(images, space_dict=model.space_dict, temperature=0)[0]
        assert not torch.equal(stale, ref_forward())
        # the model's update bumps the epoch of every momentum parameter: the prepared planes follow
        model._momentum_update()
        got = model.visual_encoder_m(images, space_dict=model.space_dict, temperature=0)[0]
        assert torch.equal(got, ref_forward())


def test_all_masked_row_raises_at_next_forward(hip):
    from madtp_amd import runtime
    g = np.load(CASES[0])
    model = _fixture_model(g)
    images, cap, _ = _fixture_inputs(g)
    same = torch.full((int(g["B"]),), 5, dtype=torch.long, device="cuda")
    with runtime.precision("fp32"), torch.no_grad():
        model(images, cap, 0.4, same, temperature=0)
        assert bool((model.last_negatives == -1).all())
        with pytest.raises(RuntimeError, match="no admissible hard negative"):
            model(images, cap, 0.4, same, temperature=0)
        model(images, cap, 0.4, torch.arange(int(g["B"]), device="cuda"), temperature=0)  # the flag was cleared


def test_train_mode_dropout_repeatable(hip):
    from madtp_amd import runtime
    g = np.load(CASES[0])
    model = _fixture_model(g)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    images, cap, idx = _fixture_inputs(g)
    model.train()
    vals = []
    for seed in (11, 11, 12):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        runtime.set_dropout_seed(seed)
        torch.manual_seed(0)
        with runtime.precision("fp32"):
            ls = model(images, cap, 0.4, idx, temperature=float(g["temperature"]))
            (ls[0] + ls[1] + 0.1 * ls[2] + 0.1 * ls[3]).backward()
        vals.append((float(ls[0].detach()), float(ls[1].detach())))
        assert all(np.isfinite(vals[-1]))
        assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    assert vals[0] == vals[1] and vals[0] != vals[2]


def test_adamw_steps_lower_the_loss(hip):
    from madtp_amd import harness, runtime, synth
    from madtp_amd.blip_retrieval import BLIP_Retrieval
    torch.manual_seed(0)
    B = 8
    model = BLIP_Retrieval(image_size=224, queue_size=64, evaluate=False)
    sd = synth.fill_state_dict(model, 3)
    for k in ("image_queue", "text_queue"):
        sd[k] = F.normalize(sd[k], dim=0)
    sd["temp"] = torch.tensor(0.07)
    model.load_state_dict(sd, strict=True)
    model.copy_params()
    model = model.cuda().eval()
    images = synth.synth_images(B, 224, 3).cuda()
    cap = {"input_ids": synth.synth_token_ids(B, 20, 3, first_id=101).cuda(), "attention_mask": harness.padded_mask(B, 20, 2).cuda()}
    idx = torch.arange(B, device="cuda")
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=2e-6, weight_decay=0.05)
    vals = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        model.itm_uniforms = torch.full((2, B), 0.5, device="cuda")
        with runtime.precision("fp32"):
            ls = model(images, cap, 0.4, idx, temperature=0)
            loss = ls[0] + ls[1]
            loss.backward()
        vals.append(float(loss.detach()))
        opt.step()
    # (the drawn negatives move with the features: the ITM term is noisy step to step)
    assert all(np.isfinite(vals)) and min(vals[1:]) < vals[0] and np.mean(vals[1:]) < vals[0], vals


FULL = r'''
import sys, torch
sys.path.insert(0, %r)
from madtp_amd import harness, runtime, synth
from madtp_amd.blip_retrieval import BLIP_Retrieval
B = 32
model = BLIP_Retrieval(image_size=384, queue_size=57600, evaluate=False).cuda().train()
images = synth.synth_images(B, 384, 0, device="cuda")
cap = {"input_ids": synth.synth_token_ids(B, 35, 0, first_id=101).cuda(), "attention_mask": harness.padded_mask(B, 35, 5).cuda()}
with runtime.precision("f16x3"), runtime.training_f16x3():
    ls = model(images, cap, 0.4, torch.arange(B, device="cuda"), temperature=1.0)
    (ls[0] + ls[1] + 0.1 * ls[2] + 0.1 * ls[3]).backward()
vals = [float(x.detach()) for x in ls]
assert all(v == v and abs(v) < 1e6 for v in vals), vals
assert int(model.ptr_queue[0]) == B
print("full-size step ok", vals)
'''


def test_full_size_training_step(hip):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", FULL % ROOT], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "full-size step ok" in r.stdout


def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _world_worker(rank, world, port, out_dir, path):
    os.environ.update(WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(4)
    sys.path.insert(0, ROOT)
    from madtp_amd import dist as mdist, hip as h, runtime
    from madtp_amd.backward import LinearFunction
    torch.cuda.set_device(0)
    w, r, _ = mdist.init("gloo")  # one GPU for both ranks: gloo moves host copies
    assert (w, r) == (world, rank)
    h.load()
    g = np.load(path)
    model = _fixture_model(g)
    model.negative_all_rank = True
    B = int(g["B"])
    images_all, cap_all, _ = _fixture_inputs(g)  # both ranks: B samples each, rank 1 the images in reverse order
    images = images_all if rank == 0 else images_all.flip(0).contiguous()
    cap = {k: (v if rank == 0 else v.flip(0).contiguous()) for k, v in cap_all.items()}
    idx = torch.arange(B, device="cuda") + 10 * rank
    temp0 = float(model.temp.detach())
    with runtime.precision("fp32"):
        ls = model(images, cap, 0.4, idx, temperature=0)  # step 1 with gradients (all_gather_with_grad's backward)
        (ls[0] + ls[1]).backward()
        assert model.last_negatives.shape == (2, B) and int(model.last_negatives.max()) < world * B
        ptr1 = int(model.ptr_queue[0])
        iq0, tq0, idq0 = model.image_queue.clone(), model.text_queue.clone(), model.idx_queue.clone()
        with torch.no_grad():
            ls = model(images, cap, 0.4, idx, temperature=0)  # step 2: its ITC inputs are restated below from this rank
            # this rank's features of step 2 (inference path, the same weights: the EMA ran inside step 2)
            vit = lambda enc: enc(images, space_dict=model.space_dict, temperature=0)[0][:, 0, :]  # noqa: E731
            ids = cap["input_ids"]
            txt = lambda enc: enc(ids, attention_mask=cap["attention_mask"], return_dict=True, mode="text",  # noqa: E731
                                  space_dict=model.space_dict, temperature=0)[0].last_hidden_state[:, 0, :]
            lin = lambda x, m: LinearFunction.apply(x.contiguous(), m.weight, m.bias, h.ACT_NONE)  # noqa: E731  (as forward())
            img_f = F.normalize(lin(vit(model.visual_encoder), model.vision_proj), dim=-1)
            txt_f = F.normalize(lin(txt(model.text_encoder), model.text_proj), dim=-1)
            img_m = F.normalize(model._linear("vp_m", model.vision_proj_m, vit(model.visual_encoder_m)), dim=-1)
            txt_m = F.normalize(model._linear("tp_m", model.text_proj_m, txt(model.text_encoder_m)), dim=-1)
    ref_i2t = _itc_ref(img_f.cpu(), img_m.cpu(), txt_m.cpu(), tq0.cpu(), idx.cpu(), idq0[0].cpu(), temp0, 0.4)[0].mean()
    ref_t2i = _itc_ref(txt_f.cpu(), txt_m.cpu(), img_m.cpu(), iq0.cpu(), idx.cpu(), idq0[0].cpu(), temp0, 0.4)[0].mean()
    unequal = ""
    try:
        model._check_equal_lengths(10 + rank)
    except RuntimeError as e:
        unequal = str(e)
    torch.save({"image_queue": model.image_queue.cpu(), "text_queue": model.text_queue.cpu(), "idx_queue": model.idx_queue.cpu(),
                "ptr": int(model.ptr_queue[0]), "ptr1": ptr1, "init_ptr": int(g["init_ptr"]), "img_m": img_m.cpu(), "txt_m": txt_m.cpu(),
                "idx": idx.cpu(), "loss_ita": float(ls[0].detach()), "ref_ita": float((ref_i2t + ref_t2i) / 2),
                "finite_grads": all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None),
                "unequal": unequal}, os.path.join(out_dir, f"r{rank}.pt"))
    mdist.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.timeout(900)
def test_world2_queues_losses_and_length_check(hip, tmp_path):
    """World 2 on one GPU (gloo), T = 0, negative_all_rank=True: the queues advance by world * B with both ranks' momentum
    features, each rank's loss_ita equals the float64 restatement, and unequal image-token lengths raise on every rank."""
    world = 2
    path = CASES[0]
    mp.spawn(_world_worker, args=(world, _free_port(), str(tmp_path), path), nprocs=world, join=True)
    res = [torch.load(os.path.join(str(tmp_path), f"r{r}.pt"), weights_only=False) for r in range(world)]
    B = res[0]["idx"].numel()
    for k in ("image_queue", "text_queue", "idx_queue"):
        assert torch.equal(res[0][k], res[1][k]), k
    n, Q = world * B, int(np.load(path)["queue_size"])
    p0 = res[0]["init_ptr"] // n * n  # the reference rounds the pointer down to the gathered batch
    assert res[0]["ptr1"] == res[1]["ptr1"] == (p0 + n) % Q        # step 1: world * B columns
    assert res[0]["ptr"] == res[1]["ptr"] == (p0 + 2 * n) % Q      # step 2
    cols = slice(res[0]["ptr1"], res[0]["ptr1"] + n)                # what step 2 enqueued
    assert _rel(res[0]["image_queue"][:, cols].t(), torch.cat([res[0]["img_m"], res[1]["img_m"]])) < 1e-5
    assert _rel(res[0]["text_queue"][:, cols].t(), torch.cat([res[0]["txt_m"], res[1]["txt_m"]])) < 1e-5
    assert torch.equal(res[0]["idx_queue"][0, cols], torch.cat([res[0]["idx"], res[1]["idx"]]))
    for r in res:
        assert abs(r["loss_ita"] - r["ref_ita"]) < 1e-5 * abs(r["ref_ita"]), (r["loss_ita"], r["ref_ita"])
        assert r["finite_grads"]
        assert "different lengths" in r["unequal"]
