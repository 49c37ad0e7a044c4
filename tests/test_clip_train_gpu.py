"""CLIP's training step on a real MI355X (CLIP(evaluate=False).forward, csrc/clip.hip):
  * madtp_clip_embed bit-equal to torch indexing, madtp_embedding_grad against a float64 index_add_ within the sequential-f32-sum
    bound, with exact zeros for absent rows, bit-identical repeats and no dependence on the output's prior contents,
  * one training step against the reference's own (tests/golden/trainstep_clip_*.npz, tools/make_golden.py::clip_train_case):
    losses, every gradient, momentum parameters, queues, pointer, per-layer lengths, and the losses of a second step,
  * run-to-run identical token-embedding gradients, a few AdamW steps, the evaluation model's forward raising.
Multi-rank behaviour (the gathered queue update) reuses blip_retrieval._all_gather, which tests/test_retrieval_train_gpu.py covers
at world 2; it is not repeated here."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "trainstep_clip_*.npz")))
TRAIN_MODES = ["fp32", "f16x3"]
SIZE = 96  # ViT-B/16 at 96^2: 37 tokens


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


# ---- the embedding kernels --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,L,D", [(3, 77, 512), (1, 5, 64)])
def test_clip_embed_bit_equal_to_torch_indexing(hip, B, L, D):
    g = torch.Generator().manual_seed(B * 1000 + L)
    V = 97
    table, pos = torch.randn(V, D, generator=g).cuda(), torch.randn(77, D, generator=g).cuda()
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[0, 0], ids[-1, -1] = V - 1, 0
    ids = ids.cuda()
    got = hip.clip_embed(ids, table, pos)
    assert got.shape == (B, L, D) and torch.equal(got, table[ids] + pos[:L])  # one add per element


def _caption_ids(B, L, V, seed):
    """CLIP-shaped rows: id V-1 first, a few words, zero padding from about position 17 on (about 60 of 77 ids are 0)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        n = min(14 + 2 * b, L - 1)
        ids[b, 0] = V - 1
        ids[b, 1:1 + n] = torch.randint(2, V - 2, (n,), generator=g)  # non-monotonic, with repeats
    return ids


def _grad_check(hip, ids, dx, V):
    """-> dtable; asserts the float64 bound, exact zeros, repeatability and independence of the output's prior contents"""
    n, D = dx.shape
    got = hip.embedding_grad(ids, dx, V)
    flat = ids.view(-1)
    ref = torch.zeros(V, D, dtype=torch.float64, device="cuda").index_add_(0, flat, dx.double())
    mag = torch.zeros(V, D, dtype=torch.float64, device="cuda").index_add_(0, flat, dx.double().abs())
    count = torch.bincount(flat, minlength=V).double().view(V, 1)
    # the error of a sequential f32 sum of c terms: at most c * 2^-24 * sum |terms| (c - 1 roundings of relative size 2^-24 each)
    bound = count * 2.0 ** -24 * mag
    err = (got.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"embedding_grad n={n} D={D} V={V}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, "
          f"max count {int(count.max())}")
    assert worst <= 0.0, worst
    absent = count.view(-1) == 0
    assert bool((got[absent] == 0).all())  # (bound 0 there: also implied above; NaN-free)
    assert torch.equal(got, hip.embedding_grad(ids, dx, V))
    out = torch.full((V, D), float("nan"), device="cuda")
    assert hip.embedding_grad(ids, dx, V, out=out) is out and torch.equal(out, got)
    return got, count.view(-1)


def test_embedding_grad_caption_rows(hip):
    V, D, B, L = 97, 512, 3, 77
    ids = _caption_ids(B, L, V, 0)
    ids[1, 5] = 1          # id 1 occurs exactly once
    assert int((ids == 1).sum()) == 1 and int((ids == 0).sum()) > 64 * 2 and int((ids == V - 1).sum()) == B
    assert bool((ids[:, 1:16].diff(dim=1) < 0).any())
    dx = torch.randn(B * L, D, generator=torch.Generator().manual_seed(1)).cuda()
    got, count = _grad_check(hip, ids.cuda(), dx, V)
    assert int(count[0]) > 64 and int(count[1]) == 1 and int(count[V - 1]) == B and int((count == 0).sum()) > 0
    assert torch.equal(got[1], dx[1 * L + 5])  # a single occurrence is copied
    # ascending flat position: the long segment equals the explicit left-to-right f32 sum
    seq = torch.zeros(D, device="cuda")
    for i in torch.nonzero(ids.view(-1) == 0).view(-1).tolist():
        seq = seq + dx[i]
    assert torch.equal(got[0], seq)


def test_embedding_grad_single_position(hip):
    dx = torch.randn(1, 64, generator=torch.Generator().manual_seed(2)).cuda()
    got, _ = _grad_check(hip, torch.tensor([[96]]).cuda(), dx, 97)
    assert torch.equal(got[96], dx[0]) and int((got != 0).any(dim=1).sum()) == 1


def test_embedding_grad_range_limit(hip):
    """n = 256 * 77 positions on CLIP's table (49408 x 512): the largest supported call"""
    V, D, B, L = 49408, 512, 256, 77
    g = torch.Generator().manual_seed(3)
    ids = torch.zeros(B, L, dtype=torch.int64)
    ids[:, 0] = 49406
    ids[:, 1:16] = torch.randint(1000, 40000, (B, 15), generator=g)
    ids[:, 16] = V - 1
    dx = torch.randn(B * L, D, generator=g).cuda()
    _grad_check(hip, ids.cuda(), dx, V)
    with pytest.raises(RuntimeError, match="madtp_embedding_grad"):
        hip.embedding_grad(torch.zeros(B * L + 1, dtype=torch.int64).cuda(), torch.zeros(B * L + 1, D).cuda(), V)


def test_clip_text_embed_function_gradients(hip):
    from madtp_amd.backward import ClipTextEmbedFunction
    g = torch.Generator().manual_seed(4)
    V, D, B, L = 97, 64, 2, 9
    table = torch.randn(V, D, generator=g).cuda().requires_grad_(True)
    pos = torch.randn(12, D, generator=g).cuda().requires_grad_(True)  # more rows than L: the tail's gradient is zero
    ids = _caption_ids(B, L, V, 5).cuda()
    w = torch.randn(B, L, D, generator=g).cuda()
    (ClipTextEmbedFunction.apply(ids, table, pos) * w).sum().backward()
    t2, p2 = table.detach().clone().requires_grad_(True), pos.detach().clone().requires_grad_(True)
    ((t2[ids] + p2[:L]) * w).sum().backward()
    assert _rel(table.grad, t2.grad) < 1e-6 and _rel(pos.grad, p2.grad) < 1e-6
    assert bool((pos.grad[L:] == 0).all())


# ---- the training step -------------------------------------------------------------------------------------------------------

_MODEL = {}


def _model(queue_size):
    """one CLIP(evaluate=False) per queue size for the module (ViT-B/16 at 96^2, the 12-layer text tower); _reset reloads it"""
    from madtp_amd.clip_model import CLIP
    if queue_size not in _MODEL:
        torch.manual_seed(0)
        _MODEL[queue_size] = CLIP(512, SIZE, 12, 768, 16, 77, 49408, 512, 8, 12, False, None, queue_size=queue_size).cuda().eval()
    return _MODEL[queue_size]


def _reset(model, seed, queues):
    from madtp_amd import specs
    sd = specs.synth_weights(specs.clip_shapes(SIZE), seed, device="cuda")
    sd["logit_scale"] = torch.tensor(2.6592600369327779, device="cuda")
    sd.update(queues)
    msg = model.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys and all(k.endswith("_m") or "_m." in k for k in msg.missing_keys)
    model.copy_params()
    model.zero_grad(set_to_none=True)
    return model


def _fixture_model(g):
    model = _model(int(g["queue_size"]))
    queues = {"image_queue": torch.from_numpy(g["init_image_queue"]).cuda(), "text_queue": torch.from_numpy(g["init_text_queue"]).cuda(),
              "idx_queue": torch.from_numpy(g["init_idx_queue"]).cuda(), "ptr_queue": torch.tensor([int(g["init_ptr"])]).cuda()}
    _reset(model, int(g["seed"]), queues)
    text = torch.from_numpy(g["text"])
    model.tokenize = lambda caption: text  # the driver sets clip.tokenize here; the fixture's token rows stand in for it
    return model


def _fixture_inputs(g):
    from madtp_amd import synth
    B = int(g["B"])
    return synth.synth_images(B, SIZE, int(g["seed"])).cuda(), ["caption"] * B, torch.from_numpy(g["idx"]).cuda()


class _Lens:
    """output length of every block call, as the recording's forward hooks"""

    def __init__(self, model):
        self.lens = {"vit": [], "txt": [], "vit_m": []}
        self.hooks = [blk.register_forward_hook(lambda m, a, o, t=t: self.lens[t].append(o[0].shape[0]))
                      for t, blocks in (("vit", model.visual.transformer.resblocks), ("txt", model.transformer.resblocks),
                                        ("vit_m", model.visual_m.transformer.resblocks)) for blk in blocks]

    def remove(self):
        for h in self.hooks:
            h.remove()


def _check_losses(losses, ref, what):
    l = [float(x.detach()) for x in losses]
    print(what, "losses", l, "reference", [float(r) for r in ref])
    assert abs(l[0] - ref[0]) < 1e-3 * abs(ref[0]), (what, "loss_ita", l[0], ref[0])
    assert abs(l[1] - ref[1]) < 1e-4 * max(1.0, abs(ref[1])), (what, "loss_fdt", l[1], ref[1])
    assert abs(l[2] - ref[2]) < 1e-4 * max(1.0, abs(ref[2])), (what, "loss_fdt_m", l[2], ref[2])


@pytest.mark.parametrize("mode", TRAIN_MODES)
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(c)[:-4] for c in CASES])
def test_clip_training_step_matches_reference(hip, path, mode):
    from tests import grad_case
    g = np.load(path)
    model = _fixture_model(g)
    images, cap, idx = _fixture_inputs(g)
    alpha, T, B = float(g["alpha"]), float(g["temperature"]), int(g["B"])
    rec = _Lens(model)
    try:
        with _train_mode(mode):
            losses = model(images, cap, alpha, idx, temperature=T)
            _check_losses(losses, g["losses"], mode)
            if T == 0:
                assert losses[1] is losses[0] and losses[2] is losses[0]  # (its gradient counts 1.2 x, as in the reference)
            (losses[0] + 0.1 * losses[1] + 0.1 * losses[2]).backward()
    finally:
        rec.remove()
    # per-layer lengths: student vision, momentum vision, and both calls of the student text blocks
    print("lens", rec.lens)
    assert rec.lens["vit"] == g["vit_lens"].tolist() and rec.lens["vit_m"] == g["vit_m_lens"].tolist()
    assert rec.lens["txt"] == g["txt_lens"].tolist() + g["txt_m_lens"].tolist()
    grads = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    missing = [k[2:-7] for k in g.files if k.startswith("g_") and k.endswith("_sample") and k[2:-7] not in grads]
    assert not missing, missing[:5]
    assert "token_embedding.weight" in grads and "logit_scale" in grads and "text_projection" in grads
    grad_case.check_against_fixture(g, grads, 1e-3, f"HIP CLIP training step ({mode}) vs reference")
    # momentum parameters after the EMA: bit-exact (same f32 inputs, same three roundings)
    params = dict(model.named_parameters())
    n_m = 0
    for k in g.files:
        if k.startswith("m_"):
            flat = params[k[2:]].detach().reshape(-1).cpu()
            got = flat[torch.from_numpy(grad_case.grad_sample_index(flat.numel(), 16, stride=104729))].numpy()
            assert np.array_equal(got, g[k]), k
            n_m += 1
    assert n_m == len(model.momentum_pairs())
    # queues: the student features in the B columns at the rounded-down pointer, everything else untouched
    p0, Q = int(g["enq_at"]), int(g["queue_size"])
    rest = np.ones(Q, dtype=bool)
    rest[p0:p0 + B] = False
    for k in ("image_queue", "text_queue"):
        after = getattr(model, k).cpu()
        assert _rel(after[:, p0:p0 + B], torch.from_numpy(g[f"enq_{k}"])) < 1e-4, k
        assert np.array_equal(after.numpy()[:, rest], g[f"init_{k}"][:, rest]), k
    assert np.array_equal(model.idx_queue.cpu().numpy(), g["idx_queue"]) and int(model.ptr_queue[0]) == int(g["ptr"])
    torch.optim.SGD([p for p in model.parameters() if p.grad is not None], lr=float(g["lr"])).step()
    with _train_mode(mode), torch.no_grad():
        losses2 = model(images, cap, alpha, idx, temperature=T)
    _check_losses(losses2, g["losses2"], mode + " second step")


def test_two_identical_steps_give_identical_embedding_gradients(hip):
    g = np.load(CASES[0])
    images, cap, idx = _fixture_inputs(g)
    got = []
    for _ in range(2):
        model = _fixture_model(g)
        with _train_mode("fp32"):
            ls = model(images, cap, float(g["alpha"]), idx, temperature=float(g["temperature"]))
            (ls[0] + 0.1 * ls[1] + 0.1 * ls[2]).backward()
        got.append((model.token_embedding.weight.grad.clone(), model.positional_embedding.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    used = torch.from_numpy(g["text"]).unique().cuda()
    rows = torch.zeros(49408, dtype=torch.bool, device="cuda")
    rows[used] = True
    assert bool((got[0][0][~rows] == 0).all()) and bool((got[0][0][rows] != 0).any(dim=1).all())


def test_adamw_steps_lower_the_loss(hip):
    """Five AdamW steps on one batch.  The queue is put back before every step: the reference enqueues the STUDENT features, so a
    repeated batch would meet its own earlier features as extra positives and the loss would follow the targets' entropy instead of
    the parameters."""
    import torch.nn.functional as F
    from madtp_amd import synth
    B, Q = 8, 96
    model = _model(Q)
    gq = torch.Generator().manual_seed(7)
    queues = {"image_queue": F.normalize(torch.randn(512, Q, generator=gq), dim=0).cuda(),
              "text_queue": F.normalize(torch.randn(512, Q, generator=gq), dim=0).cuda(),
              "idx_queue": torch.full((1, Q), -100).cuda(), "ptr_queue": torch.zeros(1, dtype=torch.long).cuda()}
    _reset(model, 3, queues)
    images = synth.synth_images(B, SIZE, 3).cuda()
    text = synth.synth_clip_tokens(B, 77, 3).cuda()
    idx = torch.arange(B, device="cuda")
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=2e-6, weight_decay=0.05)
    vals = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            for k, v in queues.items():
                getattr(model, k).copy_(v)
        with _train_mode("fp32"):
            ls = model(images, text, 0.4, idx, temperature=0)
            ls[0].backward()
        vals.append(float(ls[0].detach()))
        opt.step()
    print("AdamW losses", vals)
    assert all(np.isfinite(vals)) and min(vals[1:]) < vals[0] and np.mean(vals[1:]) < vals[0], vals


def test_evaluation_model_forward_raises(hip):
    from madtp_amd.clip_model import CLIP
    model = CLIP(64, 32, 1, 64, 16, 77, 100, 64, 1, 1, True, None).cuda()
    with pytest.raises(NotImplementedError, match="evaluate=False"):
        model(torch.zeros(1, 3, 32, 32).cuda(), torch.zeros(1, 77, dtype=torch.int64).cuda(), 0.4, torch.zeros(1, dtype=torch.int64).cuda())
