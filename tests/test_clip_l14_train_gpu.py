"""CLIP's training step at the ViT-L/14 widths on a real MI355X: vision width 1024 / 16 heads, text width 768 / 12 heads,
embed_dim 768 (madtp_itc_loss on its wide kernel), patch 14 - against the reference's own step
(tests/golden/trainstep_clipl14_b3_T4.npz, tools/make_golden.py::clip_train_case; 4 layers per tower at 112^2, 65 tokens),
with the helpers and bounds of tests/test_clip_train_gpu.py::test_clip_training_step_matches_reference."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trainstep_clipl14_b3_T4.npz")
TRAIN_MODES = ["fp32", "f16x3"]
SIZE, PATCH, VW, VL, ED, TW, TL = 112, 14, 1024, 4, 768, 768, 4

_MODEL = {}


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


def _fixture_model(g):
    from madtp_amd import specs
    from madtp_amd.clip_model import CLIP
    Q = int(g["queue_size"])
    if Q not in _MODEL:
        torch.manual_seed(0)
        _MODEL[Q] = CLIP(ED, SIZE, VL, VW, PATCH, 77, 49408, TW, TW // 64, TL, False, None, queue_size=Q).cuda().eval()
    model = _MODEL[Q]
    sd = specs.synth_weights(specs.clip_shapes(SIZE, PATCH, VW, VL, ED, TW, TL), int(g["seed"]), device="cuda")
    sd["logit_scale"] = torch.tensor(float(g["init_logit_scale"]), dtype=torch.float32, device="cuda")
    sd.update({"image_queue": torch.from_numpy(g["init_image_queue"]).cuda(), "text_queue": torch.from_numpy(g["init_text_queue"]).cuda(),
               "idx_queue": torch.from_numpy(g["init_idx_queue"]).cuda(), "ptr_queue": torch.tensor([int(g["init_ptr"])]).cuda()})
    msg = model.load_state_dict(sd, strict=False)
    assert not msg.unexpected_keys and all(k.endswith("_m") or "_m." in k for k in msg.missing_keys)
    model.copy_params()
    model.zero_grad(set_to_none=True)
    text = torch.from_numpy(g["text"])
    model.tokenize = lambda caption: text  # the driver sets clip.tokenize here; the fixture's token rows stand in for it
    return model


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
def test_clip_l14_training_step_matches_reference(hip, mode):
    from madtp_amd import synth
    from tests import grad_case
    g = np.load(FIXTURE)
    model = _fixture_model(g)
    assert model.embed_dim == 768 and model.text_queue.shape == (768, int(g["queue_size"]))
    alpha, T, B = float(g["alpha"]), float(g["temperature"]), int(g["B"])
    images, cap, idx = synth.synth_images(B, SIZE, int(g["seed"])).cuda(), ["caption"] * B, torch.from_numpy(g["idx"]).cuda()
    rec = _Lens(model)
    try:
        with _train_mode(mode):
            losses = model(images, cap, alpha, idx, temperature=T)
            _check_losses(losses, g["losses"], mode)
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
    grad_case.check_against_fixture(g, grads, 1e-3, f"HIP CLIP L/14-width training step ({mode}) vs reference")
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


def test_l14_state_raises_nothing_at_build():
    """build_model on a state dict with the ViT-L/14@336 key shapes (one layer per tower), evaluate=False"""
    from madtp_amd import clip_model, specs
    sd = {k: torch.zeros(shp[1:] if shp and shp[0] == "int64" else shp) for k, shp in
          specs.clip_shapes(336, 14, 1024, 1, 768, 768, 1).items()}
    model = clip_model.build_model(sd, evaluate=False)
    assert model.embed_dim == 768 and not model.evaluate
    assert model.image_queue.shape == (768, model.queue_size) and model.text_queue.shape == (768, model.queue_size)
    assert model.visual.conv1.weight.shape == (1024, 3, 14, 14) and model.text_projection.shape == (768, 768)
