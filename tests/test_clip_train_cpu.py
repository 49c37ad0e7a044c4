"""CLIP(evaluate=False) without a GPU: the reference's state-dict keys, copy_params, the queue pointer arithmetic of
_dequeue_and_enqueue (clip/model.py:598-618) on CPU tensors, and the host-side argument checks of the two embedding entry points."""
import glob
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "trainstep_clip_*.npz")))


def _tiny(evaluate, queue_size=8, layers=12):
    """the fixtures' layer counts at toy widths (one 64-wide head per tower): the key list depends on the layer counts only"""
    from madtp_amd.clip_model import CLIP
    torch.manual_seed(0)
    return CLIP(64, 32, layers, 64, 16, 77, 100, 64, 1, layers, evaluate, None, **({} if evaluate else {"queue_size": queue_size}))


def test_fixtures_present():
    assert [os.path.basename(c) for c in CASES] == ["trainstep_clip_b3_T4.npz", "trainstep_clip_b4_T0.npz"]


def test_state_dict_keys_equal_the_reference():
    from madtp_amd import specs
    train_keys = sorted(_tiny(False).state_dict().keys())
    for path in CASES:
        assert train_keys == np.load(path)["state_dict_keys"].tolist()
    eval_keys = sorted(_tiny(True).state_dict().keys())
    assert eval_keys == sorted(specs.clip_shapes(32, 16, 64, 12, 64, 64, 12, 77, 100).keys())  # the evaluation model is unchanged
    extra = sorted(set(train_keys) - set(eval_keys))
    assert set(eval_keys) <= set(train_keys)
    assert all(k.startswith(("visual_m.", "transformer_m.", "token_embedding_m.", "ln_final_m.")) or k in (
        "text_projection_m", "positional_embedding_m", "image_queue", "text_queue", "idx_queue", "ptr_queue") for k in extra), extra
    assert not any(hasattr(_tiny(True, layers=1), a) for a in ("visual_m", "image_queue", "momentum", "criterion"))


def test_training_state_matches_the_reference_constructor():
    m = _tiny(False, queue_size=8, layers=1)
    assert m.momentum == 0.995 and isinstance(m.criterion, torch.nn.CosineEmbeddingLoss) and m.queue_size == 8
    assert m.image_queue.shape == (64, 8) and m.text_queue.shape == (64, 8)
    assert torch.allclose(m.image_queue.norm(dim=0), torch.ones(8), atol=1e-6)
    assert torch.allclose(m.text_queue.norm(dim=0), torch.ones(8), atol=1e-6)
    assert m.idx_queue.shape == (1, 8) and m.idx_queue.dtype == torch.int64 and bool((m.idx_queue == -100).all())
    assert m.ptr_queue.dtype == torch.int64 and int(m.ptr_queue) == 0
    assert [len(p) for p in (m.model_pairs, m.params_pairs)] == [4, 2]
    from madtp_amd.clip_model import CLIP
    import inspect
    assert inspect.signature(CLIP.__init__).parameters["queue_size"].default == 57600


def test_copy_params_makes_every_pair_equal_and_frozen():
    m = _tiny(False, layers=2)
    pairs = m.momentum_pairs()
    n_student = sum(1 for mod, _ in m.model_pairs for _ in mod.parameters()) + 2
    assert len(pairs) == n_student
    with torch.no_grad():
        for p, _ in pairs:
            p.add_(torch.randn_like(p))
    assert not all(torch.equal(p, pm) for p, pm in pairs)
    m.copy_params()
    for p, pm in pairs:
        assert torch.equal(p, pm) and p.data_ptr() != pm.data_ptr()
        assert not pm.requires_grad and p.requires_grad
    assert any(pm is m.text_projection_m for _, pm in pairs) and any(pm is m.positional_embedding_m for _, pm in pairs)


def test_queue_pointer_wraps_and_rounds_down():
    m = _tiny(False, queue_size=8, layers=1)
    q0 = m.image_queue.clone()
    f = lambda v: torch.full((4, 64), float(v))  # noqa: E731
    m._dequeue_and_enqueue(f(1), f(2), torch.tensor([10, 11, 12, 13]))
    assert int(m.ptr_queue) == 4 and m.idx_queue[0].tolist() == [10, 11, 12, 13, -100, -100, -100, -100]
    assert bool((m.image_queue[:, :4] == 1).all()) and bool((m.text_queue[:, :4] == 2).all())
    assert torch.equal(m.image_queue[:, 4:], q0[:, 4:])
    m._dequeue_and_enqueue(f(3), f(4), torch.tensor([20, 21, 22, 23]))
    assert int(m.ptr_queue) == 0  # wrap-around: (4 + 4) % 8
    assert m.idx_queue[0].tolist() == [10, 11, 12, 13, 20, 21, 22, 23]
    m.ptr_queue.fill_(5)  # an unaligned pointer (a checkpoint written at another batch size): rounded down to 4 (:609-610)
    m._dequeue_and_enqueue(f(5), f(6), torch.tensor([30, 31, 32, 33]))
    assert m.idx_queue[0].tolist() == [10, 11, 12, 13, 30, 31, 32, 33] and int(m.ptr_queue) == 0
    assert bool((m.image_queue[:, 4:] == 5).all()) and bool((m.image_queue[:, :4] == 1).all())
    with pytest.raises(AssertionError):  # queue_size % batch != 0 (:607)
        m._dequeue_and_enqueue(torch.zeros(3, 64), torch.zeros(3, 64), torch.tensor([1, 2, 3]))
    m.reset_queue()
    assert int(m.ptr_queue) == 0 and bool((m.idx_queue == -100).all()) and m.image_queue.shape == (64, 8)
    assert torch.allclose(m.image_queue.norm(dim=0), torch.ones(8), atol=1e-6)


def test_evaluation_model_has_no_forward():
    with pytest.raises(NotImplementedError, match="evaluate=False"):
        _tiny(True, layers=1)(None, None, 0.4, None)


def test_embedding_entry_points_exported_and_validate_on_the_host():
    from madtp_amd import build, hip
    build.build(verbose=False)
    lib = hip.load()
    for name in ("madtp_clip_embed", "madtp_embedding_grad", "madtp_embedding_grad_workspace"):
        assert name in hip.exported_symbols() and hasattr(lib, name)
    assert callable(hip.clip_embed) and callable(hip.embedding_grad)
    assert lib.madtp_clip_embed(0, 16, 16, 16, 2, 77, 512, 100, None) == -1        # null pointer
    assert lib.madtp_clip_embed(16, 16, 16, 16, 2, 77, 512, 0, None) == -1         # empty table
    assert lib.madtp_clip_embed(16, 16, 16, 16, 2, 77, 510, 100, None) == -2       # D % 4
    assert int(lib.madtp_embedding_grad_workspace(10)) == 120
    assert int(lib.madtp_embedding_grad_workspace(0)) == 0 and int(lib.madtp_embedding_grad_workspace(256 * 77 + 1)) == 0
    assert int(lib.madtp_embedding_grad_workspace(256 * 77)) == 256 * 77 * 12
    assert lib.madtp_embedding_grad(16, 16, 0, 16, 1 << 20, 10, 512, 100, None) == -1          # null pointer
    assert lib.madtp_embedding_grad(16, 16, 16, 16, 1 << 20, 10, 96, 100, None) == -2          # D % 64
    assert lib.madtp_embedding_grad(16, 16, 16, 16, 1 << 20, 10, 1088, 100, None) == -2        # D > 1024
    assert lib.madtp_embedding_grad(16, 16, 16, 16, 1 << 30, 256 * 77 + 1, 512, 100, None) == -2   # n past the range
    assert lib.madtp_embedding_grad(16, 16, 16, 16, 119, 10, 512, 100, None) == -1             # workspace too small
