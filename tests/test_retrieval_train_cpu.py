"""CPU checks of the retrieval training step (BLIP_Retrieval(evaluate=False), csrc/retrieval.hip): the training state mirrors
the reference's by key and momentum pairing, the evaluation model is unchanged, and the new C-ABI entry points reject bad
arguments on the host before any launch."""
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "trainstep_retr_*.npz")))


def _named(model):
    names = {}
    for n, p in model.named_parameters(remove_duplicate=False):
        names.setdefault(id(p), n)
    return names


@pytest.fixture(scope="module")
def train_model():
    from madtp_amd.blip_retrieval import BLIP_Retrieval
    g = np.load(CASES[0])
    return BLIP_Retrieval(image_size=int(g["size"]), queue_size=int(g["queue_size"]), evaluate=False), g


def test_fixtures_present():
    assert len(CASES) == 2


def test_training_state_dict_keys_match_reference(train_model):
    model, g = train_model
    assert list(sorted(model.state_dict().keys())) == sorted(g["state_dict_keys"].tolist())
    assert model.image_queue.shape == (256, int(g["queue_size"])) and model.idx_queue.shape == (1, int(g["queue_size"]))
    assert bool((model.idx_queue == -100).all()) and int(model.ptr_queue[0]) == 0
    assert abs(float(model.temp.detach()) - 0.07) < 1e-7 and model.temp.shape == ()
    # unit-norm queue columns (:88-89)
    assert np.allclose(model.image_queue.norm(dim=0).numpy(), 1.0, atol=1e-5)


def test_momentum_pairing_matches_reference(train_model):
    model, g = train_model
    names = _named(model)
    mine = {f"{names[id(p)]}|{names[id(pm)]}" for p, pm in model.momentum_pairs()}
    assert mine == set(g["pairing"].tolist())
    for p, pm in model.momentum_pairs():
        assert not pm.requires_grad and bool((p.detach() == pm.detach()).all())  # copy_params (:285-291)


def test_evaluation_model_unchanged():
    import torch
    from madtp_amd.blip_retrieval import BLIP_Retrieval
    model = BLIP_Retrieval(image_size=96, queue_size=12, evaluate=True)
    keys = set(model.state_dict().keys())
    assert not any(k.endswith("_m") or "_m." in k for k in keys)
    assert not {"temp", "image_queue", "text_queue", "idx_queue", "ptr_queue"} & keys
    with pytest.raises(NotImplementedError):
        model(torch.zeros(1, 3, 96, 96), {"input_ids": torch.zeros(1, 4, dtype=torch.long),
                                          "attention_mask": torch.ones(1, 4, dtype=torch.long)}, 0.4, torch.zeros(1))


def test_training_forward_needs_fp32_mode(train_model):
    import torch
    from madtp_amd import runtime
    model, _ = train_model
    with runtime.precision("bf16"):
        with pytest.raises(NotImplementedError):
            model(torch.zeros(1, 3, 96, 96), {}, 0.4, torch.zeros(1))


def test_new_symbols_validate_arguments_without_gpu():
    from madtp_amd import build, hip
    build.build(verbose=False)
    lib = hip.load()
    assert lib.madtp_abi_version() == 31
    assert lib.madtp_itc_loss(0, 0, 0, 0, 0, 0, 0, 0.4, 0, 0, 0, 0, 0, 4, 256, 12, None) == -1     # null pointers
    ws = int(lib.madtp_itc_workspace(4, 96, 12))
    assert ws > 0
    assert lib.madtp_itc_loss(16, 16, 16, 16, 16, 16, 16, 0.4, 16, 16, 16, 16, ws, 4, 96, 12, None) == -2   # D % 64
    assert lib.madtp_itc_loss(16, 16, 16, 16, 16, 16, 16, 0.4, 16, 16, 16, 16, 1 << 30, 257, 256, 12, None) == -2  # B > 256
    assert lib.madtp_itc_loss(16, 16, 16, 16, 16, 16, 16, 0.4, 16, 16, 16, 16, 1, 4, 256, 12, None) == -1  # workspace too small
    assert lib.madtp_ema_update(0, 3, 3, 0.995, 0.005, None) == -1
    assert lib.madtp_ema_update(16, 0, 3, 0.995, 0.005, None) == -1
    assert lib.madtp_itm_negatives(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 256, None) == -1
    assert lib.madtp_itm_negatives(*([16] * 10), 4, 4, 100, None) == -2                          # D % 64
    assert lib.madtp_itm_negatives(*([16] * 10), 4, 2, 256, None) == -2                          # fewer columns than rows
