"""madtp_itc_loss for 512 < D <= 1024 without a GPU: the host-side range and workspace checks (nothing launches), and the
ViT-L/14-width training fixture (tests/golden/trainstep_clipl14_b3_T4.npz, tools/make_golden.py::clip_train_case)."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trainstep_clipl14_b3_T4.npz")


@pytest.fixture(scope="module")
def lib():
    from madtp_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def _itc(lib, ws_bytes, B, D, Q):
    """non-null dummy pointers: only for arguments that are refused before anything launches"""
    return lib.madtp_itc_loss(16, 16, 16, 16, 16, 16, 16, 0.4, 16, 16, 16, 16, ws_bytes, B, D, Q, None)


def test_wide_workspace_is_sized(lib):
    assert int(lib.madtp_itc_workspace(16, 768, 57600)) > 0
    assert int(lib.madtp_itc_workspace(32, 1024, 57600)) > int(lib.madtp_itc_workspace(32, 768, 57600))


def test_wide_dims_pass_the_shape_check(lib):
    assert _itc(lib, 1, 4, 768, 12) == -1     # the shape is accepted; the workspace is too small
    assert _itc(lib, 1, 4, 576, 12) == -1
    assert _itc(lib, 1, 4, 1024, 12) == -1


def test_dims_out_of_range_are_refused(lib):
    assert _itc(lib, 1 << 30, 4, 1088, 12) == -2   # D > 1024
    assert _itc(lib, 1 << 30, 4, 800, 12) == -2    # D % 64
    assert _itc(lib, 1 << 30, 257, 768, 12) == -2  # B > 256


def test_l14_fixture_present_with_the_training_keys():
    from madtp_amd.clip_model import CLIP
    g = np.load(FIXTURE)
    assert g["init_image_queue"].shape == (768, int(g["queue_size"])) and g["init_text_queue"].shape == (768, int(g["queue_size"]))
    assert len(g["vit_lens"]) == 4 and len(g["txt_lens"]) == 4 and len(g["txt_m_lens"]) == 4
    assert g["vit_lens"][-1] < g["vit_lens"][0] <= 65 and g["txt_lens"][-1] < g["txt_lens"][0]  # both towers prune
    # the key list depends on the layer counts only: toy widths, one 64-wide head per tower
    torch.manual_seed(0)
    tiny = CLIP(64, 28, 4, 64, 14, 77, 100, 64, 1, 4, False, None, queue_size=8)
    assert sorted(tiny.state_dict().keys()) == g["state_dict_keys"].tolist()
    torch.manual_seed(0)
    m = CLIP(768, 28, 1, 64, 14, 77, 100, 64, 1, 1, False, None, queue_size=int(g["queue_size"]))
    assert m.embed_dim == 768 and m.image_queue.shape == g["init_image_queue"].shape
