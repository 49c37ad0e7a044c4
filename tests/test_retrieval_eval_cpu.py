"""Retrieval evaluation without a GPU: the host-side argument checks of madtp_rank_embeds / madtp_rank_scores, target_lists,
recall_metrics against the restated itm_eval, and the refusal of CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_ref  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from madtp_amd import build, hip
    build.build(verbose=False)
    return hip.load()


def test_entry_points_are_bound_and_the_abi_version_is_unchanged(lib):
    from madtp_amd import hip
    for name in ("madtp_rank_workspace", "madtp_rank_embeds", "madtp_rank_scores"):
        assert name in hip.exported_symbols() and hasattr(lib, name)
    assert hip.ABI_VERSION == 31 and lib.madtp_abi_version() == 31


def test_rank_embeds_validates_on_the_host(lib):
    P = 4096  # never dereferenced: every call below is rejected before a launch

    def call(q=P, ldq=512, keys=P, ldk=512, nq=4, nk=9, D=512, ptr=P, idx=P, rr=P, rt=P, sc=P, ws=P, ws_bytes=1 << 20):
        return lib.madtp_rank_embeds(q, ldq, keys, ldk, nq, nk, D, ptr, idx, rr, rt, sc, ws, ws_bytes, None)

    for null in ("q", "keys", "ptr", "idx", "rr", "rt", "sc", "ws"):
        assert call(**{null: 0}) == -1, null                       # MADTP_E_BADARG
    for shape in (dict(D=40, ldq=40, ldk=40), dict(D=1088, ldq=1088, ldk=1088), dict(nq=0), dict(nk=0), dict(D=0),
                  dict(ldq=448), dict(ldk=256)):
        assert call(**shape) == -2, shape                          # MADTP_E_SHAPE
    assert call(ldq=514) == -4 and call(q=P + 4) == -4             # MADTP_E_ALIGN: 16-byte loads of the rows
    assert call(ws_bytes=0) == -1


def test_rank_scores_validates_on_the_host(lib):
    P = 4096
    assert lib.madtp_rank_scores(0, 9, 4, 9, P, P, P, P, None) == -1
    assert lib.madtp_rank_scores(P, 9, 4, 9, P, 0, P, P, None) == -1
    assert lib.madtp_rank_scores(P, 9, 0, 9, P, P, P, P, None) == -2
    assert lib.madtp_rank_scores(P, 8, 4, 9, P, P, P, P, None) == -2   # ld < nk


def test_rank_workspace_grows_with_the_targets(lib):
    small, large = int(lib.madtp_rank_workspace(5000, 25010, 512, 5000)), int(lib.madtp_rank_workspace(5000, 25010, 512, 25010))
    assert 0 < small < large
    assert int(lib.madtp_rank_workspace(1, 1, 64, 1)) > 0
    assert int(lib.madtp_rank_workspace(0, 5, 64, 1)) == 0


def test_target_lists_forms_and_errors():
    from madtp_amd import retrieval_eval as re
    img2txt = [[0, 1], [2], [3, 4, 5]]
    txt2img = [0, 0, 1, 2, 2, 2]
    t = re.target_lists(txt2img, img2txt, 3, 6)
    assert all(x.dtype == torch.int32 and not x.is_cuda for x in t)
    assert t.i2t_ptr.tolist() == [0, 2, 3, 6] and t.i2t_idx.tolist() == [0, 1, 2, 3, 4, 5]
    assert t.t2i_ptr.tolist() == list(range(7)) and t.t2i_idx.tolist() == txt2img
    for other in (re.target_lists(dict(enumerate(txt2img)), dict(enumerate(img2txt)), 3, 6),
                  re.target_lists(np.array(txt2img), [np.array(x) for x in img2txt], 3, 6),
                  re.target_lists([[i] for i in txt2img], [tuple(x) for x in img2txt], 3, 6)):
        assert all(torch.equal(a, b) for a, b in zip(t, other))
    ptr, idx = rank_ref.csr(img2txt)
    assert t.i2t_ptr.tolist() == ptr.tolist() and t.i2t_idx.tolist() == idx.tolist()
    with pytest.raises(ValueError, match="outside"):
        re.target_lists(txt2img, [[0, 1], [2], [3, 4, 6]], 3, 6)
    with pytest.raises(ValueError, match="outside"):
        re.target_lists([0, 0, 1, 2, 2, -1], img2txt, 3, 6)
    with pytest.raises(ValueError, match="17 targets"):
        re.target_lists([0] * 17, [list(range(17))], 1, 17)
    assert re.target_lists([0] * 16, [list(range(16))], 1, 16).i2t_ptr.tolist() == [0, 16]
    with pytest.raises(ValueError, match="rows"):
        re.target_lists(txt2img[:5], img2txt, 3, 6)
    with pytest.raises(ValueError, match="no entry"):
        re.target_lists({0: 0}, img2txt, 3, 6)


def test_recall_metrics_equal_the_restated_itm_eval():
    from madtp_amd import retrieval_eval as re
    img, txt = rank_ref.realistic_features(40, 5, 64)
    s = (img.double() @ txt.double().t()).numpy()
    txt2img, img2txt = rank_ref.pairing(40, 5)
    want = rank_ref.itm_eval(s, s.T, txt2img, img2txt)
    ri, _ = rank_ref.ranks(s, img2txt)
    rt, _ = rank_ref.ranks(s.T, [[t] for t in txt2img])
    got = re.recall_metrics(torch.from_numpy(ri), rt)
    assert list(got) == ["txt_r1", "txt_r5", "txt_r10", "txt_r_mean", "img_r1", "img_r5", "img_r10", "img_r_mean", "r_mean"]
    assert got == want
    assert 0 < got["txt_r1"] < got["txt_r10"] <= 100 and 0 < got["img_r1"] < got["img_r10"] <= 100
    assert got["txt_r_mean"] == (got["txt_r1"] + got["txt_r5"] + got["txt_r10"]) / 3
    assert got["r_mean"] == (got["txt_r_mean"] + got["img_r_mean"]) / 2
    assert re.recall_metrics([0, 4, 5, 9, 10], [0])["txt_r5"] == 40.0


def test_cpu_tensors_are_refused(lib):
    from madtp_amd import retrieval_eval as re
    q, k = torch.zeros(2, 64), torch.zeros(3, 64)
    ptr, idx = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        re.rank_embeds(q, k, ptr, idx)
    with pytest.raises(RuntimeError, match="GPU"):
        re.rank_scores(torch.zeros(2, 3), ptr, idx)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recall_metrics_on_the_recorded_ranks_equal_the_recorded_dict():
    """tests/golden/clipeval_b6_T4.npz: the reference driver's own itm_eval() on its own evaluate()"""
    from madtp_amd import retrieval_eval as re
    g = np.load(os.path.join(ROOT, "tests", "golden", "clipeval_b6_T4.npz"))
    assert g["image_embeds"].shape == (6, 512) and g["text_embeds"].shape == (18, 512) and g["sims"].shape == (6, 18)
    assert g["vit_lens"].shape == (2, 12) and g["txt_lens"].shape == (1, 12) and float(g["temperature"]) == 4.0
    assert np.array_equal(g["rank_row_i2t"], g["rank_tgt_i2t"].reshape(6, 3).min(1))
    got = re.recall_metrics(g["rank_row_i2t"], g["rank_tgt_t2i"])
    assert got == dict(zip(g["metric_names"].tolist(), g["metrics"].tolist()))
    txt2img, img2txt = rank_ref.pairing(6, 3)
    assert rank_ref.itm_eval(g["sims"].astype(np.float64), g["sims"].T.astype(np.float64), txt2img, img2txt) == got
    assert float(g["gap"]) >= 1e-4 and float(g["gap"]) == min(g["gap_i2t"].min(), g["gap_t2i"].min())


def test_the_recording_is_registered_in_make_golden():
    src = open(os.path.join(ROOT, "tools", "make_golden.py")).read()
    assert '"clipeval_b6_T4": lambda: clip_eval_case("clipeval_b6_T4", 6, 4, 3, 4.0)' in src


def test_no_targets_at_all_and_transposed_views(lib):
    """hip.rank_embeds / rank_scores check the tensors before anything else, so the empty-target path cannot be reached on the
    CPU; what can: target_lists of a set without ground truth gives empty index vectors and flat pointers."""
    from madtp_amd import retrieval_eval as re
    t = re.target_lists([[], [], []], [[], []], 2, 3)
    assert t.i2t_ptr.tolist() == [0, 0, 0] and t.i2t_idx.numel() == 0 and t.t2i_ptr.tolist() == [0, 0, 0, 0]
