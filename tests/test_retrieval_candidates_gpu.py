"""blip_retrieval.evaluate(candidates="device") on a real MI355X: the k_test candidates of every row come from two
search.topk_embeds calls and no sims_matrix is formed.  Against the score matrices the reference's own evaluate() recorded
(tests/golden/retr_*.npz) and against the default candidates="dense" path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["retr_i6_t12", "retr_384_i4_t6"]


@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("case", CASES)
def test_device_candidates_match_the_recording_and_the_dense_path(case, mode, monkeypatch):
    """The -100 pattern equals the recording's, the scores are within its 1e-3, two rank slices merge to the whole, and against
    candidates="dense" the pattern is equal and the scores differ only by the ITC term's f32 rounding (the exact-f32 MFMA chain
    of search.hip against the dense f32 matmul): measured 6.0e-08 to 1.2e-07 on the four cases, asserted under 1e-5."""
    from madtp_amd import build, hip, harness, runtime, search
    from madtp_amd import blip_retrieval as br
    build.build(verbose=False)
    hip.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", case + ".npz"))
    n_img, img_bs, n_txt, size = int(g["n_img"]), int(g["img_bs"]), int(g["n_txt"]), int(g["size"])
    T, k_test, seed = float(g["temperature"]), int(g["k_test"]), int(g["seed"])
    model = harness.build_retrieval(size, seed)
    batches, ids, att = harness.retrieval_inputs(n_img, img_bs, n_txt, size, 35, seed, device="cuda")
    loader = harness.RetrievalLoader(batches, ids, att)
    cfg = {"k_test": k_test}
    calls = []
    real = search.topk_embeds
    monkeypatch.setattr(search, "topk_embeds", lambda q, keys, k: (calls.append((tuple(q.shape), tuple(keys.shape), k)), real(q, keys, k))[1])
    with runtime.precision(mode):
        i2t, t2i, gflops = br.evaluate(model, loader, torch.device("cuda"), cfg, T, candidates="device")
        assert [(c[0][0], c[1][0], c[2]) for c in calls] == [(n_img, n_txt, k_test), (n_txt, n_img, k_test)]  # two calls, before the loops
        parts = [br.evaluate(model, loader, torch.device("cuda"), cfg, T, rank=r, world_size=2, candidates="device") for r in range(2)]
        n_calls = len(calls)
        d_i2t, d_t2i, _ = br.evaluate(model, loader, torch.device("cuda"), cfg, T)  # the default: dense
        assert len(calls) == n_calls  # (the default path does not come here)
        nc_i2t, nc_t2i, _ = br.evaluate(model, loader, torch.device("cuda"), cfg, T, kv_cache=False, candidates="device")
    assert gflops == 0.0
    for ours, ref in ((i2t, g["score_i2t"]), (t2i, g["score_t2i"])):
        assert ((ours == -100.0) == (ref == -100.0)).all()
        assert np.abs(ours - ref).max() < 1e-3
    for k, full in ((0, i2t), (1, t2i)):
        merged = np.where(parts[0][k] != -100.0, parts[0][k], parts[1][k])
        assert np.array_equal(merged, full)
        assert not ((parts[0][k] != -100.0) & (parts[1][k] != -100.0)).any()
    assert np.array_equal(nc_i2t, i2t) and np.array_equal(nc_t2i, t2i)  # the K/V cache changes no bit here either
    worst = 0.0
    for ours, dense in ((i2t, d_i2t), (t2i, d_t2i)):
        assert ((ours == -100.0) == (dense == -100.0)).all()
        worst = max(worst, float(np.abs(ours - dense).max()))
    print(f"{case} {mode}: max |device - dense| = {worst:.3g}")
    assert worst < 1e-5
