"""bench.py --dump-outputs: what it writes (CPU only; the GPU side is the timed path itself)."""
import os

import numpy as np
import torch

import bench


def test_dump_dtypes_and_names(tmp_path):
    arrays = bench.dump_arrays("retrieval", (torch.randn(4, 2, dtype=torch.bfloat16), torch.arange(5)))
    rep = bench.write_dump(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["itc_similarity.npy", "itm_logits.npy"]
    a, b = np.load(tmp_path / "itm_logits.npy"), np.load(tmp_path / "itc_similarity.npy")
    assert a.dtype == np.float32 and a.shape == (4, 2)
    assert b.dtype == np.float64 and b.tolist() == list(range(5))
    assert not rep["sampled"]


def test_dump_stays_under_64_mb_and_samples_the_same_elements(tmp_path):
    big = torch.randn(20_000_000)  # 80 MB as float32
    small = torch.randn(10)
    for d in ("a", "b"):
        rep = bench.write_dump(str(tmp_path / d), [("big", big), ("small", small)])
        assert rep["sampled"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64_000_000
    assert np.array_equal(np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())  # small outputs are kept whole
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and np.isin(s, big.numpy()).all()
