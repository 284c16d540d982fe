"""bench.py --dump-outputs, host side: what a step returned becomes DIR/<name>.npy in float32 / float64, the whole dump within
64 MB, outputs above their share of it as a sample whose elements are the same in every run."""
import os

import numpy as np
import torch

import bench


def _step_like_outputs():
    g = torch.Generator().manual_seed(3)
    return {
        "depth_est_b1thw": torch.randn(2, 1, 4, 8, 8, generator=g).to(torch.bfloat16),
        "pose": {"R": torch.randn(2, 3, 3, generator=g, dtype=torch.float64), "valid": torch.tensor([True, False])},
        "tracks": [torch.arange(6, dtype=torch.int64).view(2, 3), None],
        "big": torch.randn(3 << 20, generator=g),  # 12 MB of float32: more than one array's share
        "note": "not an array",
    }


def test_dump_names_dtypes_and_values(tmp_path):
    out = _step_like_outputs()
    bench.dump_outputs(out, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(["depth_est_b1thw.npy", "pose.R.npy", "pose.valid.npy", "tracks.0.npy", "big.npy"])
    d = np.load(tmp_path / "depth_est_b1thw.npy")
    assert d.dtype == np.float32 and d.shape == (2, 1, 4, 8, 8)
    assert np.array_equal(d, out["depth_est_b1thw"].float().numpy())
    r = np.load(tmp_path / "pose.R.npy")
    assert r.dtype == np.float64 and np.array_equal(r, out["pose"]["R"].numpy())
    assert np.array_equal(np.load(tmp_path / "pose.valid.npy"), np.array([1.0, 0.0], dtype=np.float32))
    assert np.array_equal(np.load(tmp_path / "tracks.0.npy"), np.arange(6, dtype=np.float32).reshape(2, 3))


def test_dump_samples_large_outputs_within_budget(tmp_path):
    out = _step_like_outputs()
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.dtype == np.float32 and big.ndim == 1 and big.nbytes <= bench.DUMP_ARRAY_BYTES
    assert np.isin(big, out["big"].numpy()).all()  # values of the output, not something derived from it
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))  # the same elements in every run
    # many outputs: every one gets its share, the whole dump stays within the budget
    many = {f"o{i}": torch.randn(1 << 20) for i in range(40)}
    bench.dump_outputs(many, str(tmp_path / "c"))
    total = sum(os.path.getsize(tmp_path / "c" / f) for f in os.listdir(tmp_path / "c"))
    assert len(os.listdir(tmp_path / "c")) == 40 and total <= bench.DUMP_BUDGET_BYTES
