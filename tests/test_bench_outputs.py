"""CPU: bench.py --dump-outputs writes a fixed seeded sample of the step's outputs as float32 / float64 .npy files."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_sample_and_dtypes(tmp_path):
    B, L = 5000, 3
    g = torch.Generator().manual_seed(1)
    phi = torch.randn(B, 16, dtype=torch.complex64, generator=g)
    head = torch.randn(3, B, L, generator=g)
    counts = torch.randint(0, 9, (B,), dtype=torch.int32, generator=g)
    outs = {"head": (head, 1), "peak_counts": (counts, 0)}
    bench.dump_outputs(str(tmp_path / "a"), phi, outs)
    bench.dump_outputs(str(tmp_path / "b"), phi, outs)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["head.npy", "peak_counts.npy", "phi.npy", "signal_index.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    idx = np.load(tmp_path / "a" / "signal_index.npy").astype(np.int64)
    assert len(idx) == bench.DUMP_ROWS and np.all(np.diff(idx) > 0) and idx[-1] < B
    assert np.array_equal(np.load(tmp_path / "a" / "phi.npy"), torch.view_as_real(phi[idx]).numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "head.npy"), head[:, idx].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "peak_counts.npy"), counts[idx].numpy().astype(np.float64))


def test_dump_outputs_small_batch_is_whole(tmp_path):
    B = 7
    bench.dump_outputs(str(tmp_path), torch.ones(B, 4, dtype=torch.complex64), {})
    assert np.array_equal(np.load(tmp_path / "signal_index.npy"), np.arange(B, dtype=np.float64))
    assert np.load(tmp_path / "phi.npy").shape == (B, 4, 2)
