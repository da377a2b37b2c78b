"""bench.py --dump-outputs (CPU part): the arrays written for one step's outputs.

Every status field and ThrottleMillis is a u32, written as float64 (exact); a batch above
bench.DUMP_ROWS descriptors is written as a fixed, seeded sample of rows, so two builds given the
same arguments write comparable files of at most 64 MB in all.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _outputs(d, seed):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 2**32, size=(d, 5), dtype=np.uint64).astype(np.uint32)
    thr = rng.integers(0, 2**32, size=d, dtype=np.uint64).astype(np.uint32)
    # the device buffers' types: statuses as bytes, ThrottleMillis as int32
    return st, thr, (torch.from_numpy(st.view(np.uint8).reshape(-1)), torch.from_numpy(thr.view(np.int32)))


def _load(p):
    return {f.name: np.load(f) for f in sorted(Path(p).iterdir())}


def test_whole_batch_is_written_exactly(tmp_path):
    d = 3001
    st, thr, out = _outputs(d, 1)
    bench.dump_outputs(tmp_path / "a", out, d, 0, 1)
    got = _load(tmp_path / "a")
    assert sorted(got) == ["status.npy", "throttle_ms.npy"]
    assert got["status.npy"].dtype == np.float64 and got["status.npy"].shape == (d, 5)
    assert got["throttle_ms.npy"].dtype == np.float64 and got["throttle_ms.npy"].shape == (d,)
    assert np.array_equal(got["status.npy"], st.astype(np.float64))
    assert np.array_equal(got["throttle_ms.npy"], thr.astype(np.float64))


def test_large_batch_is_a_fixed_sample_within_64_mb(tmp_path):
    d = bench.DUMP_ROWS + 70_001
    st, thr, out = _outputs(d, 2)
    bench.dump_outputs(tmp_path / "a", out, d, 0, 1)
    bench.dump_outputs(tmp_path / "b", out, d, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["sample_index.npy", "status.npy", "throttle_ms.npy"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 10**6
    idx = a["sample_index.npy"].astype(np.int64)
    assert len(idx) == bench.DUMP_ROWS and len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < d
    assert np.array_equal(a["status.npy"], st[idx].astype(np.float64))
    assert np.array_equal(a["throttle_ms.npy"], thr[idx].astype(np.float64))


def test_other_ranks_write_their_own_files(tmp_path):
    d = 17
    _, _, out = _outputs(d, 3)
    bench.dump_outputs(tmp_path, out, d, 2, 4)
    assert sorted(f.name for f in tmp_path.iterdir()) == ["status_rank2.npy", "throttle_ms_rank2.npy"]
