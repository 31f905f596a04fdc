"""bench.py --dump-outputs (bench.dump_outputs) on the CPU: the seeded row sample a large output
is written as (the default Twitter-World run takes that branch), and the all-rows case."""
import numpy as np
import torch

import bench
from graphconvgeo_amd.synth import SEED

K, LD, N_ROWS = 5, 8, 20


def _strided_output():
    """An N_ROWS x K view of wider rows, as sparse.empty_dense lays the bench's Y out."""
    base = torch.arange(N_ROWS * LD, dtype=torch.float32).reshape(N_ROWS, LD)
    return base[:, :K]


def _sample(rank, keep):
    return np.sort(np.random.default_rng(SEED + rank).choice(N_ROWS, size=keep, replace=False))


def test_dump_outputs_row_sample(tmp_path, monkeypatch):
    budget = 4 * K * 7  # room for 7 of the 20 rows
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    Y = _strided_output()
    info = bench.dump_outputs(str(tmp_path / "a"), Y, K, 0, 1)
    assert [p.name for p in (tmp_path / "a").iterdir()] == ["Y.npy"]
    arr = np.load(tmp_path / "a" / "Y.npy")
    rows = _sample(0, 7)
    assert len(set(rows.tolist())) == 7 and list(rows) == sorted(rows)
    assert arr.dtype == np.float32 and arr.shape == (7, K) and arr.nbytes <= budget
    assert np.array_equal(arr, Y.numpy()[rows])
    assert info["Y"]["shape"] == [7, K] and info["Y"]["dtype"] == "float32"
    # the same arguments write the same file
    bench.dump_outputs(str(tmp_path / "b"), Y, K, 0, 1)
    assert (tmp_path / "a" / "Y.npy").read_bytes() == (tmp_path / "b" / "Y.npy").read_bytes()


def test_dump_outputs_ranks_share_the_budget(tmp_path, monkeypatch):
    budget = 4 * K * 7
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    Y = _strided_output()
    total = 0
    for rank in (0, 1):
        info = bench.dump_outputs(str(tmp_path), Y, K, rank, 2)
        arr = np.load(tmp_path / f"Y_rank{rank}.npy")
        assert list(info) == [f"Y_rank{rank}"] and arr.shape == (3, K)  # (budget / 2) // (4 K)
        assert np.array_equal(arr, Y.numpy()[_sample(rank, 3)])
        total += arr.nbytes
    assert total <= budget


def test_dump_outputs_all_rows_when_they_fit(tmp_path):
    Y = _strided_output()
    info = bench.dump_outputs(str(tmp_path), Y, K, 0, 1)
    arr = np.load(tmp_path / "Y.npy")
    assert arr.dtype == np.float32 and np.array_equal(arr, Y.numpy())
    assert info["Y"]["rows"] == f"all {N_ROWS} rows"
    assert bench.DUMP_BUDGET_BYTES <= 64 * 10**6
