"""bench.py --dump-outputs: the files dump_outputs writes (CPU only; no GPU, no bench run).

Whole iterate when it fits the size cap, else a fixed seeded sample with its row numbers;
float64 throughout; the same call writes the same files; all ranks together stay below the cap."""
import os

import numpy as np

import bench


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_whole_iterate_when_it_fits(tmp_path):
    x, hist = np.linspace(-1.0, 1.0, 1001), np.array([3.0, 1.0, 0.25])
    bench.dump_outputs(str(tmp_path), x, hist, 0, 1)
    got = _load(tmp_path)
    assert sorted(got) == ["residual_history.npy", "x.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["x.npy"], x) and np.array_equal(got["residual_history.npy"], hist)


def test_seeded_sample_above_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    x, hist = np.random.default_rng(1).standard_normal(1001), np.array([2.0, 1.0])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), x, hist, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["residual_history.npy", "x_sample.npy", "x_sample_index.npy"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)  # same arguments, same files
    idx = a["x_sample_index.npy"].astype(np.int64)
    assert idx.size == 100 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < x.size
    assert np.array_equal(a["x_sample.npy"], x[idx])
    assert sum(v.nbytes for v in a.values()) <= 4096


def test_ranks_share_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    x, hist = np.arange(300.0), np.array([1.0, 0.5])
    for r in range(4):
        bench.dump_outputs(str(tmp_path), x + r, hist, r, 4)
    got = _load(tmp_path)
    assert sorted(got) == (["residual_history.npy"] + [f"x_sample_index_rank{r}.npy" for r in range(4)]
                           + [f"x_sample_rank{r}.npy" for r in range(4)])
    assert sum(v.nbytes for v in got.values()) <= 4096
    for r in range(4):
        idx = got[f"x_sample_index_rank{r}.npy"].astype(np.int64)
        assert idx.size == 25 and np.array_equal(got[f"x_sample_rank{r}.npy"], x[idx] + r)
