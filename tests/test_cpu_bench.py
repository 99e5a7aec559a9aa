"""bench.py's output dump, host side: arrays land as .npy files; a set larger than the budget is cut to a fixed, seeded
sample, the same on every run."""

import numpy as np

import bench


def test_dump_outputs_writes_npy_files(tmp_path):
    arrays = {"loss": np.array(1.5, dtype=np.float64), "offsets": np.arange(12, dtype=np.float32).reshape(3, 4)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(got, a)


def test_dump_outputs_samples_a_large_set_the_same_way_every_time(tmp_path):
    arrays = {"params": np.arange(3000, dtype=np.float32), "loss": np.array(2.0, dtype=np.float64)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=4000)
    got = {d: {n: np.load(tmp_path / d / f"{n}.npy") for n in arrays} for d in ("a", "b")}
    assert sum(a.nbytes for a in got["a"].values()) <= 4000
    p = got["a"]["params"]
    assert 0 < p.size < 3000 and p.dtype == np.float32
    assert np.all(np.diff(p) > 0)                          # elements of the original, in their original order
    assert np.array_equal(p, got["b"]["params"])           # the same sample on every run
    assert got["a"]["loss"].size == 1 and got["a"]["loss"].item() == 2.0
