"""bench.py --dump-outputs on the host (no GPU): file names, dtypes, and the fixed sample that keeps a large state under the cap."""
import numpy as np

import bench


def test_dump_outputs_small_state_is_written_whole(tmp_path):
    rng = np.random.default_rng(1)
    st = dict(z=rng.normal(size=(4, 3, 3, 2)).astype(np.float32), theta=None, key=np.array([7, 2 ** 32 - 1], np.uint32),
              baseline=rng.normal(size=4).astype(np.float32))
    bench.dump_outputs(str(tmp_path), st)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["baseline.npy", "key.npy", "z.npy"]
    z, key = np.load(tmp_path / "z.npy"), np.load(tmp_path / "key.npy")
    assert z.dtype == np.float32 and np.array_equal(z, st["z"])
    assert key.dtype == np.float64 and np.array_equal(key, [7.0, 2.0 ** 32 - 1])


def test_dump_outputs_large_state_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    st = dict(z=np.arange(3000, dtype=np.float32).reshape(30, 100), baseline=np.arange(30, dtype=np.float32))
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), st)
    total = sum(p.stat().st_size - 128 for p in (tmp_path / "a").iterdir())   # (.npy header: 128 bytes)
    assert total <= 4096
    z = np.load(tmp_path / "a" / "z.npy")
    assert z.ndim == 1 and 0 < z.size < 3000 and np.all(np.diff(z) > 0)        # a sample of distinct elements, in order
    assert np.array_equal(z, np.load(tmp_path / "b" / "z.npy"))                 # the same sample every time
    assert np.array_equal(np.load(tmp_path / "a" / "baseline.npy"), st["baseline"])
