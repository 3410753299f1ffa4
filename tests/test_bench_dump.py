"""CPU: what `bench.py --dump-outputs DIR` writes - the whole frame up to DUMP_MAX_PIXELS pixels, else the same fixed
sample in every run, float32 and within 64 MB."""
import numpy as np


def _bench():
    import bench
    return bench


def test_dump_sample_is_fixed_distinct_and_in_range():
    bench = _bench()
    limit = bench.DUMP_MAX_PIXELS
    assert bench.dump_sample_index(1920 * 1080) is None
    assert bench.dump_sample_index(limit) is None
    for n in (limit + 1, 4096 * 4096, 8192 * 8192):
        idx = bench.dump_sample_index(n)
        assert np.array_equal(idx, bench.dump_sample_index(n))
        assert len(idx) == limit and idx[0] >= 0 and idx[-1] < n
        assert np.all(np.diff(idx) > 0)


def test_dump_outputs_writes_the_sampled_frame(tmp_path):
    bench = _bench()
    n = bench.DUMP_MAX_PIXELS + 12345
    frame = np.arange(n * 4, dtype=np.float32).reshape(n, 4)
    bench.dump_outputs(str(tmp_path / "out"), frame)
    path = tmp_path / "out" / "frame.npy"
    got = np.load(path)
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_MAX_PIXELS, 4)
    assert np.array_equal(got, frame[bench.dump_sample_index(n)])
    assert path.stat().st_size <= 64 << 20

    small = frame[:1000]
    bench.dump_outputs(str(tmp_path / "small"), small)
    assert np.array_equal(np.load(tmp_path / "small" / "frame.npy"), small)
