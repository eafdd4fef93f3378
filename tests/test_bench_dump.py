"""bench.py --dump-outputs on the host: the writer of the output files (no GPU; bench.py runs in a child process, since importing
it sets GPU_MAX_HW_QUEUES for the process that imports it)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dump(out_dir, arrays_npz):
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import bench; a = np.load(%r); "
            "bench.dump_outputs(%r, {k: a[k] for k in a.files})" % (ROOT, arrays_npz, out_dir))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)


def test_small_outputs_are_written_whole_as_float64(tmp_path):
    z = np.random.default_rng(1).standard_normal((64, 184)); st = np.arange(64, dtype=np.int32) % 7
    np.savez(tmp_path / "in.npz", z=z, status=st)
    _dump(str(tmp_path / "out"), str(tmp_path / "in.npz"))
    assert sorted(os.listdir(tmp_path / "out")) == ["status.npy", "z.npy"]
    got_z, got_st = np.load(tmp_path / "out" / "z.npy"), np.load(tmp_path / "out" / "status.npy")
    assert got_z.dtype == np.float64 and np.array_equal(got_z, z)
    assert got_st.dtype == np.float64 and np.array_equal(got_st, st)


def test_large_outputs_keep_a_fixed_sample_of_rows_within_64_mb(tmp_path):
    B = 50000                                                   # z alone is 73.6 MB
    z = np.random.default_rng(2).standard_normal((B, 184)); st = (np.arange(B) % 7).astype(np.int32)
    np.savez(tmp_path / "in.npz", z=z, status=st)
    for d in ("a", "b"):
        _dump(str(tmp_path / d), str(tmp_path / "in.npz"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20
    for name, full in (("z", z), ("status", st)):
        rows = np.load(tmp_path / "a" / (name + "_rows.npy"))
        assert np.array_equal(rows, np.load(tmp_path / "b" / (name + "_rows.npy")))          # the same sample every run
        idx = rows.astype(np.int64)
        assert np.array_equal(idx, rows) and np.all(np.diff(idx) > 0) and 0 < len(idx) < B
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), full[idx])
