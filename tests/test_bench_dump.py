"""bench.py --dump-outputs on CPU: what is written for a dump of config-2 size (the visibilities of the last timed step)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_is_a_fixed_exact_sample_under_64_mb(tmp_path):
    """Float64 files of at most 64 MB in all; the same positions on every call, both planes at each; every value exact."""
    vis = np.random.RandomState(3).randint(-2 ** 31, 2 ** 31 - 1, size=2 * bench.NCHAN * 249216, dtype=np.int64).astype(np.int32)
    bench.dump_outputs(str(tmp_path / "a"), vis, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), vis[::-1].copy(), 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["visibilities.npy", "visibilities_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 2 ** 20
    got, idx = np.load(tmp_path / "a" / "visibilities.npy"), np.load(tmp_path / "a" / "visibilities_index.npy")
    assert got.dtype == idx.dtype == np.float64
    assert np.array_equal(idx, np.load(tmp_path / "b" / "visibilities_index.npy"))
    assert got.shape == (2, bench.DUMP_SAMPLE) and np.all(np.diff(idx) > 0)
    assert np.array_equal(got, vis.reshape(2, -1)[:, idx.astype(np.int64)].astype(np.float64))
    bench.dump_outputs(str(tmp_path / "r"), vis, 1, 2)
    assert sorted(os.listdir(tmp_path / "r")) == ["visibilities_index_rank1.npy", "visibilities_rank1.npy"]


def test_dump_outputs_refuses_the_workloads_it_does_not_dump(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "config5", "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
