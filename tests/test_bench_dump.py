"""bench.py --dump-outputs without a GPU: the writer of the last timed step's arrays (float64, a fixed, seeded sample of the instances past the
size limit) and the command-line checks that run before any device is opened."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(B, rng):
    return {"u0": rng.standard_normal((B, 2)), "status": rng.integers(0, 5, B).astype(np.int32), "x": rng.standard_normal((B, 41, 8))}


def test_dump_writes_every_array_whole_in_float64(tmp_path):
    import bench

    a = _arrays(50, np.random.default_rng(1))
    names = bench.dump_outputs(str(tmp_path), a)
    assert names == ["status", "u0", "x"]
    for n in names:
        got = np.load(tmp_path / f"{n}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, a[n])
    bench.dump_outputs(str(tmp_path / "r"), a, suffix="_rank1")
    assert sorted(os.listdir(tmp_path / "r")) == ["status_rank1.npy", "u0_rank1.npy", "x_rank1.npy"]


def test_dump_past_the_limit_is_the_same_seeded_sample_in_every_array(tmp_path):
    import bench

    B, limit = 4000, 1 << 20                 # 4000 x 2640 B = 10.6 MB of rows against a 1 MB limit
    a = _arrays(B, np.random.default_rng(2))
    a["row"] = np.arange(B)
    names = bench.dump_outputs(str(tmp_path / "a"), a, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), a, limit=limit)
    assert "sample_index" in names
    total = sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in names)
    assert total <= limit
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert 0 < idx.size < B and np.all(np.diff(idx) > 0) and idx.dtype == np.float64
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "row.npy"), idx)             # every array holds the rows of the index
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "x.npy"), a["x"][idx.astype(np.int64)])
    for n in names:                                                                        # and the sample is the same from run to run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy"))


def test_bench_refuses_arguments_it_could_not_honour_before_opening_a_device():
    for extra, msg in ((["--steps", "0"], "--steps"), (["--warmup", "-1"], "--warmup"),
                       (["--config", "3", "--dump-outputs", "x"], "--dump-outputs"), (["--live-options", "--dump-outputs", "x"], "--dump-outputs")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr[-500:])
