"""bench.py's options and its output dump, on the CPU (the dump takes any torch tensor; the GPU run itself is smoke / bench)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _edges(m, seed=3):
    import torch
    rng = np.random.default_rng(seed)
    e = np.stack([rng.integers(0, 90_000_000, m), rng.integers(0, 90_000_000, m), rng.integers(0, 150, m)], axis=1).astype(np.int32)
    return torch.from_numpy(e), e


def test_plain_run_is_the_default():
    a = bench.parse_args(["--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    b = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert b.full and b.dump_outputs == "d"


def test_small_list_is_dumped_whole_and_exactly(tmp_path):
    t, e = _edges(1000)
    bench.dump_outputs(str(tmp_path), t)
    got = np.load(tmp_path / "edges.npy")
    assert got.dtype == np.float64 and (got == e).all()
    assert not (tmp_path / "edges_rows.npy").exists()
    dg = np.load(tmp_path / "edges_digest.npy")
    assert dg.dtype == np.float64 and dg[0] == 1000 and (dg[1:] < 65536).all()


def test_large_list_is_a_fixed_sample_under_64_mb(tmp_path):
    m = bench.DUMP_ROWS + 123_457
    t, e = _edges(m)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), t)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["edges.npy", "edges_digest.npy", "edges_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    for f in files:
        assert (np.load(tmp_path / "a" / f) == np.load(tmp_path / "b" / f)).all()
    rows = np.load(tmp_path / "a" / "edges_rows.npy").astype(np.int64)
    assert (np.diff(rows) > 0).all() and rows[-1] < m
    assert (np.load(tmp_path / "a" / "edges.npy") == e[rows]).all()
    # the digest covers the whole list: one changed edge outside the sample changes it
    outside = np.setdiff1d(np.arange(m), rows)[0]
    t[outside, 2] += 1
    bench.dump_outputs(str(tmp_path / "c"), t)
    assert (np.load(tmp_path / "c" / "edges.npy") == np.load(tmp_path / "a" / "edges.npy")).all()
    assert (np.load(tmp_path / "c" / "edges_digest.npy") != np.load(tmp_path / "a" / "edges_digest.npy")).any()
