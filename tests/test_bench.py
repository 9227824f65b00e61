"""bench.py's host-side helpers on CPU (the oracle's kinematics stand in for the HIP library's):
  * `generate`: the random draws of every batch run in the worker processes, the kinematics they need are computed in the
    main process and replayed -- the batches must equal scenes.make_batch bitwise, seed for seed;
  * `write_outputs` (--dump-outputs): every array as float64 .npy, within the byte budget, the same seeded rows each time."""
import multiprocessing
import os

import numpy as np
import pytest

import bench
import oracle_lib as O
from boundplanner_amd import scenes


def test_generate_equals_make_batch():
    N, B = 6, 48
    seeds = [8192, [8192, 1], [65536, 0, 1]]
    pool = multiprocessing.get_context("fork").Pool(2)
    try:
        got = list(bench.generate(seeds, B, N, O.fk_batch, pool))
    finally:
        pool.close(); pool.join()
    assert len(got) == len(seeds)
    for seed, g in zip(seeds, got):
        ref = scenes.make_batch(B, N, seed, O.fk_batch, randomize_sets=True)
        for k in ("x0", "lbx", "ubx", "p"):
            assert np.array_equal(g[k], ref[k], equal_nan=True), (seed, k)
    alone = next(bench.generate(seeds[:1], B, N, O.fk_batch, None))
    for k in ("x0", "lbx", "ubx", "p"):
        assert np.array_equal(alone[k], got[0][k], equal_nan=True), k


def test_replayed_kinematics_must_match():
    rec, calls = bench._fk_recorder(O.fk_batch)
    q = np.zeros((3, 7))
    rec(q)
    replay = bench._fk_replayer(calls)
    with pytest.raises(RuntimeError):
        replay(q + 1.0)


def test_write_outputs_within_budget(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"x": rng.normal(size=(100, 50)), "f": rng.normal(size=100), "iters": np.arange(100, dtype=np.int32)}
    bench.write_outputs(str(tmp_path / "all"), [("", arrays)], budget=10 ** 6)
    for k, v in arrays.items():
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, v)
    assert not (tmp_path / "all" / "rows.npy").exists()

    budget = 20_000                       # 100 rows of 52 doubles do not fit: a sample of rows does
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), [("", arrays), ("gathered_", {"x": arrays["x"]})], budget=budget)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["f.npy", "gathered_rows.npy", "gathered_x.npy", "iters.npy", "rows.npy", "x.npy"]
    data_bytes = sum(np.load(tmp_path / "s1" / f).nbytes for f in files)
    assert data_bytes <= budget
    rows = np.load(tmp_path / "s1" / "rows.npy").astype(int)
    assert len(rows) > 0 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "s1" / "x.npy"), arrays["x"][rows])
    assert np.array_equal(np.load(tmp_path / "s1" / "iters.npy"), arrays["iters"][rows])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)), f
