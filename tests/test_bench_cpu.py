"""bench.py's options and its --dump-outputs writer, without a GPU"""
import os

import numpy as np

import bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse(["--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_write_outputs_float_dtypes_and_seeded_sample(tmp_path):
    n = 1000
    arrays = {"board": np.arange(n * 25).astype(np.int8).reshape(n, 5, 5), "reward": np.linspace(-1.0, 1.0, n),
              "flags": np.arange(n).astype(np.uint8)}
    names = bench.write_outputs(str(tmp_path / "all"), arrays)
    assert names == ["board", "flags", "reward"]
    for name in names:
        a = np.load(str(tmp_path / "all" / (name + ".npy")))
        assert a.dtype == (np.float64 if name == "reward" else np.float32)
        assert np.array_equal(a, arrays[name].astype(a.dtype))
    # past the limit: the same seeded lanes from every array, their indices in lane_index.npy, the files within the limit
    limit = 20000
    for d in ("s1", "s2"):
        assert bench.write_outputs(str(tmp_path / d), arrays, limit=limit) == ["board", "flags", "lane_index", "reward"]
    s1 = {f[:-4]: np.load(str(tmp_path / "s1" / f)) for f in os.listdir(str(tmp_path / "s1"))}
    s2 = {f[:-4]: np.load(str(tmp_path / "s2" / f)) for f in os.listdir(str(tmp_path / "s2"))}
    idx = s1["lane_index"].astype(np.int64)
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0) and s1["lane_index"].dtype == np.float64
    for name, a in s1.items():
        assert np.array_equal(a, s2[name])
        if name != "lane_index":
            assert np.array_equal(a, arrays[name][idx].astype(a.dtype))
    assert sum(a.nbytes for a in s1.values()) <= limit
