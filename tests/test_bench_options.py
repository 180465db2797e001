"""bench.py's options on CPU: a plain run is the default (--full off, nothing dumped), --steps / --warmup are checked,
and the --dump-outputs writer keeps under its byte limit with the same fixed sample every time."""
import numpy as np
import pytest


def test_plain_run_is_the_default():
    import bench
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None and a.steps == 200 and a.warmup == 20
    a = bench.parse_args(["--steps", "5", "--warmup", "0", "--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out" and a.steps == 5 and a.warmup == 0
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_writes_whole_arrays_under_the_limit(tmp_path):
    import bench
    arrays = {"x": np.arange(12, dtype=np.float32).reshape(3, 4), "s": np.array([0.5, 1.5])}
    assert bench.write_outputs(arrays, str(tmp_path)) == {"x": 12, "s": 2}
    for k, v in arrays.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_dump_samples_the_large_arrays_over_the_limit(tmp_path):
    import bench
    arrays = {"big": np.arange(100_000, dtype=np.float64), "mid": np.arange(20_000, dtype=np.float32),
              "small": np.arange(1_000, dtype=np.float32), "scalars": np.array([0.25, 2.0])}
    limit, whole = 80_000, 10_000
    n1 = bench.write_outputs(arrays, str(tmp_path / "a"), limit=limit, whole=whole)
    n2 = bench.write_outputs(arrays, str(tmp_path / "b"), limit=limit, whole=whole)
    assert n1 == n2 and n1["big"] < 100_000 and n1["mid"] < 20_000
    assert n1["small"] == 1_000 and n1["scalars"] == 2                   # small arrays are never sampled
    assert abs(n1["big"] / 100_000 - n1["mid"] / 20_000) < 1e-3          # the large ones keep the same fraction
    assert sum(n1[k] * arrays[k].itemsize for k in arrays) <= limit
    for k, v in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b) and a.dtype == v.dtype            # the same sample in every run
        assert (np.diff(a) > 0).all() and np.isin(a, v).all()          # elements of the array, in their order
    assert np.array_equal(np.load(tmp_path / "a" / "scalars.npy"), arrays["scalars"])
    with pytest.raises(TypeError):
        bench.write_outputs({"i": np.arange(3)}, str(tmp_path / "c"))             # integers: not an output format
    with pytest.raises(ValueError):                                                 # nothing left for the large ones
        bench.write_outputs({"s": np.zeros(1_000), "big": np.zeros(100_000)}, str(tmp_path / "d"), limit=8_000, whole=8_000)
