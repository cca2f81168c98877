"""bench.py's command line and --dump-outputs writer on CPU (the timed run itself: tests/test_gpu_bench_contract.py)."""
import numpy as np
import pytest

import bench


def test_steps_must_be_positive():
    assert bench.parse_args(["--steps", "3"]).steps == 3
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True

def test_dump_outputs_needs_the_engine():
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--dry-run", "--dump-outputs", "d"])


def test_dump_outputs_writes_ids_as_float64_and_values_as_float32(tmp_path):
    d = tmp_path / "out"
    bench.dump_outputs(d, {"tokens": np.array([3, 31999], np.int32), "logprobs": np.array([-0.5, -1.25], np.float32)})
    t, lp = np.load(d / "tokens.npy"), np.load(d / "logprobs.npy")
    assert t.dtype == np.float64 and t.tolist() == [3.0, 31999.0]
    assert lp.dtype == np.float32 and lp.tolist() == [-0.5, -1.25]
