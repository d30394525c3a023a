"""bench.py's command line: a plain run measures the headline only (``--full`` adds the other legs), and ``--dump-outputs DIR``
writes the last timed step's outputs as float .npy files, at most 64 MB in all, the same rows in every run.  CPU tests: they
exercise the option parser and the writer, no GPU."""
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _parse(monkeypatch, argv):
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "37", "--warmup", "3"])
    assert a.full is False and a.dump_outputs == "" and a.steps == 37 and a.warmup == 3
    a = _parse(monkeypatch, ["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_every_array_as_given_under_the_limit(tmp_path):
    bench = importlib.import_module("bench")
    rng = np.random.default_rng(1)
    arrays = dict(loss=np.array([3.5]), grad_x=rng.standard_normal((1000, 2)), grad_u=rng.standard_normal((900, 2)).astype(np.float32))
    shapes = bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert shapes == {"loss": [1], "grad_x": [1000, 2], "grad_u": [900, 2]}
    for k, v in arrays.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_dump_outputs_samples_the_same_rows_when_over_the_limit(tmp_path):
    bench = importlib.import_module("bench")
    big = np.arange(40000, dtype=np.float64).reshape(-1, 4)        # 10000 rows of 32 B
    arrays = dict(loss=np.array([1.0]), g=big)
    a = bench.dump_outputs(str(tmp_path / "a"), arrays, max_bytes=64 * 1024)
    b = bench.dump_outputs(str(tmp_path / "b"), arrays, max_bytes=64 * 1024)
    ga, gb = np.load(tmp_path / "a" / "g.npy"), np.load(tmp_path / "b" / "g.npy")
    assert a == b and np.array_equal(ga, gb), "the sample is fixed: two runs write the same rows"
    assert ga.nbytes <= 64 * 1024 and ga.shape[0] >= 2000 and ga.shape[1] == 4
    rows = ga[:, 0] / 4
    assert np.all(np.diff(rows) > 0) and np.array_equal(ga, big[rows.astype(np.int64)]), "whole rows, ascending order"
    assert np.array_equal(np.load(tmp_path / "a" / "loss.npy"), arrays["loss"])
    # the default limit keeps the files under 64 MB
    assert bench.DUMP_BYTES_MAX + 3 * 4096 <= 64 * 2 ** 20


def test_dump_outputs_refuses_non_float_arrays(tmp_path):
    bench = importlib.import_module("bench")
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), dict(idx=np.arange(4)))
