"""bench.py's --full / --dump-outputs plumbing. CPU only: option parsing and the .npy writer, no launch."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_measures_the_headline_only():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert a.alt_math == [] and a.head_density == 0
    assert a.no_config5 and a.no_train and a.no_guided and a.no_guided_train and a.no_cpu_baseline


def test_full_keeps_every_leg_and_its_selectors():
    a = bench.parse(["--full"])
    assert a.full and a.alt_math == ["bf16x9", "bf16x3"] and a.head_density == 0.40
    assert not (a.no_config5 or a.no_train or a.no_guided or a.no_guided_train or a.no_cpu_baseline)
    a = bench.parse(["--full", "--no-train", "--alt-math", ""])
    assert a.no_train and a.alt_math == [] and not a.no_guided


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_float32_npy(tmp_path):
    x = torch.arange(24, dtype=torch.float32).reshape(2, 1, 3, 4)
    bench.dump_outputs(str(tmp_path / "d"), {"estimated_depth": x})
    y = np.load(tmp_path / "d" / "estimated_depth.npy")
    assert y.dtype == np.float32 and y.shape == (2, 1, 3, 4) and (y == x.numpy()).all()
    bench.dump_outputs(str(tmp_path / "d"), {"estimated_depth": x.double()}, rank=1)
    assert np.load(tmp_path / "d" / "estimated_depth_rank1.npy").dtype == np.float64


def test_dump_outputs_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 400)
    x = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    bench.dump_outputs(str(tmp_path / "a"), {"y": x})
    bench.dump_outputs(str(tmp_path / "b"), {"y": x})
    ya, yb = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert ya.dtype == np.float32 and ya.shape == (100,) and ya.nbytes <= 400
    assert (ya == yb).all() and (np.diff(ya) > 0).all()  # distinct elements of x, in order
