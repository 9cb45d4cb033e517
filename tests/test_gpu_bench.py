"""bench.py's own contract: a plain run times exactly --steps steps and prints one line with the headline fields and
nothing that takes a run of its own; --full adds those; --dump-outputs writes what the last timed step left, the same
arrays from run to run.  Tiny shapes (2 images of 64x64), in-process."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import REPO

if REPO not in sys.path:
    sys.path.insert(0, REPO)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "per_kernel_ms", "full_run", "mixed_branch_run", "cpu_baseline", "step_tflops")
TINY = ["--gpus", "1", "--batch", "2", "--height", "64", "--width", "64", "--steps", "3", "--warmup", "1"]


def _run(monkeypatch, capsys, extra):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + TINY + extra)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    """An array over the per-array limit is written as the same DUMP_MAX_ELEMS elements every time."""
    n = bench.DUMP_MAX_ELEMS + 12345
    x = torch.arange(n, dtype=torch.float32)
    bench._dump_outputs(str(tmp_path / "a"), {"x": x, "s": torch.tensor(2.5, dtype=torch.float64)})
    bench._dump_outputs(str(tmp_path / "b"), {"x": x})
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a, b) and np.all(np.diff(a) >= 0) and a.max() < n
    s = np.load(tmp_path / "a" / "s.npy")
    assert s.dtype == np.float64 and float(s) == 2.5
    assert 3 * 4 * bench.DUMP_MAX_ELEMS < 64 * 2 ** 20   # noise + two Adam moments stay under 64 MB


@pytest.mark.gpu
def test_plain_run_line_and_outputs(monkeypatch, capsys, tmp_path):
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    out = _run(monkeypatch, capsys, ["--dump-outputs", d1])
    for k in HEADLINE:
        assert k in out, k
    assert not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(2 * 1e3 / out["ms_per_step"], rel=1e-2)
    assert out["branch_census"]["image_steps"] == 2 * 3   # --steps sets the timed steps
    _run(monkeypatch, capsys, ["--dump-outputs", d2])
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) == ["adam_m.npy", "adam_v.npy", "branch.npy", "loss_i.npy", "noise.npy"]
    for f in names:
        a, b = np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f))
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
    noise = np.load(os.path.join(d1, "noise.npy"))
    assert noise.shape == (2, 3, 64, 64) and 0 < np.abs(noise).max() <= 16 / 255.0


@pytest.mark.gpu
def test_full_run_adds_the_rest(monkeypatch, capsys):
    out = _run(monkeypatch, capsys, ["--full", "--no-cpu-baseline", "--full-run", "0"])
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["roofline"]["kernel"] in out["per_kernel_ms"]
    assert out["timing"]["profiling_pass_expensive_image_steps"] <= 2 * 3
