"""bench.py's command line, in-process on an MI355X at a small batch:
  * a plain run prints the headline line only -- `--steps` timed steps,
    `ms_per_step`, no roofline / baseline / parity keys;
  * `--dump-outputs DIR` writes the last timed step's loss, gradient and
    parameters as float32 .npy files, the same arguments giving the same
    arrays from run to run;
  * `--full` adds the per-kernel, roofline and accuracy keys to the same line.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "roofline_other_mfma", "roofline_path_step", "allreduce_us", "step_alg_tflops",
             "step_kernel_ms", "accuracy", "cpu_baseline")


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench as b
    return b


def run(bench, monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--paths-per-gpu", "128", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    rng, crng = torch.get_rng_state(), torch.cuda.get_rng_state(0)   # main() seeds torch: put the streams back
    try:
        bench.main()
    finally:
        torch.set_rng_state(rng)
        torch.cuda.set_rng_state(crng, 0)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only_and_dumps_its_outputs(bench, monkeypatch, capsys, tmp_path):
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        out = run(bench, monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--dump-outputs", str(d))
        for k in HEADLINE:
            assert k in out, k
        assert not set(FULL_ONLY) & set(out), sorted(out)
        assert out["steps"] == 3 and out["warmup"] == 2
        assert out["unit"] == "path-steps/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
        assert out["ms_per_step"] > 0
        # value and ms_per_step describe the same timed window: paths x time steps per step time
        assert out["value"] == pytest.approx(128 * 50 / (out["ms_per_step"] * 1e-3), rel=1e-9)
        assert sorted(os.listdir(d)) == ["grad.npy", "loss.npy", "params.npy"]
        arrs = {n: np.load(d / (n + ".npy")) for n in ("loss", "grad", "params")}
        for n, a in arrs.items():
            assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all(), n
        assert arrs["loss"].shape == (1,) and arrs["grad"].shape == arrs["params"].shape
        assert float(arrs["loss"][0]) == pytest.approx(out["final_loss"], rel=1e-6)
        assert np.abs(arrs["grad"]).max() > 0
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
        dumps.append(arrs)
    # same arguments, same inputs; the kernels reduce in a fixed order (no
    # floating-point atomics), so the same build gives the same bits
    for n in ("loss", "grad", "params"):
        np.testing.assert_array_equal(dumps[0][n], dumps[1][n], err_msg=n)


def test_full_run_adds_the_other_measurements(bench, monkeypatch, capsys):
    out = run(bench, monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline",
              "--no-parity")
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert out["roofline"]["achieved"] > 0 and out["step_kernel_ms"]
    assert out["cpu_baseline"] is None and out["accuracy"]["parity"] is None
    assert out["accuracy"]["bench_model"]["train_iterations"] == 1 + 3 + 3
