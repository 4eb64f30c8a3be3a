"""Guards for the bench.py driver contract.

The round driver invokes `python bench.py --gpus N --steps K --warmup W`
(N>1 via torch.distributed.run OR directly — bench.py self-launches) and
parses ONE JSON line from rank 0.  These tests run the ref backend on
tiny synthetic data to lock the surface without a GPU.
"""

import json
import os
import subprocess
import sys

import pytest

from flake16_framework_amd.dataset.synthetic import make_synthetic_tests

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def _run_bench(*args, timeout=420):
    env = dict(os.environ, PYTHONPATH=REPO)
    proc = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), *args],
        capture_output=True, text=True, timeout=timeout, env=env, cwd=REPO)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    lines = [ln for ln in proc.stdout.strip().splitlines()
             if ln.startswith("{")]
    assert lines, proc.stdout
    return json.loads(lines[-1])


@pytest.mark.timeout(600)
def test_single_rank_json_contract():
    out = _run_bench("--backend", "ref", "--cells", "3", "--n-tests", "300",
                     "--steps", "1", "--warmup", "0")
    assert REQUIRED_KEYS <= set(out)
    assert out["n_gpus"] == 1
    assert out["steps"] == 1 and out["warmup"] == 0
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["higher_is_better"] is True
    assert out["scaling"] == "strong"
    assert out["data"] == "synthetic"
    assert out["config"]["grid_cells"] == 3
    assert out["config"]["n_tests"] == 300


@pytest.mark.timeout(600)
def test_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's scores as float .npy arrays,
    identical from run to run with the same arguments; --full is accepted
    and leaves the result line's meaning unchanged."""
    import numpy as np

    common = ("--backend", "ref", "--cells", "1", "--n-tests", "300",
              "--warmup", "0")
    a = _run_bench(*common, "--steps", "1",
                   "--dump-outputs", str(tmp_path / "a"))
    b = _run_bench(*common, "--steps", "1", "--full",
                   "--dump-outputs", str(tmp_path / "b"))
    assert a["steps"] == 1 and b["steps"] == 1
    # value and ms_per_step describe the same timed steps
    assert a["value"] == pytest.approx(1000.0 / a["ms_per_step"])
    assert REQUIRED_KEYS <= set(b)
    assert a["metric"] == b["metric"] and a["unit"] == b["unit"]

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["scores_counts.npy", "scores_prf.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    n_proj = len(make_synthetic_tests(n_tests=300, seed=0))
    for name in names:
        xa = np.load(tmp_path / "a" / name)
        xb = np.load(tmp_path / "b" / name)
        assert xa.dtype in (np.float32, np.float64)
        assert xa.shape == (1, n_proj + 1, 3)
        np.testing.assert_array_equal(xa, xb)
    counts = np.load(tmp_path / "a" / "scores_counts.npy")
    # the totals row is the sum of the per-project rows
    np.testing.assert_array_equal(counts[:, -1], counts[:, :-1].sum(axis=1))
    assert counts.sum() > 0


@pytest.mark.timeout(600)
def test_self_launch_two_ranks():
    """--gpus 2 with no torchrun env must self-launch 2 ranks (gloo on
    CPU) and report n_gpus=2 — the SCALE-run contract."""
    out = _run_bench("--gpus", "2", "--backend", "ref", "--cells", "3",
                     "--n-tests", "300", "--steps", "1", "--warmup", "0")
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"].startswith("cell-sharded dp2")


@pytest.mark.timeout(600)
def test_shap_stage_contract():
    out = _run_bench("--stage", "shap", "--backend", "ref", "--n-tests",
                     "120", "--steps", "1", "--warmup", "0")
    assert REQUIRED_KEYS <= set(out)
    assert out["metric"].startswith("shap-configs/sec")
    assert len(out["config"]["shap_configs"]) == 2
