"""bench.py from the command line on one GPU: a plain run prints the headline figure and runs nothing else; --full adds
every side block.  Small step counts and chain counts -- these check the shape of the line, not its numbers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_BLOCKS = ("cpu_baseline", "cpu_baseline_c", "fused", "roofline_hbm", "f32", "other_configs", "acceptance_rate",
               "pooled_variance_mean")


def _bench(*options):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(options), cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1, "stdout carries exactly the JSON line"
    return json.loads(lines[0])


def _check_headline(line, steps, warmup):
    assert line["metric"] == "MC steps/sec (chains x sweeps) at 2^20 chains, 16 params"
    assert line["unit"] == "chain-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (steps, warmup, 1)
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = chains x steps / wall and ms_per_step = wall / steps describe the same timed region
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(line["config"]["chains_per_gpu"], rel=1e-9)
    assert line["roofline"]["kernel_ms"] > 0


def test_plain_run_is_the_headline_alone(tmp_path):
    line = _bench("--steps", "40", "--warmup", "10", "--dump-outputs", str(tmp_path / "out"))
    _check_headline(line, 40, 10)
    assert line["full"] is False
    assert all(line[name] is None for name in SIDE_BLOCKS)
    assert line["multi_gpu"]["pooled_chains"] is None and line["multi_gpu"]["rccl_version"] is None
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == ["accept_stats.npy", "chain_index.npy", "energy.npy", "real_params.npy", "sampling_width.npy"]
    accepted, proposed = np.load(tmp_path / "out" / "accept_stats.npy")
    assert proposed == 50 * (1 << 20) and 0 < accepted < proposed


def test_full_run_adds_every_side_block():
    line = _bench("--steps", "40", "--warmup", "10", "--chains-log2", "16", "--full", "--cpu-seconds", "0.5",
                  "--hbm-chains-log2", "18", "--fused-sweeps", "4")
    _check_headline(line, 40, 10)
    assert line["full"] is True
    assert all(line[name] is not None for name in SIDE_BLOCKS)
    assert line["cpu_baseline"]["value"] > 0 and line["fused"]["value"] > 0 and line["f32"]["value"] > 0
    assert line["roofline_hbm"]["value"] > 0
    assert not any("error" in (block or {}) for block in line["other_configs"].values()), line["other_configs"]
    assert line["multi_gpu"]["pooled_chains"] == 1 << 16 and line["multi_gpu"]["ranks_seen_by_pooled_allreduce"] == 1
    assert 0.0 < line["acceptance_rate"] < 1.0
