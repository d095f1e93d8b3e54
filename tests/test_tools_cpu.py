"""Host-side checks of the dev tools that guard the numbers (no GPU)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(headline, cycle):
    return json.dumps({"value": headline, "other_configs": {"config3_cycle_f64": {"chain_steps_per_s": cycle, "acceptance_rate": 0.3}},
                       "fused": None})


def test_compare_bench_flags_a_fallen_throughput(tmp_path):
    old, same, fallen = tmp_path / "old.json", tmp_path / "same.json", tmp_path / "fallen.json"
    old.write_text("banner on stdout\n" + _line(2.0e10, 3.0e10) + "\n")
    same.write_text(_line(1.98e10, 3.05e10) + "\n")
    fallen.write_text(_line(2.0e10, 1.9e10) + "\n")       # what round 3's closing bench line showed after an energy-functor change
    tool = os.path.join(ROOT, "tools", "compare_bench.py")
    ok = subprocess.run([sys.executable, tool, str(old), str(same)], capture_output=True, text=True)
    assert ok.returncode == 0 and "config3_cycle_f64.chain_steps_per_s" in ok.stdout
    bad = subprocess.run([sys.executable, tool, str(old), str(fallen)], capture_output=True, text=True)
    assert bad.returncode == 1 and "<-- fell" in bad.stdout


def test_compare_bench_reads_a_plain_line(tmp_path):
    """A plain bench line (no --full) carries null side blocks: only the headline is compared."""
    old, new = tmp_path / "old.json", tmp_path / "new.json"
    old.write_text(json.dumps({"value": 2.0e10, "other_configs": None, "fused": None}) + "\n")
    new.write_text(json.dumps({"value": 1.5e10, "other_configs": None, "fused": None}) + "\n")
    tool = os.path.join(ROOT, "tools", "compare_bench.py")
    ok = subprocess.run([sys.executable, tool, str(old), str(old)], capture_output=True, text=True)
    assert ok.returncode == 0 and "headline" in ok.stdout
    bad = subprocess.run([sys.executable, tool, str(old), str(new)], capture_output=True, text=True)
    assert bad.returncode == 1 and "<-- fell" in bad.stdout


def test_bench_side_measurements_need_full():
    """bench.py without --full runs no side measurement, whatever the side options say; --full keeps their defaults and
    honours each of them.  The headline options are untouched by it."""
    import bench
    side = ("cpu_seconds", "fused_sweeps", "hbm_chains_log2", "extras")
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not plain.full and all(getattr(plain, name) == 0 for name in side)
    forced = bench.parse_args(["--cpu-seconds", "5", "--fused-sweeps", "8", "--extras", "1", "--hbm-chains-log2", "22"])
    assert not forced.full and all(getattr(forced, name) == 0 for name in side)
    full = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    assert full.full and (full.cpu_seconds, full.fused_sweeps, full.hbm_chains_log2, full.extras) == (12.0, 32, 22, 1)
    chosen = bench.parse_args(["--full", "--cpu-seconds", "0", "--fused-sweeps", "4"])
    assert (chosen.cpu_seconds, chosen.fused_sweeps, chosen.hbm_chains_log2, chosen.extras) == (0.0, 4, 22, 1)
    for args in (plain, full):
        assert (args.gpus, args.steps, args.warmup, args.dtype, args.sweeps, args.chains_log2) == (1, 7, 3, "f64", 1, 20)


def test_host_units_are_named_once():
    """build.HOST_UNITS names every csrc/*.hip but me_kernels.hip, and tools/build_variant.sh takes its units from that list: it
    spells out none of them itself (a hand-kept second list once missed two new units and its variants stopped linking)."""
    import re
    from metropolisengine_amd import build
    units = [name for name, _ in build.HOST_UNITS]
    on_disk = sorted(f[:-len(".hip")] for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(units + ["me_kernels"]) == on_disk and len(set(units)) == len(units)
    assert dict(build.HOST_UNITS)["me_population"] == ["-ffp-contract=off"]
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as fh:
        script = fh.read()
    assert "build.HOST_UNITS" in script
    assert set(re.findall(r"\bme_\w+", script)) == {"me_kernels"}
