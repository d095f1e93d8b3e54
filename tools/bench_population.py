"""GPU box: time one population-annealing stage (MetropolisEngine.resample) at 2^20 chains x 16 real parameters
(IsoQuadratic), float64 and float32: 100 stages between two waits for the engine's stream, after warm-up.  Prints microseconds
per stage and the bytes a stage must move over that time, one JSON line per dtype.

    python tools/bench_population.py [--chains N] [--dim D] [--stages K]

It also times single stages with a wait after each, an ordinary one and a steep one (T 2 -> 0.001 on energies ~
Gamma(8, 2)) whose weights collapse onto a few chains: the median of ten, with the stage's neff_fraction.

Bytes per stage: the weight and scan passes read the ledger twice; the gather reads x, the ledger rows and the family id
of every slot's ancestor and writes them to scratch; the copy back reads and writes them once more; the ancestor array
is written once and read once.  (Launch gaps and the one-block finalize are in the time, not in the bytes.)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metropolisengine_amd as me  # noqa: E402
from metropolisengine_amd import _capi  # noqa: E402


def stage_bytes(n, d, n_terms, esize):
    ledger = n * n_terms * esize
    moved = n * (d * esize + n_terms * esize + 8)          # x, ledger rows, family id
    return 2 * ledger + 2 * moved + 2 * moved + 2 * 4 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=16)
    ap.add_argument("--stages", type=int, default=100)
    args = ap.parse_args()
    for dtype, esize in (("f64", 8), ("f32", 4)):
        eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * args.dim, None, n_chains=args.chains, seed=1,
                                  dtype=dtype, temp=2.0)
        eng.step_all(20)
        # a schedule that barely moves: every stage does the full work whatever the weights
        temps = 2.0 * (1 - 1e-4) ** np.arange(1, 2 * args.stages + 11)
        for t in temps[:10]:
            eng.resample(t)
        eng.population_stats()                     # waits for the engine stream
        t0 = time.perf_counter()
        for t in temps[10:10 + args.stages]:
            eng.resample(t)
        eng.population_stats()
        dt = (time.perf_counter() - t0) / args.stages
        nbytes = stage_bytes(args.chains, args.dim, 1, esize)
        n_families = eng.n_families()
        # one stage at a time (a wait after each): an ordinary step, then a steep one whose weights collapse onto a few
        # chains, so that runs of up to all N slots go to one ancestor (the scan's longest writes)
        rng = np.random.default_rng(3)
        single = {}
        for name, t_new in (("ordinary", 1.9), ("collapsed", 1e-3)):
            times = []
            for _ in range(10):
                eng.set_temp(2.0)
                eng._set(_capi.FIELD_ENERGY, rng.gamma(8.0, 2.0, (args.chains, 1)))
                eng.population_stats()
                t1 = time.perf_counter()
                eng.resample(t_new)
                eng.population_stats()
                times.append(time.perf_counter() - t1)
            single[name] = {"us_per_stage": round(1e6 * float(np.median(times)), 2),
                            "neff_fraction": float(eng.population_stats()["neff_fraction"][-1]),
                            "n_families": eng.n_families()}
        print(json.dumps({"what": "population_resample", "dtype": dtype, "chains": args.chains, "dim": args.dim,
                          "single_stage_with_wait": single,
                          "stages": args.stages, "us_per_stage": round(dt * 1e6, 2), "bytes_per_stage": nbytes,
                          "achieved_TBps": round(nbytes / dt / 1e12, 3),
                          "n_families": n_families}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
