"""Observables of a temperature ladder on a fine temperature grid: the double well of demo_ladder_free_energy.py,
E = 4 (x^2 - 1)^2, sampled by parallel tempering with |x| and x^2 of every chain recorded next to its energy.  MBAR
(``reweight_observables``, on the GPU; the samples never leave it) turns the eight rungs into <|x|>(T), <x^2>(T) and their
temperature derivatives Cov(A, E) / T^2, printed next to a numerical quadrature; ``observable_uncertainties`` adds the
asymptotic standard error of every mean, scaled by the statistical inefficiency of the recorded series.

    python examples/demo_reweight_observables.py        (needs an MI355X and the built library)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metropolisengine_amd as me  # noqa: E402
from metropolisengine_amd import statistics  # noqa: E402
from demo_parallel_tempering import BARRIER, LADDER, double_well  # noqa: E402

WHICH = ("abs_real_0", "real_0_sq")


def quadrature(temps, half_width=4.0, n=400001):
    """``(<|x|>, <x^2>, d<|x|>/dT, d<x^2>/dT)`` of the double well at every temperature, by the trapezoidal rule on [-4, 4]."""
    x = np.linspace(-half_width, half_width, n)
    trapz = lambda y: (y.sum() - 0.5 * (y[0] + y[-1])) * (x[1] - x[0])      # noqa: E731
    e = BARRIER * (x * x - 1.0) ** 2
    out = np.empty((4, len(temps)))
    for i, t in enumerate(temps):
        w = np.exp(-e / t)
        z = trapz(w)
        mean_e = trapz(w * e) / z
        for j, a in enumerate((np.abs(x), x * x)):
            mean = trapz(w * a) / z
            out[j, i] = mean
            out[2 + j, i] = trapz(w * (a - mean) * (e - mean_e)) / z / t ** 2
    return out


def sample(chains_per_rung=4096, burn_in=600, n_records=64, sweeps=5, rounds_per_record=2, seed=7):
    """Parallel tempering with recording, as in demo_ladder_free_energy.py, plus the observables.  Returns the engine."""
    engine = me.MetropolisEngine(double_well, None, [-1.0], None, n_chains=chains_per_rung * LADDER.size, seed=seed,
                                 temperatures=LADDER, dtype="f64")
    for _ in range(burn_in):
        engine.step_all(sweeps)
        engine.replica_exchange()
    engine.record_energies(n_records)
    engine.record_observables(WHICH)                # after record_energies: one column per name, same capacity
    for _ in range(n_records):
        for _ in range(rounds_per_record):
            engine.step_all(sweeps)
            engine.replica_exchange()
        engine.record_energy()                      # the energy row and the observables' row of the same moment
    return engine


def main(grid=None, **kw):
    engine = sample(**kw)
    temps = engine.temperatures
    grid = np.geomspace(temps[0], temps[-1], 22) if grid is None else np.asarray(grid, dtype=np.float64)
    out = engine.reweight_observables(grid)
    exact = quadrature(grid)
    print("     T      <|x|>: MBAR  quadrature     <x^2>: MBAR  quadrature   d<|x|>/dT: MBAR  quadrature   d<x^2>/dT: MBAR  "
          "quadrature   neff")
    for i, t in enumerate(grid):
        print("%6.3f   %12.5f  %10.5f   %12.5f  %10.5f   %15.5f  %10.5f   %15.5f  %10.5f   %6.4f"
              % (t, out["mean"][i, 0], exact[0, i], out["mean"][i, 1], exact[1, i], out["dmean_dT"][i, 0], exact[2, i],
                 out["dmean_dT"][i, 1], exact[3, i], out["neff_fraction"][i]))
    # error bars: the asymptotic MBAR covariance assumes independent samples, and the records of a slot are correlated in
    # time, so every variance is scaled by the statistical inefficiency of the slot's series (the mean over 64 slots)
    series = engine.observable_samples()[:, :, ::max(1, engine.n_chains // 64)]
    g = [float(np.mean([statistics.statistical_inefficiency(series[:, q, c]) for c in range(series.shape[2])]))
         for q in range(len(WHICH))]
    bars = engine.observable_uncertainties(grid, f=None, inefficiency=g)
    print("statistical inefficiency of the recorded series: |x| %.2f, x^2 %.2f" % tuple(g))
    print("     T      <|x|>: MBAR +- error      quadrature     <x^2>: MBAR +- error      quadrature")
    for i, t in enumerate(grid):
        print("%6.3f   %12.5f ± %.5f  %10.5f   %12.5f ± %.5f  %10.5f"
              % (t, bars["mean"][i, 0], bars["d_mean"][i, 0], exact[0, i], bars["mean"][i, 1], bars["d_mean"][i, 1], exact[1, i]))
    return {"temps": grid, "result": out, "exact": exact, "engine": engine, "uncertainties": bars}


if __name__ == "__main__":
    main()
