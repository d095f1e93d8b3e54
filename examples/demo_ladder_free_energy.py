"""Free energies and the heat capacity of a temperature ladder: the double well of demo_parallel_tempering.py,
E = 4 (x^2 - 1)^2, sampled by parallel tempering with the energy of every chain recorded between swap rounds.  MBAR
(``ladder_free_energies`` / ``reweight``, solved on the GPU) combines the eight rungs into ln Z(T) / Z(T_max) and
C(T) = Var E / T^2 on a fine temperature grid, printed next to a numerical quadrature of
Z(T) = integral exp(-4 (x^2 - 1)^2 / T) dx; the last column is C(T) of all samples with its asymptotic standard error
(``fluctuation_uncertainties``).

A swap pairs slot j of rung k with slot j of rung k+1, so the sixteen sub-ensembles {slots with j mod 16 = s} never
exchange anything: sixteen independent estimates, whose spread is the error bar printed.

    python examples/demo_ladder_free_energy.py        (needs an MI355X and the built library)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metropolisengine_amd as me  # noqa: E402
from metropolisengine_amd import statistics  # noqa: E402
from demo_parallel_tempering import BARRIER, LADDER, double_well  # noqa: E402

N_SUBSETS = 16


def quadrature(temps, half_width=4.0, n=400001):
    """``(ln Z, <E>, Var E)`` of the double well at every temperature, by the trapezoidal rule on [-4, 4] (the integrand is
    below exp(-200) at the ends for every temperature used here)."""
    x = np.linspace(-half_width, half_width, n)
    trapz = lambda y: (y.sum() - 0.5 * (y[0] + y[-1])) * (x[1] - x[0])      # noqa: E731
    e = BARRIER * (x * x - 1.0) ** 2
    out = np.empty((3, len(temps)))
    for i, t in enumerate(temps):
        w = np.exp(-e / t)
        z = trapz(w)
        mean = trapz(w * e) / z
        out[:, i] = np.log(z), mean, trapz(w * (e - mean) ** 2) / z
    return out


def sample(chains_per_rung=4096, burn_in=600, n_records=64, sweeps=5, rounds_per_record=2, seed=7):
    """Parallel tempering with recording: ``burn_in`` x (``sweeps`` sweeps + one swap round), then ``n_records`` records
    ``rounds_per_record`` such rounds apart.  Returns the engine."""
    engine = me.MetropolisEngine(double_well, None, [-1.0], None, n_chains=chains_per_rung * LADDER.size, seed=seed,
                                 temperatures=LADDER, dtype="f64")
    for _ in range(burn_in):
        engine.step_all(sweeps)
        engine.replica_exchange()
    engine.record_energies(n_records)
    for _ in range(n_records):
        for _ in range(rounds_per_record):
            engine.step_all(sweeps)
            engine.replica_exchange()
        engine.record_energy()
    return engine


def subset_estimates(engine, grid):
    """MBAR on each of the independent sub-ensembles: ``(ln Z(T)/Z(T_max), C(T))`` as ``(N_SUBSETS, len(grid))`` arrays."""
    temps = engine.temperatures
    m = engine.n_chains // temps.size
    energies = engine.energy_samples().reshape(-1, temps.size, m)            # [record][rung][slot]
    ln_z, heat = [], []
    for s in range(N_SUBSETS):
        sub = energies[:, :, s::N_SUBSETS]
        rungs = np.broadcast_to(np.arange(temps.size)[None, :, None], sub.shape)
        f = statistics.mbar_free_energies(sub, rungs, temps)["f"]
        out = statistics.mbar_reweight(sub, rungs, temps, f, np.append(grid, temps[-1]))
        ln_z.append(out["ln_z"][:-1] - out["ln_z"][-1])
        heat.append(out["heat_capacity"][:-1])
    return np.array(ln_z), np.array(heat)


def asymptotic_sigma(engine, grid):
    """The asymptotic standard error of ``ln Z(T) / Z(T_max)`` on ``grid`` from ALL samples in one further pass
    (``statistics.mbar_uncertainties``).  The errors are relative to rung 0, so the ladder is handed over hottest rung first.
    The formula takes the samples as independent; records a few sweeps apart are not, so this is a lower bound here."""
    temps = engine.temperatures
    energies = engine.energy_samples()
    rungs = np.tile(np.repeat(np.arange(temps.size), engine.n_chains // temps.size), energies.shape[0])
    f = engine.ladder_free_energies()["f"]
    out = statistics.mbar_uncertainties(energies, temps.size - 1 - rungs, temps[::-1], (f - f[-1])[::-1], targets=grid)
    return out["d_ln_z"]


def main(grid=None, **kw):
    engine = sample(**kw)
    temps = engine.temperatures
    grid = np.geomspace(temps[0], temps[-1], 22) if grid is None else np.asarray(grid, dtype=np.float64)
    whole = engine.reweight(grid, engine.ladder_free_energies()["f"])
    ln_z, heat = subset_estimates(engine, grid)
    sigma = asymptotic_sigma(engine, grid)
    # the asymptotic error of C(T) from ALL samples, taken as independent like sigma: beside the se of the sub-ensembles' mean
    heat_sigma = engine.fluctuation_uncertainties(grid, engine.ladder_free_energies()["f"])["d_heat_capacity"]
    exact = quadrature(np.append(grid, temps[-1]))
    exact_ln_z, exact_heat = exact[0, :-1] - exact[0, -1], exact[2, :-1] / grid ** 2
    se = lambda a: a.std(axis=0, ddof=1) / np.sqrt(a.shape[0])      # noqa: E731
    print("asymptotic sigma ", end="")       # of ln Z(T)/Z(T_max), from all samples taken as independent: beside the se
    print("     T   ln Z(T)/Z(T_max): MBAR +- se   quadrature      C(T): MBAR +- se   quadrature   neff   C(T) of all samples +- sigma")
    for i, t in enumerate(grid):
        print("     %.5f     " % sigma[i], end="")
        print("%6.3f   %10.5f +- %.5f   %10.5f       %8.5f +- %.5f   %8.5f   %6.4f   %8.5f +- %.5f"
              % (t, ln_z[:, i].mean(), se(ln_z)[i], exact_ln_z[i], heat[:, i].mean(), se(heat)[i], exact_heat[i],
                 whole["neff_fraction"][i], whole["heat_capacity"][i], heat_sigma[i]))
    return {"temps": grid, "ln_z": ln_z, "heat_capacity": heat, "exact_ln_z": exact_ln_z, "exact_heat_capacity": exact_heat,
            "engine": engine}


if __name__ == "__main__":
    main()
