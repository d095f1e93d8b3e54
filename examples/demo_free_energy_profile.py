"""The free-energy profile of a temperature ladder along a coordinate: the double well of demo_ladder_free_energy.py,
E = 4 (x^2 - 1)^2, sampled by parallel tempering with x of every chain recorded next to its energy.  MBAR
(``free_energy_profile``, on the GPU; the samples never leave it) turns the eight rungs into the reweighted histogram p(x; T)
on 40 bins and F(x; T) = -T ln p(x; T) at three temperatures -- a cold one at which the plain samples of that temperature alone
hardly ever see the barrier, one in between and a hot one -- printed next to the exact profile of the same bins,
-T ln (integral over the bin of exp(-E / T) dx / (width Z(T))) = 4 (x^2 - 1)^2 + T ln Z(T) averaged over the bin, from a
numerical quadrature.  ``free_energy_profile_uncertainties`` adds the asymptotic standard error of every F(x; T), printed as
+-, and the covariance of the bins, from which the error bar of the barrier height F(0) - F(well) follows: the two values
come from the same samples, so their errors do not simply add in quadrature.

    python examples/demo_free_energy_profile.py [--quick]        (needs an MI355X and the built library)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metropolisengine_amd as me  # noqa: E402
from demo_parallel_tempering import BARRIER, LADDER, double_well  # noqa: E402

EDGES = np.linspace(-2.0, 2.0, 41)
TEMPS = np.array([0.25, 0.8, 2.5])
QUICK = dict(chains_per_rung=256, burn_in=100, n_records=16)


def quadrature(edges, temps, half_width=4.0, per_bin=2000):
    """The exact F of every bin, ``(len(temps), bins)``: -T ln of the bin's share of Z(T) per unit width, by the trapezoidal
    rule (``per_bin`` intervals per bin; Z on [-4, 4], beyond which the integrand is below exp(-200) at these temperatures)."""
    def integral(lo, hi, t, n):
        x = np.linspace(lo, hi, n + 1)
        y = np.exp(-BARRIER * (x * x - 1.0) ** 2 / t)
        return (y.sum() - 0.5 * (y[0] + y[-1])) * (x[1] - x[0])
    out = np.empty((len(temps), len(edges) - 1))
    for i, t in enumerate(temps):
        z = integral(-half_width, half_width, t, 400000)
        for b in range(len(edges) - 1):
            out[i, b] = -t * np.log(integral(edges[b], edges[b + 1], t, per_bin) / ((edges[b + 1] - edges[b]) * z))
    return out


def sample(chains_per_rung=4096, burn_in=600, n_records=64, sweeps=5, rounds_per_record=2, seed=7):
    """Parallel tempering with recording, as in demo_reweight_observables.py, with the coordinate itself.  Returns the engine."""
    engine = me.MetropolisEngine(double_well, None, [-1.0], None, n_chains=chains_per_rung * LADDER.size, seed=seed,
                                 temperatures=LADDER, dtype="f64")
    for _ in range(burn_in):
        engine.step_all(sweeps)
        engine.replica_exchange()
    engine.record_energies(n_records)
    engine.record_observables(["real_0"])
    for _ in range(n_records):
        for _ in range(rounds_per_record):
            engine.step_all(sweeps)
            engine.replica_exchange()
        engine.record_energy()
    return engine


def barrier_height(out, i):
    """``(height, error, bin of the barrier top, bin of the well)`` at temperature ``i``: F of the bin left of x = 0 minus F of
    the bin of largest density, and its standard error ``T sqrt(C_tt + C_ww - 2 C_tw)`` from ``C = log_mass_cov[i]``."""
    top, well = int(np.searchsorted(out["edges"], 0.0)) - 1, int(out["lowest"][i])
    c = out["log_mass_cov"][i]
    height = out["free_energy"][i, top] - out["free_energy"][i, well]
    return height, out["temps"][i] * np.sqrt(max(c[top, top] + c[well, well] - 2.0 * c[top, well], 0.0)), top, well


def main(temps=TEMPS, edges=EDGES, **kw):
    engine = sample(**kw)
    out = engine.free_energy_profile_uncertainties("real_0", edges, temps)
    exact = quadrature(out["edges"], out["temps"])
    print("samples %d, outside the bins: %s; neff_fraction %s" % (out["counts"].sum() + out["counts_outside"].sum(),
                                                                 out["counts_outside"].tolist(), np.round(out["neff_fraction"], 4)))
    print("      x    samples" + "".join("   F(x; %.2f): MBAR    +-       exact" % t for t in out["temps"]))
    for b, x in enumerate(out["centers"]):
        print("%7.3f   %8d" % (x, out["counts"][b]) +
              "".join("   %17.4f  %6.4f  %8.4f" % (out["free_energy"][i, b], out["d_free_energy"][i, b], exact[i, b])
                      for i in range(len(out["temps"]))))
    for i, t in enumerate(out["temps"]):
        height, error, top, well = barrier_height(out, i)
        print("T = %.2f: barrier height F(%.2f) - F(%.2f) = %.4f +- %.4f (exact %.4f); errors of the two bins alone %.4f and %.4f"
              % (t, out["centers"][top], out["centers"][well], height, error, exact[i, top] - exact[i, well],
                 out["d_free_energy"][i, top], out["d_free_energy"][i, well]))
    return {"result": out, "exact": exact, "engine": engine}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small run: 8 x 256 chains, 16 records")
    cli = ap.parse_args()
    main(**(QUICK if cli.quick else {}))
