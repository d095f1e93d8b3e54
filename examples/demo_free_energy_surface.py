"""The free-energy SURFACE of a temperature ladder over two coordinates: a two-parameter double well whose minima at (x, y) =
(-1, 1/2) and (1, 1/2) are joined by a curved valley y = x^2 / 2 through the saddle at the origin,
E = 4 (x^2 - 1)^2 + 4 (y - x^2 / 2)^2, sampled by parallel tempering with x and y of every chain recorded next to its energy.
MBAR (``free_energy_surface``, on the GPU; the samples never leave it) turns the eight rungs into the joint reweighted
histogram p(x, y; T) on 13 x 9 bins and F(x, y; T) = -T ln p(x, y; T); ``free_energy_surface_uncertainties`` adds the
asymptotic standard error of every cell and of the saddle height, a difference of two cells of the same correlated samples.
Neither the path between the wells nor the saddle follows from the two 1-D profiles: the valley is curved.  The surface is
printed at the coldest of three temperatures, at which the plain samples of that temperature alone hardly ever see the
saddle, next to the exact value of every cell, -T ln (integral over the cell of exp(-E / T) dx dy / (area Z(T))), from a
numerical quadrature.

    python examples/demo_free_energy_surface.py [--quick]        (needs an MI355X and the built library)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metropolisengine_amd as me  # noqa: E402
from demo_parallel_tempering import LADDER  # noqa: E402

EDGES_X = np.linspace(-1.625, 1.625, 14)        # 13 bins of 0.25 centred on -1.5 ... 1.5: the wells, the saddle
EDGES_Y = np.linspace(-0.625, 1.625, 10)        # 9 bins of 0.25 centred on -0.5 ... 1.5
TEMPS = np.array([0.25, 0.8, 2.5])
QUICK = dict(chains_per_rung=256, burn_in=100, n_records=16)
WELL, SADDLE = (1.0, 0.5), (0.0, 0.0)


def valley_well(real_params, complex_params):
    x, y = real_params[0], real_params[1]
    return 4.0 * (x * x - 1.0) ** 2 + 4.0 * (y - 0.5 * x * x) ** 2


def _integral(x_lo, x_hi, y_lo, y_hi, t, nx, ny):
    """The trapezoidal rule for exp(-E / T) on a rectangle, ``nx`` x ``ny`` intervals."""
    x, y = np.linspace(x_lo, x_hi, nx + 1), np.linspace(y_lo, y_hi, ny + 1)
    wx, wy = np.full(nx + 1, (x_hi - x_lo) / nx), np.full(ny + 1, (y_hi - y_lo) / ny)
    wx[[0, -1]] *= 0.5
    wy[[0, -1]] *= 0.5
    xx, yy = x[:, None], y[None, :]
    return float(wx @ np.exp(-(4.0 * (xx * xx - 1.0) ** 2 + 4.0 * (yy - 0.5 * xx * xx) ** 2) / t) @ wy)


def quadrature(edges_x, edges_y, t, per_cell=100):
    """The exact F of every cell at temperature ``t``, ``(Bx, By)``: -T ln of the cell's share of Z(T) per unit area (Z on [-3,
    3] x [-3, 7.5], beyond which the integrand is below exp(-60) up to T = 0.6)."""
    z = _integral(-3.0, 3.0, -3.0, 7.5, t, 1200, 2100)
    out = np.empty((len(edges_x) - 1, len(edges_y) - 1))
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            area = (edges_x[i + 1] - edges_x[i]) * (edges_y[j + 1] - edges_y[j])
            out[i, j] = -t * np.log(_integral(edges_x[i], edges_x[i + 1], edges_y[j], edges_y[j + 1], t, per_cell, per_cell) / (area * z))
    return out


def sample(chains_per_rung=2048, burn_in=400, n_records=64, sweeps=5, rounds_per_record=2, seed=7):
    """Parallel tempering with recording, as in demo_free_energy_profile.py, with both coordinates.  Returns the engine."""
    engine = me.MetropolisEngine(valley_well, None, [-1.0, 0.5], None, n_chains=chains_per_rung * LADDER.size, seed=seed,
                                 temperatures=LADDER, dtype="f64")
    for _ in range(burn_in):
        engine.step_all(sweeps)
        engine.replica_exchange()
    engine.record_energies(n_records)
    engine.record_observables(["real_0", "real_1"])
    for _ in range(n_records):
        for _ in range(rounds_per_record):
            engine.step_all(sweeps)
            engine.replica_exchange()
        engine.record_energy()
    return engine


def cell_of(out, point):
    """The indices of the inner cell that holds ``point = (x, y)``."""
    return (int(np.searchsorted(out["edges_x"], point[0], side="right")) - 1,
            int(np.searchsorted(out["edges_y"], point[1], side="right")) - 1)


def saddle_height(out, t):
    """``(height, error, saddle cell, well cell)`` at temperature index ``t`` of a result of
    ``free_energy_surface_uncertainties``: ``F(saddle) - F(right well)`` and its standard error from the covariance of the two
    log masses, ``T sqrt(C_ss + C_ww - 2 C_sw)`` (cell index ``bx * By + by``)."""
    saddle, well = cell_of(out, SADDLE), cell_of(out, WELL)
    by = out["edges_y"].size - 1
    s, w = saddle[0] * by + saddle[1], well[0] * by + well[1]
    c = out["log_mass_cov"][t]
    f = out["free_energy"][t]
    return f[saddle] - f[well], float(out["temps"][t]) * np.sqrt(max(c[s, s] + c[w, w] - 2.0 * c[s, w], 0.0)), saddle, well


def _grid(title, out, values, counts, least):
    print(title)
    print("     x \\ y" + "".join("%9.3f" % y for y in out["centers_y"]))
    for i, x in enumerate(out["centers_x"]):
        print("%10.3f" % x + "".join("%9.3f" % values[i, j] if counts[i, j] >= least else "        ." for j in range(values.shape[1])))


def main(temps=TEMPS, edges_x=EDGES_X, edges_y=EDGES_Y, least=20, **kw):
    engine = sample(**kw)
    out = engine.free_energy_surface("real_0", edges_x, "real_1", edges_y, temps)
    t = float(out["temps"][0])
    exact = quadrature(out["edges_x"], out["edges_y"], t)
    print("samples %d, of them outside the grid %d; mass outside the grid %s; neff_fraction %s"
          % (out["counts_slots"].sum(), out["counts_slots"].sum() - out["counts"].sum(), np.round(out["outside"], 5),
             np.round(out["neff_fraction"], 4)))
    seen = out["counts"] >= least
    _grid("F(x, y; %.2f) from MBAR (cells with at least %d samples of any rung)" % (t, least), out, out["free_energy"][0], out["counts"], least)
    _grid("F(x, y; %.2f) by quadrature" % t, out, exact, out["counts"], least)
    well, saddle = cell_of(out, WELL), cell_of(out, SADDLE)
    left = cell_of(out, (-WELL[0], WELL[1]))
    f = out["free_energy"][0]
    print("largest |MBAR - quadrature| over those %d cells: %.4f" % (seen.sum(), np.max(np.abs(f[seen] - exact[seen]))))
    print("T = %.2f: F(saddle) - F(right well) = %.4f, F(saddle) - F(left well) = %.4f; exact %.4f"
          % (t, f[saddle] - f[well], f[saddle] - f[left], exact[saddle] - exact[well]))
    # the same surface with its error bars (every key above is the same, bit for bit); the records are successive states of
    # Metropolis chains, so every variance carries the statistical inefficiency of the recorded series
    bars = engine.free_energy_surface_uncertainties("real_0", edges_x, "real_1", edges_y, temps, inefficiency="recorded")
    _grid("standard error of F(x, y; %.2f) (asymptotic MBAR covariance, recorded inefficiency)" % t, bars, bars["d_free_energy"][0],
          bars["counts"], least)
    height, error, _, _ = saddle_height(bars, 0)
    print("T = %.2f: F(saddle) - F(right well) = %.4f +- %.4f; exact %.4f, %.2f standard errors away"
          % (t, height, error, exact[saddle] - exact[well], (height - (exact[saddle] - exact[well])) / error))
    return {"result": out, "exact": exact, "engine": engine, "uncertainties": bars}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small run: 8 x 256 chains, 16 records")
    cli = ap.parse_args()
    main(**(QUICK if cli.quick else {}))
