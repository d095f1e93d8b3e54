"""Honest MBAR error bars from the records themselves: the double-well ladder of demo_ladder_free_energy.py, recorded a few
sweeps apart.  Successive records of a Metropolis chain are correlated, so error bars that take them as independent are too
small by sqrt(g), g the statistical inefficiency of the recorded series.  ``recorded_inefficiency`` estimates g per rung on
the GPU, pooled over the chains of the rung (the stores stay on the device), and ``inefficiency="recorded"`` hands the largest
g over the rungs to the error bars.

    python examples/demo_recorded_inefficiency.py        (needs an MI355X and the built library)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from demo_ladder_free_energy import quadrature, sample  # noqa: E402


def main(**kw):
    engine = sample(**kw)
    engine_temps = engine.temperatures
    out = engine.recorded_inefficiency()
    print("%d records of %d chains per rung; statistical inefficiency g of the energy series and where its walk stopped"
          % (out["n_records"], out["chains_used"][0, 0]))
    print("     T        g    tau   stop lag")
    for k, t in enumerate(engine_temps):
        print("%6.3f   %6.2f  %5.2f   %8d" % (t, out["g"][0, k], out["tau"][0, k], out["stop_lag"][0, k]))
    f = engine.ladder_free_energies()["f"]
    plain = engine.ladder_free_energy_uncertainties(f)
    honest = engine.ladder_free_energy_uncertainties(f, inefficiency="recorded")
    exact = quadrature(engine_temps)[0]
    exact_f = -(exact - exact[0])
    print("\nf[k] = -ln Z(T_k) / Z(T_0), its error bar with inefficiency = 1 and with \"recorded\" (g = %.2f), and the deviation "
          "from a quadrature in units of each" % out["g"][0].max())
    print("     T          f     quadrature    d_f (1)   z (1)    d_f (recorded)   z (recorded)")
    for k, t in enumerate(engine_temps):
        dev = f[k] - exact_f[k]
        z = ["%6.2f" % (dev / s[k]) if s[k] > 0 else "     -" for s in (plain["d_f"], honest["d_f"])]
        print("%6.3f   %9.5f   %9.5f   %9.5f  %s   %9.5f        %s" % (t, f[k], exact_f[k], plain["d_f"][k], z[0], honest["d_f"][k], z[1]))
    return {"inefficiency": out, "f": f, "exact_f": exact_f, "d_f": plain["d_f"], "d_f_recorded": honest["d_f"], "engine": engine}


if __name__ == "__main__":
    main()
