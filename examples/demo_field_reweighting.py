"""Reweighting in a FIELD from one zero-field run: the double well of demo_parallel_tempering.py, E = 4 (x^2 - 1)^2, sampled
by parallel tempering at zero field with x of every chain recorded next to its energy.  The recorded column is a possible
perturbation of the energy: ``reweight_perturbed`` (on the GPU; the samples never leave it) takes the eight rungs to the
states H = E - h x at any temperature and field, Ferrenberg-Swendsen reweighting in (T, h).  The field tilts the wells, so the
magnetisation <x>(h) leaves 0 and the susceptibility Var x / T falls as the weight gathers in one well.  Both are printed at
three fields next to a numerical quadrature, with ln Z(T, h) / Z(T, 0).

    python examples/demo_field_reweighting.py [--quick]        (needs an MI355X and the built library)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from demo_parallel_tempering import BARRIER  # noqa: E402
from demo_free_energy_profile import QUICK, sample  # noqa: E402

TEMP = 0.6
FIELDS = np.array([0.0, 0.15, 0.4])


def quadrature(t, h, half_width=4.0, n=200000):
    """``(ln Z(t, h) / Z(t, 0), <x>, Var x)`` of H = E - h x by the trapezoidal rule on [-half_width, half_width]."""
    x = np.linspace(-half_width, half_width, n + 1)
    e = BARRIER * (x * x - 1.0) ** 2
    w, w0 = np.exp(-(e - h * x) / t), np.exp(-e / t)
    w[[0, -1]] *= 0.5
    w0[[0, -1]] *= 0.5
    mean = (w * x).sum() / w.sum()
    return np.log(w.sum() / w0.sum()), mean, (w * (x - mean) ** 2).sum() / w.sum()


def main(temp=TEMP, fields=FIELDS, **kw):
    engine = sample(**kw)
    out = engine.reweight_perturbed(temp, {"real_0": -np.asarray(fields)})
    zero = out["ln_z"][int(np.argmin(np.abs(fields)))] if 0.0 in fields else engine.reweight([temp])["ln_z"][0]
    exact = np.array([quadrature(temp, h) for h in fields])
    print("samples %d at zero field, reweighted to T = %.2f; neff_fraction %s" % (engine.energy_samples().size, temp,
                                                                                 np.round(out["neff_fraction"], 4)))
    print("      h   ln Z(h)/Z(0): MBAR     exact    <x>: MBAR     exact   Var x / T: MBAR     exact")
    for i, h in enumerate(fields):
        print("%7.3f   %18.4f  %8.4f   %10.4f  %8.4f   %15.4f  %8.4f" % (h, out["ln_z"][i] - zero, exact[i, 0], out["mean"][i, 0],
                                                                      exact[i, 1], out["var"][i, 0] / temp, exact[i, 2] / temp))
    return {"result": out, "exact": exact, "engine": engine}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a small run: 8 x 256 chains, 16 records")
    cli = ap.parse_args()
    main(**(QUICK if cli.quick else {}))
