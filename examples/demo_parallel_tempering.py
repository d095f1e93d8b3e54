"""Parallel tempering on the GPU engine: a one-parameter double well E = h (x^2 - 1)^2, written as the reference writes its
energies (a Python callable, traced into a device plugin), on a geometric temperature ladder.  The barrier at x = 0 is
h = 4, forty times the coldest temperature: local moves alone leave every cold chain in the well it started in (x = -1);
with replica-exchange swaps between neighbouring rungs, configurations that crossed the barrier at the hot end travel
down the ladder and the cold rung populates both wells equally.

    python examples/demo_parallel_tempering.py        (needs an MI355X and the built library)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import metropolisengine_amd as me  # noqa: E402

BARRIER = 4.0
LADDER = 0.1 * 1.8 ** np.arange(8)          # 0.1 ... 4.1: barrier / T_0 = 40, the hottest rung crosses freely


def double_well(real_params, complex_params):
    return BARRIER * (real_params[0] ** 2 - 1.0) ** 2


def run(swaps, chains_per_rung=4096, n_iterations=600, sweeps=5, seed=7):
    """Every chain starts at x = -1; ``n_iterations`` x (``sweeps`` sweeps [+ one swap round]).  Returns the engine."""
    engine = me.MetropolisEngine(double_well, None, [-1.0], None, n_chains=chains_per_rung * LADDER.size, seed=seed,
                                 temperatures=LADDER)
    for _ in range(n_iterations):
        engine.step_all(sweeps)
        if swaps:
            engine.replica_exchange()
    return engine


def right_well_fraction(engine):
    """Per rung: the fraction of its chains at x > 0."""
    x = engine.real_params[:, 0]
    return (x > 0).reshape(engine.temperatures.size, -1).mean(axis=1)


def main(**kw):
    with_swaps, without = run(True, **kw), run(False, **kw)
    for name, engine in (("with swaps", with_swaps), ("local moves only", without)):
        print("%-16s fraction at x > 0 per rung: %s" % (name, np.array2string(right_well_fraction(engine), precision=3)))
    print("swap acceptance per pair of rungs: %s" % np.array2string(with_swaps.swap_acceptance(), precision=3))
    return with_swaps, without


if __name__ == "__main__":
    main()
