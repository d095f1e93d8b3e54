"""Population annealing on the GPU engine: the double well E = h (x^2 - 1)^2 of demo_parallel_tempering.py, annealed from
T = 4 (where chains cross the barrier h = 4 freely) down to that demo's cold rung, T = 0.1, in geometric stages.  Every
stage resamples the population in proportion to its Boltzmann reweighting and then runs ordinary Metropolis sweeps at the
new temperature.  Both wells keep half the population on the way down, although at T = 0.1 local moves alone never
cross the barrier; the product of the stages' mean weights estimates ln Z(0.1) / Z(4), printed next to a numpy quadrature
of the integral of exp(-E / T) dx.

    python examples/demo_population_annealing.py        (needs an MI355X and the built library)
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metropolisengine_amd as me  # noqa: E402

# the same double well (and so the same prebuilt plugin) as the parallel-tempering example
_spec = importlib.util.spec_from_file_location("demo_parallel_tempering", os.path.join(HERE, "demo_parallel_tempering.py"))
_pt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_pt)
double_well = _pt.double_well
BARRIER = _pt.BARRIER

T_HOT = 4.0
T_COLD = float(_pt.LADDER[0])                # 0.1: barrier / T = 40
SCHEDULE = T_HOT * (T_COLD / T_HOT) ** (np.arange(1, 41) / 40.0)      # 40 geometric stages, ending at T_COLD


def log_z_quadrature(t_old, t_new, lo=-4.0, hi=4.0, n=400001):
    """ln Z(t_new) - ln Z(t_old), Z(T) = integral of exp(-E(x) / T) dx, on a uniform grid (the integrand vanishes at the
    ends: E(4) / T_HOT = 225)."""
    x = np.linspace(lo, hi, n)
    e = BARRIER * (x * x - 1.0) ** 2

    def log_z(t):
        a = -e / t
        m = a.max()
        y = np.exp(a - m)
        return m + np.log((x[1] - x[0]) * (y.sum() - 0.5 * (y[0] + y[-1])))     # trapezoid rule

    return log_z(t_new) - log_z(t_old)


def run(anneal=True, n_chains=1 << 16, equilibrate=1000, sweeps=10, seed=11, dtype="f64"):
    """Every chain starts at x = -1.  With ``anneal``: ``equilibrate`` sweeps at T_HOT with proposals of width 1 (the
    population must start from the Boltzmann law at T_HOT), then the schedule (resample + ``sweeps`` sweeps per stage).
    Without: the same number of sweeps, all of them at T_COLD with local moves (the default width).  Returns the engine."""
    engine = me.MetropolisEngine(double_well, None, [-1.0], None, 1.0 if anneal else 0.05, n_chains=n_chains, seed=seed,
                                 dtype=dtype, temp=T_HOT if anneal else T_COLD)
    engine.step_all(equilibrate)
    if anneal:
        engine.anneal(SCHEDULE, n_sweeps=sweeps)
    else:
        engine.step_all(sweeps * SCHEDULE.size)
    return engine


def right_well_fraction(engine):
    return float(np.mean(engine.real_params[:, 0] > 0))


def main(**kw):
    annealed, cold = run(True, **kw), run(False, **kw)
    stats = annealed.population_stats()
    print("population annealing %g -> %g in %d stages: fraction at x > 0 = %.4f, %d families survive"
          % (T_HOT, T_COLD, stats["stages"], right_well_fraction(annealed), annealed.n_families()))
    print("stepped at T = %g only:              fraction at x > 0 = %.4f" % (T_COLD, right_well_fraction(cold)))
    print("ln Z(%g) / Z(%g): population annealing %.4f, quadrature %.4f (smallest neff fraction %.3f)"
          % (T_COLD, T_HOT, stats["log_z"][-1], log_z_quadrature(T_HOT, T_COLD), stats["neff_fraction"].min()))
    return annealed, cold


if __name__ == "__main__":
    main()
