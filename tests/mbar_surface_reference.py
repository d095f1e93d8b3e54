"""numpy restatement of the joint reweighted histogram along two quantities (metropolisengine_amd/csrc/me_mbar_hist2d.hip) and
exact samples of (x_0, x_1) under E = |x|^2 (test infrastructure shared by test_mbar_surface_cpu.py and
test_gpu_mbar_surface.py).

The slot of a sample along an axis is tests/mbar_profile_reference.py's, the log weights are tests/mbar_reference.py's, and a
cell's mass is one pairwise sum of the normalised weights per cell in ``dtype`` (``np.longdouble``: the yardstick of the
device's float64), the same way as ``mbar_profile_reference.histogram``.
"""
import numpy as np

from mbar_reference import _log_weights, used
from mbar_observables_reference import LADDER8, PHYSICS_PER_RUNG, PHYSICS_SUBSETS
from mbar_profile_reference import exact_x0_masses, slots

SURFACE_EDGES_X = np.linspace(-1.5, 1.5, 5)
SURFACE_EDGES_Y = np.array([-1.2, -0.3, 0.2, 0.9, 1.6])


def histogram2d(energies, rungs, temps, f, targets, values_x, edges_x, values_y, edges_y, dtype=np.float64):
    """``(mass (T, Bx + 3, By + 3), counts (Bx + 3, By + 3) int64, neff_fraction (T,))``: per cell ``(slot_x, slot_y)`` the
    sum of the weights normalised over the used samples, and the number of used samples.  A sample is used when its energy is
    finite."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, n_k = used(energies, rungs, temps.size)
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    sx, sy = len(edges_x) + 2, len(edges_y) + 2
    cell = slots(np.asarray(values_x, dtype=np.float64).ravel()[ok], edges_x) * sy + \
        slots(np.asarray(values_y, dtype=np.float64).ravel()[ok], edges_y)
    d = np.empty(e.size, dtype=dtype)
    for i in range(0, e.size, 1 << 18):         # (in slices: the K columns of 2^22 long doubles would take gigabytes)
        _, m, s = _log_weights(e[i:i + (1 << 18)], temps, n_k, f, dtype)
        d[i:i + (1 << 18)] = m + np.log(s)
    targets = np.asarray(targets, dtype=dtype)
    mass = np.zeros((targets.size, sx * sy), dtype=dtype)
    neff = np.zeros(targets.size, dtype=dtype)
    order = np.argsort(cell, kind="stable")     # the samples of a cell side by side, in their own order
    sorted_cells = cell[order]
    seen, starts = np.unique(sorted_cells, return_index=True)
    ends = np.append(starts[1:], sorted_cells.size)
    for i, t in enumerate(targets):
        l = -e / t - d
        w = np.exp(l - l.max())
        sw = w.sum()
        w_sorted = (w / sw)[order]
        for c, lo, hi in zip(seen, starts, ends):
            mass[i, c] = w_sorted[lo:hi].sum()          # (np.bincount would narrow long double weights to float64)
        neff[i] = sw * sw / (e.size * (w * w).sum())
    counts = np.bincount(cell, minlength=sx * sy).astype(np.int64)
    return mass.reshape(targets.size, sx, sy), counts.reshape(sx, sy), neff


def xy_quadratic_subsets(seed=53, dim=4, a=1.0, temps=LADDER8, n_subsets=PHYSICS_SUBSETS, per_rung=PHYSICS_PER_RUNG):
    """mbar_observables_reference.iso_quadratic_subsets' generator with the columns ``x_0`` and ``x_1``: independent subsets
    of exact samples of E = a |x|^2 in ``dim`` real dimensions, per subset and rung ``per_rung`` configurations x ~ N(0, T_k /
    2a).  Returns a list of ``(energies [n], rungs [n], columns [2, n])``, n = K per_rung."""
    rng = np.random.default_rng(seed)
    temps = np.asarray(temps, dtype=np.float64)
    rungs = np.repeat(np.arange(temps.size), per_rung).astype(np.int32)
    out = []
    for _ in range(n_subsets):
        x = rng.standard_normal((temps.size * per_rung, dim)) * np.sqrt(temps[rungs] / (2 * a))[:, None]
        out.append((a * (x * x).sum(axis=1), rungs, np.stack([x[:, 0], x[:, 1]])))
    return out


def physics_masses(results, targets, edges_x=SURFACE_EDGES_X, edges_y=SURFACE_EDGES_Y):
    """From per-subset tables ``(T, Bx + 3, By + 3)``: ``(estimates [subsets, T, Bx + 2, By + 2], exact [T, Bx + 2, By + 2])``
    -- the bins, below and above on both axes; x_0 and x_1 are independent, so the exact mass of a cell is the product of
    mbar_profile_reference.exact_x0_masses per axis."""
    bx, by = len(edges_x) - 1, len(edges_y) - 1
    est = np.array([np.asarray(m, dtype=np.float64)[:, :bx + 2, :by + 2] for m in results])
    exact = np.array([np.outer(exact_x0_masses(edges_x, t), exact_x0_masses(edges_y, t)) for t in targets])
    return est, exact
