"""numpy restatement of the reweighted histogram along an observable (metropolisengine_amd/csrc/me_mbar_hist.hip) and the
exact bin probabilities of x_0 under E = a |x|^2 (test infrastructure shared by test_mbar_profile_cpu.py and
test_gpu_mbar_profile.py).

The masses are sums of the normalised weights per slot in ``dtype``: ``np.bincount`` in float64, one pairwise sum per slot in
``np.longdouble`` (the yardstick of the device's float64; ``np.bincount`` would narrow the weights).  The log weights are those
of tests/mbar_reference.py.
"""
import math

import numpy as np

from mbar_reference import _log_weights, used


def slots(values, edges):
    """The slot of every value for the ``B + 1`` ``edges``: bin ``b`` for ``edges[b] <= A < edges[b + 1]``, ``B`` below the
    first edge, ``B + 1`` at or above the last one, ``B + 2`` for NaN -- ``np.searchsorted(edges, A, side="right") - 1``."""
    a = np.asarray(values, dtype=np.float64).ravel()
    edges = np.asarray(edges, dtype=np.float64)
    b = edges.size - 1
    nan = np.isnan(a)
    pos = np.searchsorted(edges, np.where(nan, edges[0], a), side="right") - 1
    return np.where(nan, b + 2, np.where(pos < 0, b, np.where(pos >= b, b + 1, pos))).astype(np.int64)


def histogram(energies, rungs, temps, f, targets, values, edges, dtype=np.float64):
    """``(mass (T, B + 3), counts (B + 3,) int64, neff_fraction (T,))``: per slot the sum of the weights normalised over the
    used samples, and the number of used samples.  A sample is used when its energy is finite."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, n_k = used(energies, rungs, temps.size)
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    slot = slots(np.asarray(values, dtype=np.float64).ravel()[ok], edges)
    n_slots = len(edges) + 2
    d = np.empty(e.size, dtype=dtype)
    for i in range(0, e.size, 1 << 18):         # (in slices: the K columns of 2^22 long doubles would take gigabytes)
        _, m, s = _log_weights(e[i:i + (1 << 18)], temps, n_k, f, dtype)
        d[i:i + (1 << 18)] = m + np.log(s)
    targets = np.asarray(targets, dtype=dtype)
    mass = np.zeros((targets.size, n_slots), dtype=dtype)
    neff = np.zeros(targets.size, dtype=dtype)
    for i, t in enumerate(targets):
        l = -e / t - d
        w = np.exp(l - l.max())
        sw = w.sum()
        w_norm = w / sw
        if dtype is np.float64:
            mass[i] = np.bincount(slot, weights=w_norm, minlength=n_slots)
        else:                                   # (np.bincount would narrow long double weights to float64)
            for s in np.unique(slot):
                mass[i, s] = w_norm[slot == s].sum()
        neff[i] = sw * sw / (e.size * (w * w).sum())
    return mass, np.bincount(slot, minlength=n_slots).astype(np.int64), neff


def exact_x0_masses(edges, t, a=1.0):
    """Exact probabilities of x_0 under E = a |x|^2 at temperature ``t`` (x_0 ~ N(0, t / 2a), so P(x_0 < c) = (1 + erf(c /
    sqrt(t / a))) / 2): ``(B + 2,)`` = the B bins, then below the first edge and at or above the last one."""
    cdf = np.array([0.5 * (1.0 + math.erf(c / math.sqrt(t / a))) for c in np.asarray(edges, dtype=np.float64)])
    return np.concatenate([np.diff(cdf), [cdf[0], 1.0 - cdf[-1]]])


PROFILE_EDGES = np.linspace(-1.5, 1.5, 13)


def physics_masses(results, targets, edges=PROFILE_EDGES):
    """From per-subset masses ``(T, B + 3)``: ``(estimates [subsets, T, B + 2], exact [T, B + 2])`` -- the bins, below, above."""
    est = np.array([np.asarray(m, dtype=np.float64)[:, :len(edges) + 1] for m in results])
    return est, np.array([exact_x0_masses(edges, t) for t in targets])
