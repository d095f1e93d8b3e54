"""numpy restatement of the Newton iteration for the ladder free energies of metropolisengine_amd/csrc/me_mbar_newton.hip
(test infrastructure; this project's own statement of the published method: the Newton-Raphson solution of the MBAR
equations, Shirts & Chodera, J. Chem. Phys. 129:124105, 2008, appendix C, with a self-consistent start and fall-back).

Notation as in tests/mbar_reference.py, whose helpers this module uses.  One pass over the used samples from ``f``:

    a_nj = ln N_j + f_j - E_n / T_j,  d_n = logsumexp_j a_nj,  W_nj = exp(a_nj - d_n)        (every row of W sums to 1)
    S_j = sum_n W_nj,  G = W^T W,  gamma = max_j |S_j / N_j - 1|

and then one step:

    self-consistent   f_j <- f_j - ln(S_j / N_j), then f <- f - f_0
    Newton            H = diag(S) - G;  H[1:, 1:] delta[1:] = (N - S)[1:] by Cholesky, delta_0 = 0;  f <- f + delta

Passes 1 and 2 take the self-consistent step, every later pass the Newton step.  When the step before a pass was a
Newton step and gamma is not below or at its value of the pass before, that step is withdrawn: f and S from before it come
back and the self-consistent step is taken from there.  A Cholesky pivot that is <= 0 or not finite makes the pass take the
self-consistent step.  ``residual`` is the largest change of an ``f_j`` in the step taken; the iteration stops once it is
``<= tol``.  Everything is evaluated in ``dtype`` (float64 or ``np.longdouble``); the sums are numpy's, not the device's.
"""
import functools
import os

import numpy as np

import mbar_reference as ref

SC, NEWTON, WITHDRAWN, PIVOT = "self-consistent", "newton", "withdrawn", "pivot"


def sums(e, temps, counts, f, dtype):
    """``(S, G)`` of the used samples ``e`` at ``f``."""
    ex, _, s = ref._log_weights(e, temps, counts, f, dtype)
    w = ex / s[:, None]
    return w.sum(axis=0), w.T @ w


def cholesky_solve(h, b):
    """``x`` with ``h x = b`` through ``h = L L^T``; ``None`` when a pivot is <= 0 or not finite."""
    n = h.shape[0]
    low = np.array(h, copy=True)
    for j in range(n):
        d = low[j, j]
        if not (np.isfinite(d) and d > 0):
            return None
        low[j, j] = np.sqrt(d)
        low[j + 1:, j] = low[j + 1:, j] / low[j, j]
        for k in range(j + 1, n):
            low[k:, k] = low[k:, k] - low[k:, j] * low[k, j]
    x = np.array(b, copy=True)
    for j in range(n):
        x[j] = x[j] / low[j, j]
        x[j + 1:] = x[j + 1:] - low[j + 1:, j] * x[j]
    for j in range(n - 1, -1, -1):
        x[j] = x[j] / low[j, j]
        x[:j] = x[:j] - low[j, :j] * x[j]
    return x


def self_consistent_step(f, big_s, n):
    f_new = f - np.log(big_s / n)
    return f_new - f_new[0]


def newton_step(f, big_s, gram, n):
    """``f + delta``, or ``None`` when the Cholesky factorisation fails."""
    if f.size == 1:
        return f.copy()
    h = np.diag(big_s) - gram
    delta = cholesky_solve(h[1:, 1:], (n - big_s)[1:])
    if delta is None:
        return None
    f_new = f.copy()
    f_new[1:] = f_new[1:] + delta
    return f_new


def solve(energies, rungs, temps, tol=1e-10, max_iter=10000, dtype=np.float64):
    """``(f, iterations, residual, gradient, kinds)`` from ``f = 0``: ``gradient`` is gamma at the last pass and ``kinds[i]``
    what pass ``i`` took (SC, NEWTON, WITHDRAWN: the self-consistent step after a withdrawn Newton step, PIVOT: the
    self-consistent step after a failed factorisation)."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, counts = ref.used(energies, rungs, temps.size)
    if np.any(counts == 0):
        raise ValueError("a rung has no finite sample")
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    n = counts.astype(dtype)
    f = np.zeros(temps.size, dtype=dtype)
    kinds = []
    if temps.size == 1:
        return f, 1, dtype(0.0), dtype(0.0), [SC]
    residual = gamma = dtype(np.inf)
    before = None                                  # (f, S, gamma) from which the last step was taken
    while len(kinds) < max_iter:
        big_s, gram = sums(e, temps, counts, f, dtype)
        gamma = np.max(np.abs(big_s / n - 1))
        f_new = None
        if kinds and kinds[-1] == NEWTON and not gamma <= before[2]:
            f, big_s, kept_gamma = before
            kind = WITHDRAWN
        else:
            kept_gamma = gamma
            kind = SC
            if len(kinds) >= 2:
                f_new = newton_step(f, big_s, gram, n)
                kind = PIVOT if f_new is None else NEWTON
        if f_new is None:
            f_new = self_consistent_step(f, big_s, n)
        before = (f, big_s, kept_gamma)
        residual = np.max(np.abs(f_new - f))
        f = f_new
        kinds.append(kind)
        if residual <= tol:
            break
    return f, len(kinds), residual, gamma, kinds


def fallbacks(kinds):
    return kinds.count(WITHDRAWN) + kinds.count(PIVOT)


# the seven ladders of the README's table: (rungs, samples per rung, dim, ratio), all gamma_ladder with seed 11
LADDERS = [(8, 512, 16, 1.3), (8, 4096, 16, 1.3), (33, 256, 16, 1.1), (64, 64, 16, 1.08), (8, 512, 16, 2.0),
           (6, 512, 64, 1.8), (16, 256, 64, 1.35)]


def ladder(k, per_rung, dim, ratio, seed=11):
    """``(energies, rungs, temps)`` of one such ladder, flattened."""
    energies, temps = ref.gamma_ladder(per_rung, n_rungs=k, dim=dim, seed=seed, ratio=ratio)
    return energies.ravel(), np.repeat(np.arange(k, dtype=np.int32), per_rung), temps


def compute_fixed_point(index):
    """The long-double self-consistent fixed point of ``LADDERS[index]`` from ``f = 0`` (``tol = 1e-14``): the yardstick of both
    methods.  Thousands of long-double iterations on the poorly overlapping ladders, which is why the tests read it from
    ``tests/golden/mbar_newton_fixed_points.npz`` (``write_fixed_points``) and check there that one more iteration leaves it
    where it is."""
    e, r, t = ladder(*LADDERS[index])
    return ref.solve(e, r, t, tol=1e-14, max_iter=100000, dtype=np.longdouble)[0]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mbar_newton_fixed_points.npz")


def write_fixed_points(path=GOLDEN):
    """Every ``compute_fixed_point`` as a float64 pair ``hi + lo`` (``python tests/mbar_newton_reference.py``)."""
    out = {}
    for index in range(len(LADDERS)):
        f = compute_fixed_point(index)
        hi = f.astype(np.float64)
        out["hi_%d" % index], out["lo_%d" % index] = hi, (f - hi).astype(np.float64)
    np.savez(path, **out)


@functools.lru_cache(maxsize=None)
def fixed_point(index):
    """``compute_fixed_point(index)`` from the golden file, as long double; treat the array as read-only."""
    with np.load(GOLDEN) as z:
        return z["hi_%d" % index].astype(np.longdouble) + z["lo_%d" % index].astype(np.longdouble)


@functools.lru_cache(maxsize=None)
def solved(index, tol=1e-10):
    """``solve`` of ``LADDERS[index]`` in float64, computed once per process."""
    e, r, t = ladder(*LADDERS[index])
    return solve(e, r, t, tol=tol)


if __name__ == "__main__":
    write_fixed_points()
