"""numpy restatement of the MBAR weight matrix with observable-weighted columns and of the asymptotic covariance of reweighted
observable means (csrc/me_mbar_cov.hip, the observable form, has the definitions; Shirts & Chodera, J. Chem. Phys.
129:124105, 2008, eqs. 8, 12-15, D8).  The ladder and state columns, both routes to Theta and the bound between them are
those of tests/mbar_uncertainty_reference.py, imported; this module adds the observable columns in ``np.longdouble`` and what
is derived from Theta.  Also the shared inputs of tests/test_mbar_observable_uncertainty_cpu.py and
tests/test_gpu_mbar_observable_uncertainty.py."""
import numpy as np

from mbar_uncertainty_reference import LD, gram, route_bound, solve, theta_gram, theta_svd, weight_matrix  # noqa: F401
from mbar_observables_reference import LADDER8, PHYSICS_TARGETS, exact_iso_quadratic, iso_quadratic_subsets

CAL_SUBSETS, CAL_PER_RUNG = 64, 512


def column_shifts(energies, observables):
    """``S_q``: (the least finite value of column q over the samples with a finite energy) - 1, float64."""
    used = np.isfinite(np.asarray(energies, dtype=np.float64).ravel())
    a = np.asarray(observables, dtype=np.float64).reshape(-1, used.size)[:, used]
    return np.array([col[np.isfinite(col)].min() - 1.0 if np.isfinite(col).any() else np.inf for col in a])


def weight_matrix_observables(energies, rungs, temps, f, targets, observables, means=None, shifts=None):
    """``(W, counts, ln_z, mean, shifts)`` in long double over the samples with a finite energy.  Columns: rung k at k, the
    state column of target t at K + t (1 + Q), its observable q at K + t (1 + Q) + 1 + q.  ``means`` (T, Q) and ``shifts``
    (Q,) replace the normalising means and the shifts (to pass the device's own in); ``mean`` is always the long-double
    reweighted mean."""
    targets = np.atleast_1d(np.asarray(targets, dtype=np.float64))
    k = np.asarray(temps).size
    w_e, counts_e, ln_z, _, _ = weight_matrix(energies, rungs, temps, f, targets)
    used = np.isfinite(np.asarray(energies, dtype=np.float64).ravel())
    a = np.asarray(observables, dtype=np.float64).reshape(-1, used.size)[:, used].astype(LD)
    q = a.shape[0]
    s = (column_shifts(energies, observables) if shifts is None else np.asarray(shifts, dtype=np.float64)).astype(LD)
    cols = [w_e[:, j] for j in range(k)]
    mean = np.zeros((targets.size, q), dtype=LD)
    for t in range(targets.size):
        state = w_e[:, k + 2 * t]
        mean[t] = (state[None, :] * a).sum(axis=1)
        norm = (mean[t] if means is None else np.asarray(means, dtype=np.float64)[t].astype(LD)) - s
        cols.append(state)
        cols += [state * (a[j] - s[j]) / norm[j] for j in range(q)]
    counts = np.concatenate([counts_e[:k], np.zeros(targets.size * (1 + q), dtype=LD)])
    return np.stack(cols, axis=1), counts, ln_z, mean, s


def covariances(theta, k, n_targets, q, mean, shifts):
    """``(mean_cov (T, Q, Q), scale (T, Q, Q))`` from Theta over the K + T (1 + Q) columns, without a clamp: ``mean_cov[t]`` is
    the covariance of the Q estimates at target t, its diagonal ``d_mean ** 2``.  Every entry is a sum of four entries of
    Theta with coefficients of magnitude 1 times (mean_q - S_q)(mean_r - S_r), so two Thetas that differ by ``b max |Theta|``
    entrywise give entries within ``4 b scale`` of each other (the rule of ``mbar_uncertainty_reference.variances``)."""
    theta = np.asarray(theta, dtype=np.float64)
    m = np.asarray(mean, dtype=np.float64) - np.asarray(shifts, dtype=np.float64)[None, :]
    top = np.abs(theta).max()
    cov, scale = np.zeros((n_targets, q, q)), np.zeros((n_targets, q, q))
    for t in range(n_targets):
        a = k + t * (1 + q)
        rows = a + 1 + np.arange(q)
        outer = m[t][:, None] * m[t][None, :]
        cov[t] = outer * (theta[np.ix_(rows, rows)] + theta[a, a] - theta[rows, a][:, None] - theta[rows, a][None, :])
        scale[t] = top * np.abs(outer)
    return cov, scale


def sigmas(theta, k, n_targets, q, mean, shifts):
    """``(d_mean (T, Q), mean_cov (T, Q, Q))``: the standard errors are the clamped square roots of the diagonals."""
    cov, _ = covariances(theta, k, n_targets, q, mean, shifts)
    return np.sqrt(np.clip(np.diagonal(cov, axis1=1, axis2=2), 0.0, None)), cov


# ---- shared inputs ----------------------------------------------------------------------------------------------------
def calibration_subsets():
    """The 64 subsets of 8 x 512 exact samples of E = |x|^2 on LADDER8 with the columns x_0, |x_0|, x_0^2."""
    return iso_quadratic_subsets(seed=29, n_subsets=CAL_SUBSETS, per_rung=CAL_PER_RUNG)


def calibration_exact():
    """The exact means (T, 3) of the three columns at PHYSICS_TARGETS."""
    exact = exact_iso_quadratic(PHYSICS_TARGETS)
    return np.stack([exact["x"], exact["abs_x"], exact["x_sq"]], axis=1)


def calibration_rms_z(means, d_means):
    """RMS z-score (T, 3) over the subsets (axis 0) of ``means`` against the exact values."""
    z = (np.asarray(means, dtype=np.float64) - calibration_exact()[None]) / np.asarray(d_means, dtype=np.float64)
    return np.sqrt((z * z).mean(axis=0))


def synthetic_columns(energies, q, seed=31):
    """``q`` columns ``c_j E + s_j z_j`` for the energies of ``mbar_uncertainty_reference.synthetic``: ``z_j`` fixed-seed standard
    normals, the (c_j, s_j) distinct, and c_1 = 0: a zero-mean column among columns that follow the energy."""
    e = np.asarray(energies, dtype=np.float64)
    z = np.random.default_rng(seed).standard_normal((q, e.size))
    c = np.array([0.0 if j == 1 else 0.25 * (1 + j) for j in range(q)])
    s = 0.5 + 0.125 * np.arange(q)
    return c[:, None] * e[None, :] + s[:, None] * z
