"""numpy restatement of the MBAR weight matrix with the second-moment columns and of the asymptotic errors of reweighted
variances and energy covariances (csrc/me_mbar_cov.hip, the fluctuation form, has the definitions; Shirts & Chodera, J. Chem.
Phys. 129:124105, 2008, eqs. 8, D8, and the delta method).  The ladder and state columns, both routes to Theta and the bound
between them are those of tests/mbar_uncertainty_reference.py, imported; this module adds the columns E', E'^2, A'_q, A'_q^2,
A'_q E' in ``np.longdouble`` and what is derived from Theta.  Also the exact values of the calibration problem."""
import numpy as np

from mbar_uncertainty_reference import LD, gram, route_bound, solve, theta_gram, theta_svd, weight_matrix  # noqa: F401
from mbar_observable_uncertainty_reference import (LADDER8, PHYSICS_TARGETS, calibration_subsets, column_shifts,  # noqa: F401
                                                   iso_quadratic_subsets, synthetic_columns)

KEYS = ("d_energy_mean", "d_energy_var", "d_mean", "d_var", "d_cov_energy")


def width(q):
    """Columns of one target: state, E', E'^2, then A', A'^2, A' E' of each observable."""
    return 3 + 3 * q


def weight_matrix_fluctuations(energies, rungs, temps, f, targets, observables=None, moments=None, energy_shift=None, shifts=None):
    """``(W, counts, ln_z, moments, energy_shift, shifts)`` in long double over the samples with a finite energy.  Columns: rung
    k at k; from K + t (3 + 3 Q) on the state column of target t, W_na E' / m, W_na E'^2 / m, then for each q W_na A'_q / m,
    W_na A'_q^2 / m, W_na A'_q E' / m, with E' = E - energy_shift, A'_q = A_q - S_q and m the weighted mean of the factor.
    ``moments`` (T, 2 + 3 Q), ``energy_shift`` and ``shifts`` (Q,) replace the normalisers and the shifts (to pass the device's
    own in); the returned ``moments`` are always the long-double ones for the shifts in use."""
    targets = np.atleast_1d(np.asarray(targets, dtype=np.float64))
    k = np.asarray(temps).size
    w_e, counts_e, ln_z, _, shift_e = weight_matrix(energies, rungs, temps, f, targets)
    e64 = np.asarray(energies, dtype=np.float64).ravel()
    used = np.isfinite(e64)
    a = (np.zeros((0, used.size)) if observables is None else np.asarray(observables, dtype=np.float64).reshape(-1, used.size))
    a = a[:, used].astype(LD)
    q = a.shape[0]
    s_e = shift_e if energy_shift is None else LD(np.float64(energy_shift))
    if q == 0:
        s = np.zeros(0, dtype=LD)
    else:
        s = (column_shifts(energies, observables) if shifts is None else np.asarray(shifts, dtype=np.float64)[:q]).astype(LD)
    e1 = e64[used].astype(LD) - s_e
    factors = [e1, e1 * e1]
    for j in range(q):
        a1 = a[j] - s[j]
        factors += [a1, a1 * a1, a1 * e1]
    cols = [w_e[:, j] for j in range(k)]
    own = np.zeros((targets.size, 2 + 3 * q), dtype=LD)
    for t in range(targets.size):
        state = w_e[:, k + 2 * t]
        own[t] = [(state * x).sum() for x in factors]
        norm = own[t] if moments is None else np.asarray(moments, dtype=np.float64)[t].astype(LD)
        cols.append(state)
        cols += [state * x / norm[i] for i, x in enumerate(factors)]
    counts = np.concatenate([counts_e[:k], np.zeros(targets.size * width(q), dtype=LD)])
    return np.stack(cols, axis=1), counts, ln_z, own, s_e, s


def values(moments, q):
    """``(var_e (T,), var (T, Q), cov_energy (T, Q))`` from the shifted moments (the shifts drop out)."""
    m = np.asarray(moments)
    m_a, m_a2, m_ae = (m[:, 2 + j:2 + 3 * q:3] for j in range(3))
    return m[:, 1] - m[:, 0] ** 2, m_a2 - m_a ** 2, m_ae - m_a * m[:, [0]]


def variances(theta, k, n_targets, q, moments):
    """``(var, scale)``, dictionaries over KEYS of the squares of :func:`sigmas` without the clamp, and of the largest |Theta|
    entry times ``(sum_i |g_i m_i|)^2``.  With the state column a of the target, the covariance of the estimated moments is C_ij
    = m_i m_j (Theta_ij + Theta_aa - Theta_ia - Theta_ja) and a variance is g^T C g: a sum over (i, j) of four entries of Theta
    with coefficients of magnitude |g_i m_i g_j m_j|, so two Thetas that differ by ``b max |Theta|`` entrywise give variances
    within ``4 b scale`` of each other (the rule of ``mbar_uncertainty_reference.variances``).  Gradients: (1) on E' and on A';
    (-2 m_E, 1) on (E', E'^2); (-2 m_A, 1) on (A', A'^2); (1, -m_E, -m_A) on (A' E', A', E')."""
    theta = np.asarray(theta, dtype=np.float64)
    m = np.asarray(moments, dtype=np.float64)
    top = np.abs(theta).max()
    var = {key: np.zeros((n_targets, q) if key in KEYS[2:] else n_targets) for key in KEYS}
    scale = {key: np.zeros_like(v) for key, v in var.items()}

    def put(key, where, a, rows, mm, gradient):
        rows = np.asarray(rows, dtype=np.intp)
        c = theta[np.ix_(rows, rows)] + theta[a, a] - theta[rows, a][:, None] - theta[rows, a][None, :]
        gm = np.asarray(gradient, dtype=np.float64) * np.asarray(mm, dtype=np.float64)
        var[key][where] = gm @ c @ gm
        scale[key][where] = top * np.abs(gm).sum() ** 2

    for t in range(n_targets):
        a = k + t * width(q)
        m_e, m_e2 = m[t, 0], m[t, 1]
        put("d_energy_mean", t, a, [a + 1], [m_e], [1.0])
        put("d_energy_var", t, a, [a + 1, a + 2], [m_e, m_e2], [-2.0 * m_e, 1.0])
        for j in range(q):
            c = a + 3 + 3 * j
            m_a, m_a2, m_ae = m[t, 2 + 3 * j:5 + 3 * j]
            put("d_mean", (t, j), a, [c], [m_a], [1.0])
            put("d_var", (t, j), a, [c, c + 1], [m_a, m_a2], [-2.0 * m_a, 1.0])
            put("d_cov_energy", (t, j), a, [c + 2, c, a + 1], [m_ae, m_a, m_e], [1.0, -m_e, -m_a])
    return var, scale


def sigmas(theta, k, n_targets, q, moments):
    """The standard errors over KEYS: the clamped square roots of :func:`variances`."""
    var, _ = variances(theta, k, n_targets, q, moments)
    return {key: np.sqrt(np.clip(v, 0.0, None)) for key, v in var.items()}


# ---- the calibration problem: E = |x|^2 in 4 dimensions, columns x_0, |x_0|, x_0^2, sigma^2 = T / 2 ---------------------------
def exact_fluctuations(targets=PHYSICS_TARGETS):
    """``(Var E (T,), Var A_q (T, 3), Cov(A_q, E) (T, 3))``: 2 T^2; sigma^2, sigma^2 (1 - 2 / pi), 2 sigma^4; 0, sigma^3 sqrt(2 /
    pi), 2 sigma^4."""
    t = np.asarray(targets, dtype=np.float64)
    s2 = t / 2.0
    return (2.0 * t * t, np.stack([s2, s2 * (1.0 - 2.0 / np.pi), 2.0 * s2 ** 2], axis=1),
            np.stack([np.zeros_like(t), s2 ** 1.5 * np.sqrt(2.0 / np.pi), 2.0 * s2 ** 2], axis=1))


def calibration_rms_z(estimates, errors):
    """RMS z-score (T, 7) over the subsets (axis 0): ``estimates`` and ``errors`` are lists of ``(var_e (T,), var (T, 3), cov_energy
    (T, 3))`` per subset; columns Var E, Var A_q, Cov(A_q, E).  Cov(x_0, E) is exactly 0: its z is the estimate itself over its
    error, an absolute difference like the others."""
    def table(rows):
        return np.array([np.concatenate([np.asarray(r[0], dtype=np.float64)[:, None], r[1], r[2]], axis=1) for r in rows])
    exact = table([exact_fluctuations()])[0]
    z = (table(estimates) - exact[None]) / table(errors)
    return np.sqrt((z * z).mean(axis=0))
