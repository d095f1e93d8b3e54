"""numpy restatement of the MBAR iteration and of the temperature reweighting of metropolisengine_amd/csrc/me_mbar.hip
(test infrastructure; this project's own statement of the published method, Shirts & Chodera, J. Chem. Phys. 129:124105).

Everything is evaluated in ``dtype`` (float64, or ``np.longdouble`` as the yardstick of the device's float64).  The sums
are numpy's (pairwise), not the device's order: the two agree to rounding, which is what the tests ask for.
"""
import numpy as np


def used(energies, rungs, n_rungs):
    """``(finite mask, N_k)``: a sample is used when its energy is finite."""
    e = np.asarray(energies, dtype=np.float64).ravel()
    ok = np.isfinite(e)
    counts = np.bincount(np.asarray(rungs).ravel()[ok], minlength=n_rungs).astype(np.int64)
    return ok, counts


def _log_weights(e, temps, counts, f, dtype):
    """``a_nj = ln N_j + f_j - E_n / T_j``, ``m_n`` and ``s_n = sum_j exp(a_nj - m_n)`` for the used samples ``e``."""
    beta = dtype(1.0) / np.asarray(temps, dtype=dtype)
    c = np.log(np.asarray(counts, dtype=dtype)) + np.asarray(f, dtype=dtype)
    a = c[None, :] - e[:, None] * beta[None, :]
    m = a.max(axis=1)
    ex = np.exp(a - m[:, None])
    return ex, m, ex.sum(axis=1)


def iterate(energies, rungs, temps, f, dtype=np.float64):
    """One self-consistent iteration from ``f``: returns ``(f_new, residual)``."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, counts = used(energies, rungs, temps.size)
    if np.any(counts == 0):
        raise ValueError("a rung has no finite sample")
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    f = np.asarray(f, dtype=dtype)
    ex, _, s = _log_weights(e, temps, counts, f, dtype)
    big_s = (ex / s[:, None]).sum(axis=0)
    f_new = f - np.log(big_s / counts.astype(dtype))
    f_new = f_new - f_new[0]
    return f_new, np.max(np.abs(f_new - f))


def solve(energies, rungs, temps, tol=1e-10, max_iter=10000, dtype=np.float64):
    """``(f, iterations, residual, N_k)`` from ``f = 0``."""
    temps = np.asarray(temps, dtype=np.float64)
    _, counts = used(energies, rungs, temps.size)
    f = np.zeros(temps.size, dtype=dtype)
    residual = dtype(np.inf)
    it = 0
    while it < max_iter:
        f, residual = iterate(energies, rungs, temps, f, dtype)
        it += 1
        if residual <= tol:
            break
    return f, it, residual, counts


def reweight(energies, rungs, temps, f, targets, dtype=np.float64):
    """``(ln_z, energy_mean, energy_var, neff_fraction)`` at every temperature of ``targets``."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, counts = used(energies, rungs, temps.size)
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    _, m, s = _log_weights(e, temps, counts, f, dtype)
    d = m + np.log(s)
    out = np.zeros((4, len(targets)), dtype=dtype)
    for i, t in enumerate(np.asarray(targets, dtype=dtype)):
        l = -e / t - d
        big_m = l.max()
        w = np.exp(l - big_m)
        sw = w.sum()
        mean = (w * e).sum() / sw
        out[0, i] = big_m + np.log(sw)
        out[1, i] = mean
        out[2, i] = (w * (e - mean) ** 2).sum() / sw
        out[3, i] = sw * sw / (e.size * (w * w).sum())
    return out


def gamma_ladder(n_per_rung, n_rungs=8, dim=16, seed=11, t0=0.5, ratio=1.3):
    """Energies of a quadratic form in ``dim`` real dimensions at ``T_k = t0 ratio^k``: ``E / T`` is Gamma(dim / 2)
    distributed, so ``ln Z(T_k) / Z(T_0) = (dim / 2) ln(T_k / T_0)``, ``<E> = dim T / 2``, ``Var E = dim T^2 / 2`` exactly.
    Returns ``(energies [n_rungs, n_per_rung], temps)``."""
    rng = np.random.default_rng(seed)
    temps = t0 * ratio ** np.arange(n_rungs)
    return np.stack([rng.gamma(dim / 2.0, t, size=n_per_rung) for t in temps]), temps


def exact_gamma(temps_or_t, t0, dim=16):
    """``(ln_z, mean, var)`` of the quadratic form at temperature(s) ``T`` relative to ``t0``."""
    t = np.asarray(temps_or_t, dtype=np.float64)
    return dim / 2.0 * np.log(t / t0), dim * t / 2.0, dim * t * t / 2.0


def within_5_se(estimates, exact):
    """``(ok, mean, se)``: |mean over the independent estimates (axis 0) - exact| <= 5 standard errors, elementwise."""
    est = np.asarray(estimates, dtype=np.float64)
    mean = est.mean(axis=0)
    se = est.std(axis=0, ddof=1) / np.sqrt(est.shape[0])
    return np.abs(mean - exact) <= 5.0 * se, mean, se
