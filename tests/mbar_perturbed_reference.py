"""numpy restatement of the MBAR reweighting to perturbed energies (metropolisengine_amd/csrc/me_mbar_perturbed.hip), the
couplings the GPU tests use, and the closed forms and harness of the statistical test (test infrastructure shared by
test_mbar_perturbed_cpu.py and test_gpu_mbar_perturbed.py).

Target p has a temperature T_p and couplings lambda_p over the Q columns; with b = sum over the q with lambda_pq != 0, in
ascending q, of lambda_pq A_q and H = E + b its log weight is -H / T_p - d_n, d_n that of tests/mbar_reference.py.  The
weighted moments are plain two-pass sums in ``dtype`` (float64, or ``np.longdouble`` as the yardstick of the device's float64).
"""
import numpy as np

from mbar_reference import _log_weights, used, within_5_se

KEYS = ("ln_z", "hamiltonian_mean", "hamiltonian_var", "mean", "var", "cov_hamiltonian", "neff_fraction")


def reweight_perturbed(energies, rungs, temps, f, targets, couplings, observables, dtype=np.float64):
    """A dictionary with the ``KEYS``: ``mean``, ``var``, ``cov_hamiltonian`` are ``(P, Q)``, the others ``(P,)``.
    ``observables`` is ``(Q, n_samples)`` in the order of ``energies``, ``couplings`` ``(P, Q)``; a sample is used when its
    energy is finite, and a column whose coupling is exactly 0 is not read for the bias."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, counts = used(energies, rungs, temps.size)
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    a = np.asarray(observables, dtype=np.float64).reshape(-1, ok.size)[:, ok].astype(dtype)
    d = np.empty(e.size, dtype=dtype)
    for i in range(0, e.size, 1 << 18):         # (in slices: the K columns of 2^22 long doubles would take gigabytes)
        _, m, s = _log_weights(e[i:i + (1 << 18)], temps, counts, f, dtype)
        d[i:i + (1 << 18)] = m + np.log(s)
    targets = np.asarray(targets, dtype=dtype)
    lam = np.asarray(couplings, dtype=np.float64).reshape(targets.size, a.shape[0])
    out = {key: np.zeros((targets.size, a.shape[0]) if key in ("mean", "var", "cov_hamiltonian") else targets.size, dtype=dtype)
           for key in KEYS}
    for p, t in enumerate(targets):
        b = np.zeros(e.size, dtype=dtype)
        for q in np.flatnonzero(lam[p]):
            b = dtype(lam[p, q]) * a[q] + b
        h = e + b
        l = -h / t - d
        big_m = l.max()
        w = np.exp(l - big_m)
        sw = w.sum()
        mean_h = (w * h).sum() / sw
        out["ln_z"][p] = big_m + np.log(sw)
        out["hamiltonian_mean"][p] = mean_h
        out["hamiltonian_var"][p] = (w * (h - mean_h) ** 2).sum() / sw
        out["mean"][p] = (w[None, :] * a).sum(axis=1) / sw
        dev = a - out["mean"][p][:, None]
        out["var"][p] = (w[None, :] * dev * dev).sum(axis=1) / sw
        out["cov_hamiltonian"][p] = (w[None, :] * dev * (h - mean_h)[None, :]).sum(axis=1) / sw
        out["neff_fraction"][p] = sw * sw / (e.size * (w * w).sum())
    return out


def case_couplings(n_targets, n_columns):
    """The couplings of the GPU tests: ``0.05 (-1)^(p + q) / (q + 1)``, 0 where ``(p + 2 q) % 3 == 0`` (so every target skips
    columns and every chunk of targets has columns nobody couples to); the one-target, one-column case is ``0.05``."""
    if (n_targets, n_columns) == (1, 1):
        return np.array([[0.05]])
    p, q = np.meshgrid(np.arange(n_targets), np.arange(n_columns), indexing="ij")
    lam = 0.05 * (-1.0) ** (p + q) / (q + 1.0)
    lam[(p + 2 * q) % 3 == 0] = 0.0
    return lam


# ---- the statistical test: E = |x|^2 in 4 dimensions, columns x_0, |x_0|, x_0^2 (mbar_observables_reference.iso_quadratic_subsets)
# (T, (lambda_x0, lambda_|x0|, lambda_x0^2)); the three unperturbed targets behind them give ln_z(T, 0)
PHYSICS_TARGETS = ([(t, (0.0, 0.0, 0.5)) for t in (0.6, 1.0, 2.2)] + [(t, (-0.5, 0.0, 0.0)) for t in (0.6, 1.0, 2.2)] +
                   [(1.0, (0.0, 0.0, -0.3)), (1.0, (-0.4, 0.0, 0.25))])
PHYSICS_BASE = (0.6, 1.0, 2.2)
PHYSICS_TEMPS = np.array([t for t, _ in PHYSICS_TARGETS] + list(PHYSICS_BASE))
PHYSICS_COUPLINGS = np.array([lam for _, lam in PHYSICS_TARGETS] + [(0.0, 0.0, 0.0)] * len(PHYSICS_BASE))


def physics_exact():
    """The closed forms at ``PHYSICS_TARGETS``.  The x_0 part of H is k x_0^2 - h x_0 with h = -lambda_x0, k = 1 + lambda_x0^2:
    a Gaussian of mean h / 2k and variance T / 2k, and Z(T, lambda) / Z(T, 0) = k^(-1/2) exp(h^2 / 4kT)."""
    t = np.array([t for t, _ in PHYSICS_TARGETS])
    h = -np.array([lam[0] for _, lam in PHYSICS_TARGETS])
    k = 1.0 + np.array([lam[2] for _, lam in PHYSICS_TARGETS])
    return {"delta ln_z": -0.5 * np.log(k) + h * h / (4 * k * t), "mean x_0": h / (2 * k),
            "mean x_0^2": t / (2 * k) + (h / (2 * k)) ** 2, "var x_0": t / (2 * k)}


def physics_estimates(results):
    """The 32 compared quantities from per-subset results at ``PHYSICS_TEMPS`` / ``PHYSICS_COUPLINGS`` (dictionaries with
    ``ln_z``, ``mean``, ``var``): name -> ``(estimates [subsets, 8], exact [8])``."""
    n = len(PHYSICS_TARGETS)
    base = [PHYSICS_BASE.index(t) + n for t, _ in PHYSICS_TARGETS]
    exact = physics_exact()
    est = {"delta ln_z": np.array([np.asarray(r["ln_z"])[:n] - np.asarray(r["ln_z"])[base] for r in results]),
           "mean x_0": np.array([np.asarray(r["mean"])[:n, 0] for r in results]),
           "mean x_0^2": np.array([np.asarray(r["mean"])[:n, 2] for r in results]),
           "var x_0": np.array([np.asarray(r["var"])[:n, 0] for r in results])}
    return {name: (est[name], exact[name]) for name in exact}


def check_physics(results):
    """All 32 within 5 standard errors (printed); returns the largest deviation in standard errors."""
    worst, n = 0.0, 0
    for name, (est, exact) in physics_estimates(results).items():
        ok, m, se = within_5_se(est, exact)
        dev = np.abs(m - exact) / se
        print(name, "mean", m, "exact", exact, "se", se, "deviation / se", dev)
        assert np.all(ok), name
        worst, n = max(worst, float(dev.max())), n + ok.size
    assert n == 32
    return worst
