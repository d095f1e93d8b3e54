"""numpy restatement of the MBAR reweighting of recorded observables (metropolisengine_amd/csrc/me_mbar_obs.hip) and of
the catalogue of a chain's recordable quantities; exact moments of E = a |x|^2; the generator of the statistical test's
inputs (test infrastructure shared by test_mbar_observables_cpu.py and test_gpu_mbar_observables.py).

The weighted moments are plain two-pass sums in ``dtype`` (float64, or ``np.longdouble`` as the yardstick of the device's
float64); the log weights are those of tests/mbar_reference.py.
"""
import numpy as np

from mbar_reference import _log_weights, used

LADDER8 = 0.5 * 1.3 ** np.arange(8)


def reweight_observables(energies, rungs, temps, f, targets, observables, dtype=np.float64):
    """``(mean, var, cov_energy, neff_fraction)`` at every temperature of ``targets``: the first three ``(T, Q)``, the last
    ``(T,)``.  ``observables`` is ``(Q, n_samples)`` in the order of ``energies``; a sample is used when its energy is
    finite."""
    temps = np.asarray(temps, dtype=np.float64)
    ok, counts = used(energies, rungs, temps.size)
    e = np.asarray(energies, dtype=np.float64).ravel()[ok].astype(dtype)
    a = np.asarray(observables, dtype=np.float64).reshape(-1, ok.size)[:, ok].astype(dtype)
    d = np.empty(e.size, dtype=dtype)
    for i in range(0, e.size, 1 << 18):         # (in slices: the K columns of 2^22 long doubles would take gigabytes)
        _, m, s = _log_weights(e[i:i + (1 << 18)], temps, counts, f, dtype)
        d[i:i + (1 << 18)] = m + np.log(s)
    targets = np.asarray(targets, dtype=dtype)
    mean, var, cov = (np.zeros((targets.size, a.shape[0]), dtype=dtype) for _ in range(3))
    neff = np.zeros(targets.size, dtype=dtype)
    for i, t in enumerate(targets):
        l = -e / t - d
        w = np.exp(l - l.max())
        sw = w.sum()
        mean_e = (w * e).sum() / sw
        mean[i] = (w[None, :] * a).sum(axis=1) / sw
        dev = a - mean[i][:, None]
        var[i] = (w[None, :] * dev * dev).sum(axis=1) / sw
        cov[i] = (w[None, :] * dev * (e - mean_e)[None, :]).sum(axis=1) / sw
        neff[i] = sw * sw / (e.size * (w * w).sum())
    return mean, var, cov, neff


def catalogue_names(n_real, n_complex, term_names):
    return (["real_%d" % i for i in range(n_real)] + ["re_%d" % i for i in range(n_complex)] +
            ["im_%d" % i for i in range(n_complex)] + ["abs_real_%d" % i for i in range(n_real)] +
            ["abs_complex_%d" % i for i in range(n_complex)] + ["real_%d_sq" % i for i in range(n_real)] +
            ["energy_%s" % name for name in term_names])


def catalogue_values(params, ledger, n_real, n_complex):
    """The host's restatement of a record: ``params`` (chains, D) and ``ledger`` (chains, T) as ``me_get`` returns them (the
    device values widened to float64) -> ``(catalogue size, chains)`` float64.  ``|z|`` is ``np.hypot`` here (the device
    takes ``sqrt(fma(re, re, im im))``: each is within 1 ulp of the exact value, so they differ by at most 2 ulp)."""
    x = np.asarray(params, dtype=np.float64)
    nr, nc = n_real, n_complex
    xr, re, im = x[:, :nr], x[:, nr:nr + nc], x[:, nr + nc:]
    return np.concatenate([x, np.abs(xr), np.hypot(re, im), xr * xr, np.asarray(ledger, dtype=np.float64)], axis=1).T.copy()


def exact_iso_quadratic(t, a=1.0):
    """E = a |x|^2 at temperature ``t``, any component i: ``{"x", "abs_x", "x_sq", "var_x_sq", "cov_x_sq_e"}`` = <x_i> = 0,
    <|x_i|> = sqrt(T / pi a), <x_i^2> = T / 2a, Var x_i^2 = T^2 / 2a^2, Cov(x_i^2, E) = T^2 / 2a (so d<x_i^2>/dT = 1 / 2a)."""
    t = np.asarray(t, dtype=np.float64)
    return {"x": np.zeros_like(t), "abs_x": np.sqrt(t / (np.pi * a)), "x_sq": t / (2 * a), "var_x_sq": t * t / (2 * a * a),
            "cov_x_sq_e": t * t / (2 * a)}


PHYSICS_TARGETS = np.array([0.6, 1.0, 2.2])        # between the rungs of LADDER8
PHYSICS_SUBSETS = 16
PHYSICS_PER_RUNG = 1024


def iso_quadratic_subsets(seed=29, dim=4, a=1.0, temps=LADDER8, n_subsets=PHYSICS_SUBSETS, per_rung=PHYSICS_PER_RUNG):
    """Independent subsets of exact samples of E = a |x|^2 in ``dim`` real dimensions: per subset and rung ``per_rung``
    configurations x ~ N(0, T_k / 2a).  Returns a list of ``(energies [n], rungs [n], observables [3, n])`` with the
    columns ``x_0``, ``|x_0|``, ``x_0^2`` and n = K per_rung."""
    rng = np.random.default_rng(seed)
    temps = np.asarray(temps, dtype=np.float64)
    rungs = np.repeat(np.arange(temps.size), per_rung).astype(np.int32)
    out = []
    for _ in range(n_subsets):
        x = rng.standard_normal((temps.size * per_rung, dim)) * np.sqrt(temps[rungs] / (2 * a))[:, None]
        out.append((a * (x * x).sum(axis=1), rungs, np.stack([x[:, 0], np.abs(x[:, 0]), x[:, 0] ** 2])))
    return out


def physics_estimates(results, targets=PHYSICS_TARGETS):
    """The twelve compared quantities from per-subset results ``(mean (T, 3), cov_energy (T, 3))``: a dictionary name ->
    ``(estimates [subsets, T], exact [T])`` for the means of x_0, |x_0|, x_0^2 and for d<x_0^2>/dT."""
    exact = exact_iso_quadratic(targets)
    mean = np.array([r[0] for r in results])
    dmean = np.array([r[1][:, 2] / targets ** 2 for r in results])
    return {"mean x_0": (mean[:, :, 0], exact["x"]), "mean |x_0|": (mean[:, :, 1], exact["abs_x"]),
            "mean x_0^2": (mean[:, :, 2], exact["x_sq"]), "dmean_dT x_0^2": (dmean, exact["cov_x_sq_e"] / targets ** 2)}
