"""Post-hoc equilibration statistics -- host side, off the accelerated hot path.

Mirrors the reference's ``metropolisengine/statistics.py:25-64`` (``get_equilibration_points``,
``get_equilibrated_means``) and ``MetropolisEngine.save_equilibrium_stats`` (metropolis_engine.py:481-504).

PARITY UNPINNED.  The arithmetic of the reference lives in ``pymbar.timeseries.detectEquilibration`` (statistics.py:4,
:41-46): a third-party dependency that is not vendored, not version-pinned (setup.py:22 misspells
``install_requires``) and not installed offline, and the reference holds no output of it.  The two functions below
restate the published algorithm (J. D. Chodera, "A simple method for automated equilibration detection in molecular
simulations", JCTC 12:1799, 2016; statistical inefficiency after Chodera et al., JCTC 3:26, 2007, as implemented in
pymbar 3.x ``timeseries.statisticalInefficiency`` / ``detectEquilibration``) and are tested against analytic
AR(1) autocorrelation times only.
"""
import ctypes

import numpy as np

from . import _capi


def statistical_inefficiency(series, mintime=3, fast=False):
    """``g = 1 + 2 tau``: sum the normalised autocorrelation function until it first turns non-positive (after
    ``mintime`` lags); ``fast`` lengthens the lag increment by one at every step."""
    a = np.asarray(series, dtype=np.float64)
    n = a.size
    da = a - a.mean()
    sigma2 = np.mean(da * da)
    if sigma2 == 0:
        raise ValueError("sample covariance is zero: cannot compute the statistical inefficiency")
    g = 1.0
    t = 1
    increment = 1
    while t < n - 1:
        c = np.sum(da[:n - t] * da[t:]) / ((n - t) * sigma2)
        if c <= 0.0 and t > mintime:
            break
        g += 2.0 * c * (1.0 - t / n) * increment
        t += increment
        if fast:
            increment += 1
    return max(g, 1.0)


def detect_equilibration(series, fast=True, nskip=1):
    """``(t0, g, Neff_max)``: the start ``t0`` of the production region that maximises the number of effectively
    uncorrelated samples ``(T - t0 + 1) / g(t0)``."""
    a = np.asarray(series, dtype=np.float64)
    big_t = a.size
    if a.std() == 0.0:
        return 0, 1.0, 1.0
    g_t = np.ones(big_t - 1)
    neff_t = np.ones(big_t - 1)
    for t in range(0, big_t - 1, nskip):
        try:
            g_t[t] = statistical_inefficiency(a[t:], fast=fast)
        except ValueError:
            g_t[t] = big_t - t + 1
        neff_t[t] = (big_t - t + 1) / g_t[t]
    t0 = int(np.argmax(neff_t))
    return t0, float(g_t[t0]), float(neff_t[t0])


def detect_equilibration_batch(series, fast=True, nskip=1, device=0):
    """``detect_equilibration`` for every row of ``series[n_series, T]`` in one call on the GPU
    (``me_detect_equilibration``: one wavefront per (series, start)); returns ``(t0, g, Neff_max)`` arrays.  An
    ensemble run records thousands of chains x columns, each an O(T^2) scan on the host."""
    a = np.ascontiguousarray(series, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError("series must be [n_series, length]")
    n, length = a.shape
    t0 = np.zeros(n, dtype=np.int64)
    g = np.ones(n)
    neff = np.ones(n)
    _capi.check(_capi.load().me_detect_equilibration(
        int(device), _capi.double_ptr(a), n, length, int(bool(fast)), int(nskip), _capi.int64_ptr(t0), _capi.double_ptr(g),
        _capi.double_ptr(neff)))
    return t0, g, neff


def validate_series_lags(n_records, mintime, max_lag):
    """``(mintime, max_lag)`` of a pooled inefficiency as ints: ``mintime >= 0``; ``max_lag`` in ``[1, n_records - 2]``, ``None``
    for ``n_records - 2``.  ``ValueError`` otherwise and for fewer than 3 records.  Runs before the library is touched."""
    if n_records < 3:
        raise ValueError("a statistical inefficiency needs at least 3 records, got %d" % n_records)
    if int(mintime) != mintime or int(mintime) < 0:
        raise ValueError("mintime must be an integer >= 0")
    if max_lag is None:
        max_lag = n_records - 2
    if int(max_lag) != max_lag or not 1 <= int(max_lag) <= n_records - 2:
        raise ValueError("max_lag must be an integer in [1, records - 2 = %d]" % (n_records - 2))
    return int(mintime), int(max_lag)


def _series_inefficiency(fn, lead, n_columns, n_groups, n_records, mintime, max_lag):
    """One call of either C form (``lead``: the engine's handle, or the device and the host array) and its dictionary."""
    shape = (n_columns, n_groups)
    g, mean, var = np.empty(shape), np.empty(shape), np.empty(shape)
    stop, used = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int64)
    acf = np.empty(shape + (max_lag + 1,))
    _call(fn, lead, mintime, max_lag, _capi.double_ptr(g), _capi.double_ptr(mean), _capi.double_ptr(var), _capi.int32_ptr(stop),
          _capi.int64_ptr(used), _capi.double_ptr(acf))
    return {"g": g, "tau": (g - 1.0) / 2.0, "mean": mean, "var": var, "stop_lag": stop, "chains_used": used, "acf": acf,
            "n_records": int(n_records)}


def series_inefficiency(series, group_chains=None, mintime=3, max_lag=None, device=0):
    """The statistical inefficiency ``g = 1 + 2 tau`` of MANY series of one stationary process, pooled over the series of a
    group, on the GPU (``me_series_inefficiency_samples``): the multiple-series estimator of Chodera et al., JCTC 3:26 (2007),
    pymbar's ``statisticalInefficiencyMultiple``.  ``series`` is ``(R, n_series)``, record-major like
    :meth:`MetropolisEngine.energy_samples`; the groups are consecutive runs of ``group_chains`` series (a multiple of 64 that
    divides ``n_series``; ``None``: one group).  A series is USED when all its ``R`` values are finite; over the ``M_u`` used
    series of a group, with ``d = a - mean``::

        mean = sum_c sum_n a_c[n] / (M_u R)            P(t) = sum_c sum_{n < R - t} d_c[n] d_c[n + t]
        var  = P(0) / (M_u R)                          C(t) = P(t) R / (P(0) (R - t))
        g    = max(1, 1 + 2 sum_{t = 1}^{stop - 1} C(t) (1 - t / R))

    with ``stop`` the first ``t > mintime`` at which ``C(t) <= 0``, or ``max_lag + 1`` when there is none up to ``max_lag``
    (``None``: ``R - 2``): for one series this is :func:`statistical_inefficiency` with ``fast=False``.  Returns ``{"g", "tau",
    "mean", "var", "stop_lag", "chains_used"}``, each ``(1, groups)`` (the leading axis is the column axis of
    :meth:`MetropolisEngine.recorded_inefficiency`), ``"acf"`` ``(1, groups, max_lag + 1)`` with ``C(t)`` up to ``min(stop,
    max_lag)`` and NaN beyond, and ``"n_records"``.  A group without a used series or with zero variance has ``g`` NaN.  Bitwise
    reproducible.  ``ValueError`` for fewer than 3 records and a bad ``group_chains``, ``mintime`` or ``max_lag``."""
    a = np.ascontiguousarray(series, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError("series must be (records, n_series)")
    n_records, n_series = a.shape
    mintime, max_lag = validate_series_lags(n_records, mintime, max_lag)
    if group_chains is None:
        group_chains = n_series
    group_chains = int(group_chains)
    if group_chains < 64 or group_chains % 64 or n_series % group_chains:
        raise ValueError("group_chains must be a multiple of 64 that divides n_series = %d" % n_series)
    return _series_inefficiency(_capi.load().me_series_inefficiency_samples,
                                (int(device), _capi.double_ptr(a), n_records, n_series, group_chains), 1, n_series // group_chains,
                                n_records, mintime, max_lag)


# ---------------------------------------------------------------------------------------------- MBAR over a ladder
# (no reference counterpart; the reference reaches for the same library family, pymbar, in its post-processing)
MBAR_MAX_RUNGS = 64


def validate_mbar_solve(tol, max_iter):
    """``(tol, max_iter)`` of an MBAR solve as ``(float, int)``; ``ValueError`` unless ``tol > 0`` (and finite) and
    ``max_iter >= 1``.  Runs before the library is touched."""
    tol = float(tol)
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("tol must be finite and > 0")
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")
    return tol, int(max_iter)


MBAR_METHODS = ("self-consistent", "newton")


def validate_mbar_method(method):
    """``method`` of an MBAR solve; ``ValueError`` unless it is one of ``MBAR_METHODS``.  Runs before the library is touched."""
    if method not in MBAR_METHODS:
        raise ValueError("method must be one of %s, not %r" % (", ".join(repr(m) for m in MBAR_METHODS), method))
    return method


def validate_mbar_temps(temps, what="temps"):
    """Temperatures as a contiguous 1-D float64 array: non-empty, finite and > 0 (``ValueError`` otherwise)."""
    t = np.ascontiguousarray(np.atleast_1d(np.asarray(temps, dtype=np.float64)))
    if t.ndim != 1 or t.size < 1:
        raise ValueError("%s must be a non-empty 1-D sequence" % what)
    if not np.all(np.isfinite(t)) or not np.all(t > 0):
        raise ValueError("%s must be finite and > 0" % what)
    return t


def validate_mbar_samples(energies, rungs, temps):
    """``(energies float64, rungs int32, temps float64)`` of the engine-less MBAR forms, flattened and checked: equal
    lengths, at least one sample, ``0 <= rung < len(temps) <= 64``.  Energies may be non-finite (they are skipped)."""
    t = validate_mbar_temps(temps, "temps")
    if t.size > MBAR_MAX_RUNGS:
        raise ValueError("MBAR supports at most %d rungs" % MBAR_MAX_RUNGS)
    e = np.ascontiguousarray(np.asarray(energies, dtype=np.float64).ravel())
    r = np.asarray(rungs).ravel()
    if e.size < 1 or r.size != e.size:
        raise ValueError("energies and rungs must have the same, non-zero, number of entries")
    if r.dtype.kind not in "iu":
        raise ValueError("rungs must be integers")
    if r.min() < 0 or r.max() >= t.size:
        raise ValueError("rungs must lie in [0, %d)" % t.size)
    return e, np.ascontiguousarray(r, dtype=np.int32), t


def validate_mbar_f(f, n_rungs, finite=True):
    """``f`` as a contiguous float64 array; ``ValueError`` unless it holds one free energy per rung, all of them finite when
    ``finite``.  ``n_rungs`` ``None`` (an engine without a ladder, which the library refuses): nothing to compare with."""
    f = np.ascontiguousarray(f, dtype=np.float64)
    if n_rungs is not None and (f.shape != (n_rungs,) or (finite and not np.all(np.isfinite(f)))):
        raise ValueError("f must hold one %sfree energy per rung" % ("finite " if finite else ""))
    return f


# One implementation per operation, below its result dictionary.  ``fn`` is the C function of either form and ``lead`` its
# leading arguments: ``(handle,)`` of an engine (``MetropolisEngine``), or the samples on the host (``_host_samples``).
def _call(fn, lead, *args):
    _capi.check(fn(*lead, *args), lead[0] if len(lead) == 1 else None)


def _host_samples(device, e, r, t, observables=None):
    columns = () if observables is None else (_capi.double_ptr(observables), observables.shape[0])
    return (int(device), _capi.double_ptr(e), _capi.int32_ptr(r), e.size) + columns + (_capi.double_ptr(t), t.size)


def _solve_result(f, iterations, residual, n_used, tol):
    return {"f": f, "ln_z": -f, "iterations": int(iterations), "residual": float(residual),
            "converged": bool(residual <= tol), "n_samples": n_used}


def _solve(fn, lead, n_rungs, tol, max_iter):
    f, n_used = np.zeros(n_rungs), np.zeros(n_rungs, dtype=np.int64)
    its, res = ctypes.c_int32(), ctypes.c_double()
    _call(fn, lead, tol, max_iter, _capi.double_ptr(f), ctypes.byref(its), ctypes.byref(res), _capi.int64_ptr(n_used))
    return _solve_result(f, its.value, res.value, n_used, tol)


def _solve_newton(fn, lead, n_rungs, tol, max_iter):
    """``_solve`` through ``me_mbar_solve_newton`` / ``_samples``: the same dictionary with ``gradient`` (``max_k |S_k / N_k -
    1|`` at the last pass), ``newton_steps`` and ``fallback_steps`` added."""
    f, n_used = np.zeros(n_rungs), np.zeros(n_rungs, dtype=np.int64)
    its, res, grad = ctypes.c_int32(), ctypes.c_double(), ctypes.c_double()
    newton, fallback = ctypes.c_int32(), ctypes.c_int32()
    _call(fn, lead, tol, max_iter, _capi.double_ptr(f), ctypes.byref(its), ctypes.byref(res), ctypes.byref(grad), ctypes.byref(newton),
          ctypes.byref(fallback), _capi.int64_ptr(n_used))
    out = _solve_result(f, its.value, res.value, n_used, tol)
    out.update(gradient=float(grad.value), newton_steps=int(newton.value), fallback_steps=int(fallback.value))
    return out


def _reweight_result(temps, ln_z, mean, var, neff):
    return {"temps": temps, "ln_z": ln_z, "energy_mean": mean, "energy_var": var, "heat_capacity": var / (temps * temps),
            "neff_fraction": neff}


def _reweight(fn, lead, f, targets):
    out = [np.zeros(targets.size) for _ in range(4)]
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, *map(_capi.double_ptr, out))
    return _reweight_result(targets, *out)


def mbar_free_energies(energies, rungs, temps, tol=1e-10, max_iter=10000, device=0, method="self-consistent"):
    """MBAR free energies of a temperature ladder from samples on the host (``me_mbar_solve_samples``; the engine form is
    ``MetropolisEngine.ladder_free_energies``).  ``energies[i]`` was sampled at ``temps[rungs[i]]``.  Returns
    ``{"f", "ln_z", "iterations", "residual", "converged", "n_samples"}``: ``f[k] = -ln Z(T_k) / Z(T_0)``, ``ln_z = -f``,
    ``n_samples[k]`` the finite energies of rung ``k`` (the others are skipped).  For samples gathered from several GPU
    shards and for subsets of a run; a rung without a finite sample raises.  ``method="newton"`` solves by Newton's method
    (``me_mbar_solve_newton_samples``: quadratic convergence, every pass over the samples an iteration) and adds ``gradient``,
    ``newton_steps`` and ``fallback_steps`` to the dictionary; any other ``method`` is a ``ValueError``."""
    method = validate_mbar_method(method)
    tol, max_iter = validate_mbar_solve(tol, max_iter)
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    if method == "newton":
        return _solve_newton(_capi.load().me_mbar_solve_newton_samples, _host_samples(device, e, r, t), t.size, tol, max_iter)
    return _solve(_capi.load().me_mbar_solve_samples, _host_samples(device, e, r, t), t.size, tol, max_iter)


def mbar_reweight(energies, rungs, temps, f, targets, device=0):
    """Reweight the samples of a ladder (``temps``, free energies ``f`` of :func:`mbar_free_energies`) to the temperatures
    ``targets`` (``me_mbar_reweight_samples``).  Returns ``{"temps", "ln_z", "energy_mean", "energy_var", "heat_capacity",
    "neff_fraction"}``: ``ln_z = ln Z(T) / Z(T_0)``, ``heat_capacity = energy_var / T^2``."""
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    return _reweight(_capi.load().me_mbar_reweight_samples, _host_samples(device, e, r, t), f, targets)


MBAR_MAX_OBSERVABLES = 16       # recorded / reweighted observable columns (ME_MAX_RECORDED_OBSERVABLES)


def observable_catalogue(n_real, n_complex, term_names):
    """The names of a chain's recordable quantities in the order of the C ABI: state rows (``real_i``, ``re_i``, ``im_i``),
    observables (``abs_real_i``, ``abs_complex_i``, ``real_i_sq``), ledger rows (``energy_<term name>``)."""
    nr, nc = int(n_real), int(n_complex)
    return (["real_%d" % i for i in range(nr)] + ["re_%d" % i for i in range(nc)] + ["im_%d" % i for i in range(nc)] +
            ["abs_real_%d" % i for i in range(nr)] + ["abs_complex_%d" % i for i in range(nc)] +
            ["real_%d_sq" % i for i in range(nr)] + ["energy_%s" % name for name in term_names])


def validate_observable_selection(which, catalogue):
    """``which`` (names of ``catalogue`` or indices into it, 1 to 16 of them, duplicates allowed) as int32 indices;
    ``ValueError`` otherwise."""
    if isinstance(which, (str, bytes)):
        which = [which]
    which = list(which)
    if not 1 <= len(which) <= MBAR_MAX_OBSERVABLES:
        raise ValueError("between 1 and %d observables can be recorded, got %d" % (MBAR_MAX_OBSERVABLES, len(which)))
    idx = []
    for w in which:
        if isinstance(w, str):
            if w not in catalogue:
                raise ValueError("unknown observable %r; this engine has %s" % (w, ", ".join(catalogue)))
            idx.append(catalogue.index(w))
        elif isinstance(w, (int, np.integer)) and not isinstance(w, bool):
            if not 0 <= int(w) < len(catalogue):
                raise ValueError("observable index %d outside the catalogue of %d quantities" % (int(w), len(catalogue)))
            idx.append(int(w))
        else:
            raise ValueError("observables are named by str or int, got %r" % (w,))
    return np.asarray(idx, dtype=np.int32)


def validate_mbar_observables(observables, n_samples):
    """``observables`` of the engine-less form as a contiguous float64 ``(Q, n_samples)`` array, ``1 <= Q <= 16`` (a 1-d
    array of ``n_samples`` entries is one column).  Values may be non-finite.  ``ValueError`` otherwise."""
    a = np.asarray(observables, dtype=np.float64)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim < 2:
        raise ValueError("observables must be (Q, n_samples)")
    a = a.reshape(a.shape[0], -1)
    if not 1 <= a.shape[0] <= MBAR_MAX_OBSERVABLES:
        raise ValueError("between 1 and %d observable columns are supported" % MBAR_MAX_OBSERVABLES)
    if a.shape[1] != n_samples:
        raise ValueError("every observable column needs one value per sample (%d), got %d" % (n_samples, a.shape[1]))
    return np.ascontiguousarray(a)


def _observable_result(temps, names, mean, var, cov, neff):
    return {"temps": temps, "names": tuple(names), "mean": mean, "var": var, "cov_energy": cov,
            "dmean_dT": cov / (temps * temps)[:, None], "neff_fraction": neff}


def _reweight_observables(fn, lead, f, targets, names):
    out = [np.zeros((targets.size, len(names))) for _ in range(3)] + [np.zeros(targets.size)]
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, *map(_capi.double_ptr, out))
    return _observable_result(targets, names, *out)


def mbar_reweight_observables(energies, rungs, temps, f, targets, observables, device=0):
    """Reweight observables sampled along with the energies of a ladder (``temps``, free energies ``f`` of
    :func:`mbar_free_energies`) to the temperatures ``targets`` (``me_mbar_reweight_observables_samples``; the engine form is
    ``MetropolisEngine.reweight_observables``).  ``observables``: ``(Q, n_samples)``, ``Q <= 16``, column ``q`` holding
    ``A_q`` of every sample in the order of ``energies``.  Returns ``{"temps", "names", "mean", "var", "cov_energy",
    "dmean_dT", "neff_fraction"}``: the first four ``(T, Q)``, ``dmean_dT = cov_energy / T^2``; ``names`` are the column
    numbers.  A sample counts when its ENERGY is finite; a non-finite value in column ``q`` of such a sample makes column
    ``q``'s results non-finite and changes no other column."""
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    a = validate_mbar_observables(observables, e.size)
    return _reweight_observables(_capi.load().me_mbar_reweight_observables_samples, _host_samples(device, e, r, t, a), f, targets,
                                 tuple(range(a.shape[0])))


def validate_mbar_couplings(couplings, n_targets, names):
    """``couplings`` of a perturbed reweighting as a contiguous float64 ``(P, Q)`` array, ``P = n_targets`` and ``Q =
    len(names)`` the columns in their order.  An array: ``(P, Q)``, or ``(Q,)`` for every target alike.  A dictionary: the keys
    are entries of ``names`` or column indices, the values scalars or ``(P,)``; columns it does not name are 0.  ``ValueError``
    for a shape mismatch, an unknown name or index, a column named twice (by its name and by its index, say) or a non-finite
    coupling.  Runs before the library is touched."""
    names = tuple(names)
    p, q = int(n_targets), len(names)
    if isinstance(couplings, dict):
        lam = np.zeros((p, q))
        seen = set()
        for key, value in couplings.items():
            if isinstance(key, (int, np.integer)) and not isinstance(key, bool):
                if not 0 <= int(key) < q:
                    raise ValueError("coupling index %d outside the %d columns" % (int(key), q))
                col = int(key)
            elif key in names:
                col = names.index(key)
            else:
                raise ValueError("unknown column %r; the columns are %s" % (key, ", ".join(map(str, names))))
            if col in seen:
                raise ValueError("column %r is coupled twice" % (names[col],))
            seen.add(col)
            v = np.asarray(value, dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.size != p):
                raise ValueError("the coupling of %r must be a scalar or hold one value per target (%d)" % (key, p))
            lam[:, col] = v
    else:
        lam = np.asarray(couplings, dtype=np.float64)
        if lam.ndim == 1 and lam.size == q:
            lam = np.broadcast_to(lam, (p, q))
        if lam.shape != (p, q):
            raise ValueError("couplings must be (targets = %d, columns = %d), got %s" % (p, q, lam.shape))
    if not np.all(np.isfinite(lam)):
        raise ValueError("couplings must be finite")
    return np.ascontiguousarray(lam, dtype=np.float64)


def broadcast_mbar_targets(temps, couplings):
    """``temps`` (a scalar or ``(P,)``) as ``(P,)`` for couplings that name ``P`` targets: one temperature serves them all.
    ``P`` is the length of ``temps`` unless that is 1, then the rows of a 2-d ``couplings`` or the longest value of a
    dictionary."""
    t = validate_mbar_temps(temps, "targets")
    if t.size == 1:
        if isinstance(couplings, dict):
            p = max([np.asarray(v).size for v in couplings.values() if np.ndim(v) == 1] + [1])
        else:
            p = np.shape(couplings)[0] if np.ndim(couplings) == 2 else 1
        t = np.ascontiguousarray(np.broadcast_to(t, (max(p, 1),)))
    return t


def _perturbed_result(temps, couplings, names, ln_z, mean_h, var_h, mean, var, cov, neff):
    t2 = temps * temps
    return {"temps": temps, "couplings": couplings, "names": tuple(names), "ln_z": ln_z, "hamiltonian_mean": mean_h,
            "hamiltonian_var": var_h, "heat_capacity": var_h / t2,
            "perturbation_mean": np.array([sum(row[q] * m[q] for q in np.flatnonzero(row)) for row, m in zip(couplings, mean)],
                                          dtype=np.float64),
            "mean": mean, "var": var, "cov_hamiltonian": cov, "dmean_dT": cov / t2[:, None], "neff_fraction": neff}


def _reweight_perturbed(fn, lead, f, targets, couplings, names, columns=()):
    """``columns``: the trailing ``(observables, n_observables)`` of the engine-less form."""
    out = [np.zeros(targets.size) for _ in range(3)] + [np.zeros((targets.size, len(names))) for _ in range(3)] + [np.zeros(targets.size)]
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), _capi.double_ptr(couplings), targets.size, *columns,
          *map(_capi.double_ptr, out))
    return _perturbed_result(targets, couplings, names, *out)


def mbar_reweight_perturbed(energies, rungs, temps, f, targets, couplings, observables, device=0):
    """Reweight the samples of a ladder (``temps``, free energies ``f`` of :func:`mbar_free_energies`) to states that differ
    by more than their temperature (``me_mbar_reweight_perturbed_samples``; the engine form is
    ``MetropolisEngine.reweight_perturbed``): target ``p`` has the temperature ``targets[p]`` (a scalar serves every target)
    and the energy ``H = E + sum_q couplings[p, q] A_q`` over the columns ``A_q`` of ``observables`` ``(Q, n_samples)``.
    ``couplings``: see :func:`validate_mbar_couplings` (the names of the columns are their numbers).  Returns ``{"temps",
    "couplings" (P, Q), "names", "ln_z", "hamiltonian_mean", "hamiltonian_var", "heat_capacity", "perturbation_mean", "mean",
    "var", "cov_hamiltonian", "dmean_dT", "neff_fraction"}``: ``ln_z = ln Z(T, lambda) / Z(T_0, 0)`` (the zero of
    :func:`mbar_reweight`), the mean and variance of ``H``, ``heat_capacity = hamiltonian_var / T^2``, ``perturbation_mean =
    sum_q lambda_q mean_q``, the mean and variance of every column and its covariance with ``H`` ``(P, Q)``, ``dmean_dT =
    cov_hamiltonian / T^2``.  A column whose coupling is exactly 0 never enters ``H``; a non-finite value in a coupled column
    of a used sample makes every result of that target non-finite and changes no other target."""
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = broadcast_mbar_targets(targets, couplings)
    f = validate_mbar_f(f, t.size)
    a = validate_mbar_observables(observables, e.size)
    names = tuple(range(a.shape[0]))
    lam = validate_mbar_couplings(couplings, targets.size, names)
    return _reweight_perturbed(_capi.load().me_mbar_reweight_perturbed_samples, _host_samples(device, e, r, t), f, targets, lam, names,
                               (_capi.double_ptr(a), a.shape[0]))


MBAR_MAX_HISTOGRAM_BINS = 256   # bins of a reweighted histogram (ME_MAX_HISTOGRAM_BINS)


def validate_histogram_edges(edges):
    """Bin edges as a contiguous 1-D float64 array: between 2 and 257 of them (1 to 256 bins), finite and strictly
    increasing, any spacing (``ValueError`` otherwise)."""
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
    if e.ndim != 1 or not 1 <= e.size - 1 <= MBAR_MAX_HISTOGRAM_BINS:
        raise ValueError("edges must be a 1-D sequence of 2 to %d entries (1 to %d bins)"
                         % (MBAR_MAX_HISTOGRAM_BINS + 1, MBAR_MAX_HISTOGRAM_BINS))
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("edges must be finite and strictly increasing")
    return e


def _profile_result(temps, edges, mass, counts, neff):
    b = edges.size - 1
    widths = np.diff(edges)
    density = mass[:, :b] / widths[None, :]
    with np.errstate(divide="ignore"):
        free_energy = -temps[:, None] * np.log(density)
    free_energy[mass[:, :b] == 0] = np.inf
    return {"temps": temps, "edges": edges, "centers": 0.5 * (edges[:-1] + edges[1:]), "widths": widths,
            "mass": mass[:, :b].copy(), "below": mass[:, b].copy(), "above": mass[:, b + 1].copy(),
            "not_a_number": mass[:, b + 2].copy(), "density": density, "free_energy": free_energy,
            "counts": counts[:b].copy(), "counts_outside": counts[b:].copy(), "neff_fraction": neff}


def _free_energy_profile(fn, lead, f, targets, middle, edges):
    """``middle``: the arguments between the target count and the edges (the engine's column; the host form's values)."""
    b = edges.size - 1
    mass, counts, neff = np.zeros((targets.size, b + 3)), np.zeros(b + 3, dtype=np.int64), np.zeros(targets.size)
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, *middle, _capi.double_ptr(edges), b,
          _capi.double_ptr(mass), _capi.int64_ptr(counts), _capi.double_ptr(neff))
    return _profile_result(targets, edges, mass, counts, neff)


def mbar_free_energy_profile(energies, rungs, temps, f, targets, values, edges, device=0):
    """The reweighted histogram of ``values`` (one value ``A`` per sample, in the order of ``energies``) and the free-energy
    profile ``F(A; T) = -T ln p(A; T)`` along it at the temperatures ``targets``, from the samples of a ladder (``temps``,
    free energies ``f`` of :func:`mbar_free_energies`) on the host (``me_mbar_histogram_samples``; the engine form is
    ``MetropolisEngine.free_energy_profile``).  ``edges``: 2 to 257 finite, strictly increasing bin edges of any spacing.

    Every sample with a finite ENERGY falls into exactly one slot: bin ``b`` when ``edges[b] <= A < edges[b + 1]`` (half-open
    everywhere), *below* when ``A < edges[0]``, *above* when ``A >= edges[-1]``, *not a number* when ``A`` is NaN -- the rule
    ``np.searchsorted(edges, A, side="right") - 1``.  A value equal to the LAST edge is *above*: unlike ``np.histogram``, the
    last bin is not closed on the right.

    Returns ``{"temps", "edges", "centers", "widths", "mass", "below", "above", "not_a_number", "density", "free_energy",
    "counts", "counts_outside", "neff_fraction"}``: ``mass`` ``(T, B)`` the reweighted probability of every bin, ``below``,
    ``above`` and ``not_a_number`` ``(T,)`` that of the three outer slots (all of them together sum to 1), ``density = mass /
    widths``, ``free_energy = -T ln density`` (``+inf`` where the mass is 0), ``counts`` ``(B,)`` the samples per bin and
    ``counts_outside`` ``(3,)`` those below, above and not a number, ``neff_fraction`` as :func:`mbar_reweight`'s.  The sums
    have a fixed order: bitwise reproducible, and a temperature's row does not depend on which others are asked for."""
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    edges = validate_histogram_edges(edges)
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel())
    if a.size != e.size:
        raise ValueError("values needs one entry per sample (%d), got %d" % (e.size, a.size))
    return _free_energy_profile(_capi.load().me_mbar_histogram_samples, _host_samples(device, e, r, t), f, targets,
                                (_capi.double_ptr(a),), edges)


MBAR_MAX_HISTOGRAM2D_SLOTS = 1296       # cells (Bx + 3)(By + 3) of a joint histogram: 33 x 33 bins (ME_MAX_HISTOGRAM2D_SLOTS)


def validate_histogram2d_edges(edges_x, edges_y):
    """The edges of both axes of a joint histogram, each as :func:`validate_histogram_edges` returns them; ``ValueError`` also
    when the ``(Bx + 3)(By + 3)`` cells exceed 1296 (33 x 33 bins)."""
    ex, ey = validate_histogram_edges(edges_x), validate_histogram_edges(edges_y)
    if (ex.size + 2) * (ey.size + 2) > MBAR_MAX_HISTOGRAM2D_SLOTS:
        raise ValueError("a joint histogram holds at most %d cells (Bx + 3)(By + 3), e.g. 33 x 33 bins; got %d x %d bins"
                         % (MBAR_MAX_HISTOGRAM2D_SLOTS, ex.size - 1, ey.size - 1))
    return ex, ey


def _surface_result(temps, edges_x, edges_y, mass, counts, neff):
    """``mass`` ``(T, Bx + 3, By + 3)`` and ``counts`` ``(Bx + 3, By + 3)`` as ``me_mbar_histogram_joint`` returns them."""
    bx, by = edges_x.size - 1, edges_y.size - 1
    widths_x, widths_y = np.diff(edges_x), np.diff(edges_y)
    inner = mass[:, :bx, :by].copy()
    density = inner / (widths_x[:, None] * widths_y[None, :])
    with np.errstate(divide="ignore"):
        free_energy = -temps[:, None, None] * np.log(density)
    free_energy[inner == 0] = np.inf
    # every cell outside the inner grid, in a fixed order: the outer rows (below, above, NaN on x), then the outer columns of
    # the inner rows
    outside = mass[:, bx:, :].reshape(temps.size, -1).sum(axis=1) + mass[:, :bx, by:].reshape(temps.size, -1).sum(axis=1)
    return {"temps": temps, "edges_x": edges_x, "edges_y": edges_y, "centers_x": 0.5 * (edges_x[:-1] + edges_x[1:]),
            "centers_y": 0.5 * (edges_y[:-1] + edges_y[1:]), "widths_x": widths_x, "widths_y": widths_y, "mass": inner,
            "density": density, "free_energy": free_energy, "mass_slots": mass, "outside": outside,
            "counts": counts[:bx, :by].copy(), "counts_slots": counts, "neff_fraction": neff}


def _free_energy_surface(fn, lead, f, targets, middle_x, edges_x, middle_y, edges_y):
    """``middle_x`` / ``middle_y``: the engine form's column of an axis, given in front of that axis's edges (the host form passes
    both value arrays in ``middle_x`` and nothing in ``middle_y``)."""
    bx, by = edges_x.size - 1, edges_y.size - 1
    mass, counts = np.zeros((targets.size, bx + 3, by + 3)), np.zeros((bx + 3, by + 3), dtype=np.int64)
    neff = np.zeros(targets.size)
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, *middle_x, _capi.double_ptr(edges_x), bx,
          *middle_y, _capi.double_ptr(edges_y), by, _capi.double_ptr(mass), _capi.int64_ptr(counts), _capi.double_ptr(neff))
    return _surface_result(targets, edges_x, edges_y, mass, counts, neff)


def mbar_free_energy_surface(energies, rungs, temps, f, targets, values_x, edges_x, values_y, edges_y, device=0):
    """The joint reweighted histogram of ``values_x`` and ``values_y`` (one value of each per sample, in the order of
    ``energies``) and the free-energy surface ``F(A, B; T) = -T ln p(A, B; T)`` at the temperatures ``targets``, from the samples
    of a ladder (``temps``, free energies ``f`` of :func:`mbar_free_energies`) on the host (``me_mbar_histogram_joint_samples``; the
    engine form is ``MetropolisEngine.free_energy_surface``).  Each axis has edges of its own as in
    :func:`mbar_free_energy_profile`, and the ``(Bx + 3)(By + 3)`` cells may not exceed 1296 (33 x 33 bins).

    Every sample with a finite ENERGY falls into exactly one cell ``(slot_x, slot_y)``, each slot by the rule of
    :func:`mbar_free_energy_profile` along its axis: the bins, then *below*, *above* (a value ON the last edge is above) and
    *not a number*.

    Returns ``{"temps", "edges_x", "edges_y", "centers_x", "centers_y", "widths_x", "widths_y", "mass", "density",
    "free_energy", "mass_slots", "outside", "counts", "counts_slots", "neff_fraction"}``: ``mass`` ``(T, Bx, By)`` the
    reweighted probability of every cell of the inner grid, ``density = mass / (widths_x[:, None] * widths_y[None, :])``,
    ``free_energy = -T ln density`` (``+inf`` where the mass is 0), ``mass_slots`` ``(T, Bx + 3, By + 3)`` the full table (it
    sums to 1; its sums over an axis are the 1-D masses of the other with their below / above / NaN slots), ``outside``
    ``(T,)`` the mass outside the inner grid, ``counts`` ``(Bx, By)`` and ``counts_slots`` ``(Bx + 3, By + 3)`` the samples per
    cell, ``neff_fraction`` as :func:`mbar_reweight`'s.  The sums have a fixed order: bitwise reproducible, and a temperature's
    table does not depend on which others are asked for."""
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    edges_x, edges_y = validate_histogram2d_edges(edges_x, edges_y)
    a = np.ascontiguousarray(np.asarray(values_x, dtype=np.float64).ravel())
    b = np.ascontiguousarray(np.asarray(values_y, dtype=np.float64).ravel())
    if a.size != e.size or b.size != e.size:
        raise ValueError("values_x and values_y need one entry per sample (%d), got %d and %d" % (e.size, a.size, b.size))
    return _free_energy_surface(_capi.load().me_mbar_histogram_joint_samples, _host_samples(device, e, r, t), f, targets,
                                (_capi.double_ptr(a), _capi.double_ptr(b)), edges_x, (), edges_y)


MBAR_GRAM_MAX_COLUMNS = 128     # columns of the weight matrix per device pass (csrc/me_mbar_cov.hip)


def validate_mbar_inefficiency(inefficiency):
    """The statistical inefficiency that scales the asymptotic variances: a finite scalar ``>= 1`` (``ValueError``
    otherwise)."""
    g = float(inefficiency)
    if not (np.isfinite(g) and g >= 1.0):
        raise ValueError("inefficiency must be finite and >= 1")
    return g


def mbar_theta(gram, column_counts):
    """The asymptotic covariance matrix of MBAR from the Gram matrix ``G = W^T W`` of the weight matrix (Shirts & Chodera,
    J. Chem. Phys. 129:124105, 2008, eq. D8 through the eigendecomposition of ``G``): ``G = V diag(lam) V^T``, ``lam``
    clamped at 0, ``S = diag(sqrt(lam))``, ``Theta = V S (I - S V^T diag(N) V S)^+ S V^T`` with the pseudo-inverse cut at
    ``rcond = 1e-10``.  Host float64."""
    g = np.asarray(gram, dtype=np.float64)
    n = np.asarray(column_counts, dtype=np.float64)
    lam, v = np.linalg.eigh(g)
    sv = v * np.sqrt(np.clip(lam, 0.0, None))[None, :]
    m = np.eye(lam.size) - sv.T @ (n[:, None] * sv)
    return sv @ np.linalg.pinv(m, rcond=1e-10) @ sv.T


def _uncertainty_result(gram, column_counts, n_rungs, targets, ln_z, mean_e, n_used, inefficiency, energy_shift):
    """The dictionary of :func:`mbar_uncertainties` from what ``me_mbar_gram`` returns.  Targets are taken in the chunks the
    device used (each with the ladder columns): the blocks of ``gram`` between chunks are not computed.  ``energy_shift`` =
    the least finite energy - 1, the shift of the energy columns."""
    k = n_rungs
    n_targets = 0 if targets is None else targets.size
    per = (MBAR_GRAM_MAX_COLUMNS - k) // 2
    out = {"n_samples": int(n_used)}
    d_ln_z, d_mean = np.zeros(n_targets), np.zeros(n_targets)
    for t0 in range(0, max(n_targets, 1), per):
        nt = min(per, n_targets - t0)
        idx = np.concatenate([np.arange(k), k + 2 * t0 + np.arange(2 * nt)]).astype(np.intp)
        theta = mbar_theta(gram[np.ix_(idx, idx)], column_counts[idx])
        if t0 == 0:
            diag = np.diag(theta)[:k]
            out["theta"] = theta[:k, :k] * inefficiency
            var = diag[:, None] + diag[None, :] - 2.0 * theta[:k, :k]
            out["d_f_matrix"] = np.sqrt(np.clip(var, 0.0, None) * inefficiency)
            np.fill_diagonal(out["d_f_matrix"], 0.0)
            out["d_f"] = out["d_f_matrix"][:, 0].copy()
        for t in range(nt):
            a, b = k + 2 * t, k + 2 * t + 1
            var_z = theta[a, a] + theta[0, 0] - 2.0 * theta[a, 0]
            var_e = theta[b, b] + theta[a, a] - 2.0 * theta[b, a]
            d_ln_z[t0 + t] = np.sqrt(max(var_z, 0.0) * inefficiency)
            # (the energy column holds E - E_shift, whose mean is mean_e - E_shift; the shift drops out of the variance)
            d_mean[t0 + t] = (mean_e[t0 + t] - energy_shift) * np.sqrt(max(var_e, 0.0) * inefficiency)
    if n_targets:
        out.update({"temps": targets, "ln_z": ln_z, "d_ln_z": d_ln_z, "energy_mean": mean_e, "d_energy_mean": d_mean})
    return out


def _uncertainties(fn, lead, n_rungs, f, targets, inefficiency, energy_shift):
    """``energy_shift()``: the least finite energy - 1; asked for after the Gram matrix, and only with ``targets``."""
    n_targets = 0 if targets is None else targets.size
    c = n_rungs + 2 * n_targets
    gram, counts = np.zeros((c, c)), np.zeros(c)
    ln_z, mean_e = np.zeros(n_targets), np.zeros(n_targets)
    n_used = ctypes.c_int64()
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets) if n_targets else None, n_targets, _capi.double_ptr(gram),
          _capi.double_ptr(counts), _capi.double_ptr(ln_z), _capi.double_ptr(mean_e), ctypes.byref(n_used))
    shift = energy_shift() if n_targets else 0.0
    return _uncertainty_result(gram, counts, n_rungs, targets, ln_z, mean_e, n_used.value, inefficiency, shift)


def mbar_uncertainties(energies, rungs, temps, f, targets=None, inefficiency=1.0, device=0):
    """Asymptotic standard errors of MBAR free energies and of reweighted energies from samples on the host
    (``me_mbar_gram_samples``: one further pass over the samples builds the Gram matrix of the weight matrix on the matrix
    cores; the C x C algebra of Shirts & Chodera 2008, eqs. 8 and D8, runs here in float64; the engine form is
    ``MetropolisEngine.ladder_free_energy_uncertainties``).  ``f``: the converged free energies of
    :func:`mbar_free_energies`.  Returns ``{"theta", "d_f", "d_f_matrix", "n_samples"}``: the K x K ladder block of the
    covariance matrix, the standard error of ``f[k] - f[0]`` (``d_f[0] == 0``) and of every ``f[i] - f[j]``, and the number
    of finite samples; with ``targets`` also ``{"temps", "ln_z", "d_ln_z", "energy_mean", "d_energy_mean"}``, the values of
    :func:`mbar_reweight` with their standard errors.

    The asymptotic formula assumes INDEPENDENT samples.  For correlated samples pass their statistical inefficiency
    (:func:`statistical_inefficiency` of the energy series, ``>= 1``) as ``inefficiency``: every variance is multiplied by
    it, the customary correction.  ``ValueError`` for an ``inefficiency`` that is not a finite scalar ``>= 1``."""
    g = validate_mbar_inefficiency(inefficiency)
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    if targets is not None:
        targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    return _uncertainties(_capi.load().me_mbar_gram_samples, _host_samples(device, e, r, t), t.size, f, targets, g,
                          lambda: e[np.isfinite(e)].min() - 1.0)


def validate_mbar_observable_inefficiency(inefficiency, n_columns):
    """The statistical inefficiencies of ``n_columns`` observables as a ``(n_columns,)`` float64 array: a scalar (every
    column's) or one entry per column, each validated like :func:`validate_mbar_inefficiency` (``ValueError`` otherwise)."""
    g = np.asarray(inefficiency, dtype=np.float64)
    if g.ndim > 1 or (g.ndim == 1 and g.shape != (n_columns,)):
        raise ValueError("inefficiency must be a scalar or hold one entry per observable column (%d)" % n_columns)
    return np.array([validate_mbar_inefficiency(v) for v in np.broadcast_to(g, (n_columns,))])


def _observable_uncertainty_result(gram, column_counts, n_rungs, targets, names, ln_z, mean, shifts, n_used, inefficiency):
    """The dictionary of :func:`mbar_observable_uncertainties` from what ``me_mbar_gram_observables`` returns.  Targets are taken
    in the chunks the device used (each with the ladder columns), each chunk on those of its columns whose entries of ``gram``
    are finite: a poisoned observable column (its mean is not finite) drops out of the algebra and gets NaN."""
    k, q, n_targets = n_rungs, len(names), targets.size
    per = (MBAR_GRAM_MAX_COLUMNS - k) // (1 + q)
    d_ln_z = np.zeros(n_targets)
    d_mean, mean_cov = np.full((n_targets, q), np.nan), np.full((n_targets, q, q), np.nan)
    root_g = np.sqrt(inefficiency)
    for t0 in range(0, n_targets, per):
        nt = min(per, n_targets - t0)
        idx = np.concatenate([np.arange(k), k + (1 + q) * t0 + np.arange((1 + q) * nt)]).astype(np.intp)
        idx = idx[np.isfinite(np.diag(gram)[idx])]
        at = {int(c): i for i, c in enumerate(idx)}      # column of gram -> row of theta
        theta = mbar_theta(gram[np.ix_(idx, idx)], column_counts[idx])
        for t in range(t0, t0 + nt):
            a = at[k + (1 + q) * t]
            d_ln_z[t] = np.sqrt(max(theta[a, a] + theta[0, 0] - 2.0 * theta[a, 0], 0.0) * inefficiency.max())
            own = [c for c in range(q) if k + (1 + q) * t + 1 + c in at]
            rows = np.array([at[k + (1 + q) * t + 1 + c] for c in own], dtype=np.intp)
            if rows.size == 0:
                continue
            own = np.array(own, dtype=np.intp)
            # (column A holds A_q - S_q, whose mean is mean_tq - S_q; the shift drops out of the covariance)
            scale = (mean[t, own] - shifts[own]) * root_g[own]
            cov = theta[np.ix_(rows, rows)] + theta[a, a] - theta[rows, a][:, None] - theta[rows, a][None, :]
            mean_cov[np.ix_([t], own, own)] = scale[:, None] * scale[None, :] * cov
            d_mean[t, own] = np.abs(scale) * np.sqrt(np.clip(np.diag(cov), 0.0, None))
    return {"temps": targets, "names": tuple(names), "mean": mean, "d_mean": d_mean, "mean_cov": mean_cov, "ln_z": ln_z,
            "d_ln_z": d_ln_z, "n_samples": int(n_used)}


def _observable_uncertainties(fn, lead, n_rungs, f, targets, names, inefficiency):
    q = len(names)
    c = n_rungs + targets.size * (1 + q)
    gram, counts = np.zeros((c, c)), np.zeros(c)
    ln_z, mean, shifts = np.zeros(targets.size), np.zeros((targets.size, q)), np.zeros(q)
    n_used = ctypes.c_int64()
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, _capi.double_ptr(gram), _capi.double_ptr(counts),
          _capi.double_ptr(ln_z), _capi.double_ptr(mean), _capi.double_ptr(shifts), ctypes.byref(n_used))
    return _observable_uncertainty_result(gram, counts, n_rungs, targets, names, ln_z, mean, shifts, n_used.value, inefficiency)


def mbar_observable_uncertainties(energies, rungs, temps, f, targets, observables, inefficiency=1.0, device=0):
    """Asymptotic standard errors of the reweighted means of :func:`mbar_reweight_observables`
    (``me_mbar_gram_observables_samples``: the Gram matrix of the MBAR weight matrix with one observable-weighted column per
    target and column, on the matrix cores; the algebra of Shirts & Chodera 2008, eqs. 8, 12-15 and D8, runs here in float64;
    the engine form is ``MetropolisEngine.observable_uncertainties``).  Returns ``{"temps", "names", "mean" (T, Q), "d_mean" (T,
    Q), "mean_cov" (T, Q, Q), "ln_z", "d_ln_z", "n_samples"}``: ``mean`` is :func:`mbar_reweight_observables`' (bit for bit when
    every energy is finite), ``d_mean`` its standard error and ``mean_cov[t]`` the covariance matrix of the Q ESTIMATES at
    target ``t`` -- what the error bar of a ratio or a difference of two observables needs; ``d_mean ** 2`` is its diagonal.

    The formula assumes INDEPENDENT samples: pass the statistical inefficiency ``g >= 1`` of the series as ``inefficiency``, a
    scalar or one entry per column; ``d_mean[:, q]`` is multiplied by ``sqrt(g_q)``, ``mean_cov[:, q, r]`` by ``sqrt(g_q
    g_r)`` and ``d_ln_z`` by the square root of the largest.  A non-finite value of column ``q`` in a used sample gives NaN in
    ``mean[:, q]``, ``d_mean[:, q]`` and row and column ``q`` of ``mean_cov``, and nothing else."""
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    a = validate_mbar_observables(observables, e.size)
    g = validate_mbar_observable_inefficiency(inefficiency, a.shape[0])
    lead = _host_samples(device, e, r, t) + (_capi.double_ptr(a), a.shape[0])
    return _observable_uncertainties(_capi.load().me_mbar_gram_observables_samples, lead, t.size, f, targets,
                                     tuple(range(a.shape[0])), g)


def validate_mbar_fluctuation_observables(observables, n_samples):
    """``observables`` of :func:`mbar_fluctuation_uncertainties`: ``None`` (no column: a ``(0, n_samples)`` array) or what
    :func:`validate_mbar_observables` accepts."""
    if observables is None:
        return np.zeros((0, n_samples))
    return validate_mbar_observables(observables, n_samples)


def _fluctuation_uncertainty_result(gram, column_counts, n_rungs, targets, names, energy, observables, moments, n_used, inefficiency):
    """The dictionary of :func:`mbar_fluctuation_uncertainties` from what ``me_mbar_gram_fluctuations`` returns: ``energy`` =
    ``(mean_e, var_e)``, each ``(T,)``, ``observables`` = ``(mean, var, cov_energy)``, each ``(T, Q)``, ``moments`` ``(T, 2 + 3
    Q)`` the shifted moments ``m_i`` that normalise the columns ``E', E'^2`` and ``A'_q, A'_q^2, A'_q E'`` of each target.  With
    Theta of :func:`mbar_theta` and ``a`` the state column of the target, the covariance of the estimated moments is ``C_ij =
    m_i m_j (Theta_ij + Theta_aa - Theta_ia - Theta_ja)`` and a variance is ``g^T C g`` with the gradient ``g`` of the quantity
    (delta method): ``(-2 m_E, 1)`` on ``(E', E'^2)`` for the energy variance, ``(-2 m_A, 1)`` on ``(A', A'^2)`` for an
    observable's, ``(1, -m_E, -m_A)`` on ``(A' E', A', E')`` for its energy covariance; the shifts drop out.  Targets are taken in
    the chunks the device used, each chunk on those of its columns whose entries of ``gram`` are finite, as in
    :func:`_observable_uncertainty_result`: a poisoned observable drops out of the algebra and gets NaN."""
    k, q, n_targets = n_rungs, len(names), targets.size
    width = 3 + 3 * q
    per = (MBAR_GRAM_MAX_COLUMNS - k) // width
    mean_e, var_e = energy
    mean, var, cov = observables
    d_energy = np.full((2, n_targets), np.nan)
    d_obs = np.full((3, n_targets, q), np.nan)
    root_g = np.sqrt(inefficiency)

    def sigma(theta, a, rows, m, gradient):
        c = theta[np.ix_(rows, rows)] + theta[a, a] - theta[rows, a][:, None] - theta[rows, a][None, :]
        gm = np.asarray(gradient, dtype=np.float64) * m
        return np.sqrt(max(float(gm @ c @ gm), 0.0)) * root_g

    for t0 in range(0, n_targets, per):
        nt = min(per, n_targets - t0)
        idx = np.concatenate([np.arange(k), k + width * t0 + np.arange(width * nt)]).astype(np.intp)
        idx = idx[np.isfinite(np.diag(gram)[idx])]
        at = {int(c): i for i, c in enumerate(idx)}      # column of gram -> row of theta
        theta = mbar_theta(gram[np.ix_(idx, idx)], column_counts[idx])
        for t in range(t0, t0 + nt):
            base = k + width * t
            a, e1, e2 = at[base], at[base + 1], at[base + 2]
            m_e, m_e2 = moments[t, 0], moments[t, 1]
            d_energy[0, t] = sigma(theta, a, [e1], [m_e], [1.0])
            d_energy[1, t] = sigma(theta, a, [e1, e2], [m_e, m_e2], [-2.0 * m_e, 1.0])
            for c in range(q):
                if base + 3 + 3 * c not in at:
                    continue
                a1, a2, ae = (at[base + 3 + 3 * c + j] for j in range(3))
                m_a, m_a2, m_ae = moments[t, 2 + 3 * c:5 + 3 * c]
                d_obs[0, t, c] = sigma(theta, a, [a1], [m_a], [1.0])
                d_obs[1, t, c] = sigma(theta, a, [a1, a2], [m_a, m_a2], [-2.0 * m_a, 1.0])
                d_obs[2, t, c] = sigma(theta, a, [ae, a1, e1], [m_ae, m_a, m_e], [1.0, -m_e, -m_a])
    t_sq = targets * targets
    return {"temps": targets, "names": tuple(names), "n_samples": int(n_used),
            "energy_mean": mean_e, "d_energy_mean": d_energy[0], "energy_var": var_e, "d_energy_var": d_energy[1],
            "heat_capacity": var_e / t_sq, "d_heat_capacity": d_energy[1] / t_sq,
            "mean": mean, "d_mean": d_obs[0], "var": var, "d_var": d_obs[1], "cov_energy": cov, "d_cov_energy": d_obs[2],
            "dmean_dT": cov / t_sq[:, None], "d_dmean_dT": d_obs[2] / t_sq[:, None]}


def _fluctuation_uncertainties(fn, lead, n_rungs, f, targets, names, inefficiency):
    q, n = len(names), targets.size
    c = n_rungs + n * (3 + 3 * q)
    gram, counts = np.zeros((c, c)), np.zeros(c)
    ln_z, moments, shift, shifts = np.zeros(n), np.zeros((n, 2 + 3 * q)), np.zeros(1), np.zeros(max(q, 1))
    energy = [np.zeros(n) for _ in range(2)]
    observables = [np.zeros((n, q)) for _ in range(3)]
    n_used = ctypes.c_int64()
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), n, _capi.double_ptr(gram), _capi.double_ptr(counts),
          _capi.double_ptr(ln_z), _capi.double_ptr(moments), _capi.double_ptr(shift), _capi.double_ptr(shifts),
          *map(_capi.double_ptr, energy), *(_capi.double_ptr(a) if q else None for a in observables), ctypes.byref(n_used))
    return _fluctuation_uncertainty_result(gram, counts, n_rungs, targets, names, energy, observables, moments, n_used.value,
                                           inefficiency)


def mbar_fluctuation_uncertainties(energies, rungs, temps, f, targets, observables=None, inefficiency=1.0, device=0):
    """Asymptotic standard errors of the reweighted SECOND moments: the energy variance and the heat capacity of
    :func:`mbar_reweight`, and the variances, energy covariances and temperature derivatives of
    :func:`mbar_reweight_observables` (``me_mbar_gram_fluctuations_samples``: the Gram matrix of the MBAR weight matrix with the
    columns ``E', E'^2`` and, per observable, ``A', A'^2, A' E'`` of every target, the products formed in registers on the way
    to the matrix cores; the algebra of Shirts & Chodera 2008, eqs. 8 and D8, and the delta method run here in float64; the
    engine form is ``MetropolisEngine.fluctuation_uncertainties``).  ``observables``: ``(Q, n_samples)``, ``Q <= 16``, or
    ``None`` for the energy keys alone.  Returns ``{"temps", "names", "n_samples"}``, ``{"energy_mean", "energy_var",
    "heat_capacity"}`` ``(T,)`` and ``{"mean", "var", "cov_energy", "dmean_dT"}`` ``(T, Q)`` -- the values of the two reweighting
    functions, bit for bit when every energy is finite -- and the standard error of each under ``"d_" + key``.

    The formula assumes INDEPENDENT samples: pass the statistical inefficiency of the series, a finite scalar ``>= 1``, as
    ``inefficiency``; it multiplies every variance (``ValueError`` otherwise).  A non-finite value of column ``q`` in a used
    sample gives NaN in that column's four values and errors, and nothing else."""
    g = validate_profile_inefficiency(inefficiency)
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    a = validate_mbar_fluctuation_observables(observables, e.size)
    lead = _host_samples(device, e, r, t) + (_capi.double_ptr(a) if a.shape[0] else None, a.shape[0])
    return _fluctuation_uncertainties(_capi.load().me_mbar_gram_fluctuations_samples, lead, t.size, f, targets,
                                      tuple(range(a.shape[0])), g)


def _ladder_response(ladder_gram, column_counts):
    """``M = N^{1/2} (I - N^{1/2} G_KK N^{1/2})^+ N^{1/2}`` (K x K; the pseudo-inverse cut at ``rcond = 1e-10`` as in
    :func:`mbar_theta`): what is left of MBAR's asymptotic covariance for columns of the weight matrix that have no samples of
    their own.  For two such columns ``a``, ``b`` with Gram entries ``G_ab`` and ``G_Ka``, ``G_Kb`` against the ladder,
    ``Theta_ab = G_ab + G_Ka^T M G_Kb``."""
    root = np.sqrt(np.asarray(column_counts, dtype=np.float64))
    g = np.asarray(ladder_gram, dtype=np.float64)
    inner = np.eye(root.size) - root[:, None] * g * root[None, :]
    return root[:, None] * np.linalg.pinv(inner, rcond=1e-10) * root[None, :]


class _SlotLogCovariance:
    """The asymptotic covariance of the log masses of ONE temperature's slots (the bins of a profile with their three outer
    slots, the cells of a surface), from the slot Gram sums ``H`` ``(K + 1, S)``, the masses ``p`` ``(S,)`` and ``M`` of
    :func:`_ladder_response`.  The ``(K + 1 + S)``-column Gram matrix [ladder | state | one indicator column per slot] is NOT
    assembled: the state and slot columns have no samples of their own and the slot columns are disjoint, so with
        ``u_c = H[:K, c] / p_c - sum_c' H[:K, c']``,   ``h_c = H[K][c] / p_c``,
    ``Cov(ln p_c, ln p_c') = delta_cc' H[K][c] / p_c^2 - h_c - h_c' + sum_c'' H[K][c''] + u_c^T M u_c'``.  (``N^{1/2} u_c`` is
    orthogonal to the null vector ``N^{1/2} 1`` of the bracket because ``sum_j N_j W_nj = 1``: the cut of the pseudo-inverse does
    not enter.)  Every variance is multiplied by ``inefficiency``.

    A slot is RESOLVED, and in ``live`` (ascending slot indices; everything else here is indexed by position in ``live``), when
    ``H[K][s]``, the sum of its squared weights, is a normal float64 (at least 2.2e-308).  Below that the device's sum has lost
    its digits or is 0 -- the weights themselves are below 1.5e-154, which a cold target reaches in a slot that only the hot
    rungs populate -- and ``H[K][s] / p_s^2`` would be 0 / 0.  Rescaling cannot help, the sum is gone before the host sees it;
    the slot is left out (``unresolved`` when it has a mass all the same) and the others keep their results.  For a resolved
    slot ``p_s^2 >= H[K][s]`` (the weights are >= 0), so no division here can underflow.

    ``var`` is ``Var ln p_c`` of the live slots, O(S K^2) work like everything but :meth:`covariance`."""

    def __init__(self, h, p, response, inefficiency):
        k = response.shape[0]
        resolved = h[k] >= np.finfo(np.float64).tiny
        self.unresolved = (p > 0) & ~resolved
        self.live = np.flatnonzero(resolved)
        self.response, self.inefficiency = response, inefficiency
        self.p = p[self.live]
        self.u = h[:k, self.live] / self.p[None, :] - h[:k].sum(axis=1)[:, None]
        self.own_sums = h[k, self.live]
        self.to_state = self.own_sums / self.p
        self.own_term = self.own_sums / self.p ** 2
        self.state = h[k].sum()
        self.mu = response @ self.u
        self.var = (self.own_term - 2.0 * self.to_state + self.state + np.einsum("kc,kc->c", self.u, self.mu)) * inefficiency

    def covariance(self, sel):
        """``Cov(ln p_c, ln p_c')`` over the live slots that the mask ``sel`` picks: the only matrix over slots."""
        n = int(np.count_nonzero(sel))
        cov = self.u[:, sel].T @ self.mu[:, sel] - self.to_state[sel][:, None] - self.to_state[sel][None, :] + self.state
        cov[np.arange(n), np.arange(n)] += self.own_term[sel]
        return cov * self.inefficiency

    def var_from(self, sel, at):
        """``Var(ln p_c - ln p_at)`` of the live slots that ``sel`` picks against live slot ``at`` (the common terms cancel)."""
        du = self.u[:, sel] - self.u[:, at][:, None]
        return (self.own_term[sel] + self.own_term[at] + np.einsum("kc,kc->c", du, self.response @ du)) * self.inefficiency

    def var_of_sum(self, sel):
        """``Var sum_c p_c = sum_cc' p_c p_c' C_cc'`` over the live slots that ``sel`` picks."""
        po = self.p[sel]
        v = self.u[:, sel] @ po
        own_sum, total = self.own_sums[sel].sum(), po.sum()
        return (own_sum - 2.0 * total * own_sum + total * total * self.state + v @ (self.response @ v)) * self.inefficiency


def _slot_uncertainties(temps, mass, density, slot_gram, inner, ladder_gram, column_counts, inefficiency, covariance):
    """The error bars that a profile and a surface share, one :class:`_SlotLogCovariance` per temperature.  ``mass`` ``(T, S)``
    and ``slot_gram`` ``(T, K + 1, S)`` over all slots; ``inner`` ``(S,)``: which of them are the ``I`` bins (cells) proper, in
    whose order ``density`` ``(T, I)`` is.  Returns ``d_slots`` ``(T, S)``: ``p sqrt(Var ln p)``, 0 for an empty slot and NaN for an
    unresolved one; ``d_free`` ``(T, I)``: ``T sqrt(Var ln p)``, NaN for a slot that is not live; ``lowest`` ``(T,)``: the inner slot
    of largest density; ``d_lowest`` ``(T, I)``: ``T sqrt(Var(ln p - ln p_lowest))``, 0 at ``lowest`` and all NaN when ``lowest`` itself
    is not live; ``d_outside`` ``(T,)``: the standard error of the summed masses of the live slots outside ``inner``; ``log_cov``
    ``(T, I, I)``, NaN in the rows and columns of slots that are not live (``None`` without ``covariance``)."""
    nt, n_slots, n_inner = temps.size, inner.size, int(inner.sum())
    to_inner = np.full(n_slots, -1, dtype=np.intp)       # position among the inner slots (-1 outside)
    to_inner[inner] = np.arange(n_inner)
    d_slots, d_outside = np.zeros((nt, n_slots)), np.zeros(nt)
    d_free, d_lowest = np.full((nt, n_inner), np.nan), np.full((nt, n_inner), np.nan)
    lowest = np.zeros(nt, dtype=np.int64)
    log_cov = np.full((nt, n_inner, n_inner), np.nan) if covariance else None
    response = _ladder_response(ladder_gram, column_counts)
    for t in range(nt):
        c = _SlotLogCovariance(slot_gram[t], mass[t], response, inefficiency)
        d_slots[t, c.unresolved] = np.nan                # (a mass, but no error bar; an empty slot keeps 0)
        root = np.sqrt(np.clip(c.var, 0.0, None))
        d_slots[t, c.live] = c.p * root
        out_live = ~inner[c.live]
        if out_live.any():
            d_outside[t] = np.sqrt(max(c.var_of_sum(out_live), 0.0))
        bins = inner[c.live]
        own = to_inner[c.live[bins]]
        if own.size == 0:
            continue
        d_free[t, own] = temps[t] * root[bins]
        lowest[t] = int(np.argmax(density[t]))
        at = np.flatnonzero(own == lowest[t])
        if at.size:
            at = int(np.flatnonzero(bins)[at[0]])
            d_lowest[t, own] = temps[t] * np.sqrt(np.clip(c.var_from(bins, at), 0.0, None))
            d_lowest[t, lowest[t]] = 0.0
        if covariance:
            if own.size == n_inner:                      # (every inner slot live: own is 0 .. I - 1 in order)
                log_cov[t] = c.covariance(bins)
            else:
                log_cov[t][np.ix_(own, own)] = c.covariance(bins)
    return d_slots, d_free, lowest, d_lowest, d_outside, log_cov


def _profile_uncertainty_result(temps, edges, mass, counts, neff, slot_gram, ladder_gram, column_counts, n_used, inefficiency):
    """The dictionary of :func:`mbar_free_energy_profile_uncertainties` from what ``me_mbar_histogram_gram`` returns:
    :func:`_slot_uncertainties` over the ``B + 3`` slots, of which the ``B`` bins are the inner ones."""
    out = _profile_result(temps, edges, mass, counts, neff)
    b = edges.size - 1
    inner = np.arange(b + 3) < b
    d_slot, d_free, lowest, d_lowest, _, log_cov = _slot_uncertainties(temps, mass, out["density"], slot_gram, inner, ladder_gram,
                                                                       column_counts, inefficiency, True)
    out.update({"d_mass": d_slot[:, :b].copy(), "d_below": d_slot[:, b].copy(), "d_above": d_slot[:, b + 1].copy(),
                "d_not_a_number": d_slot[:, b + 2].copy(), "d_free_energy": d_free, "log_mass_cov": log_cov,
                "d_free_energy_from_lowest": d_lowest, "lowest": lowest, "n_samples": int(n_used)})
    return out


def _free_energy_profile_uncertainties(fn, lead, n_rungs, f, targets, middle, edges, inefficiency):
    """``middle``: as in :func:`_free_energy_profile`."""
    b, k = edges.size - 1, n_rungs
    mass, counts, neff = np.zeros((targets.size, b + 3)), np.zeros(b + 3, dtype=np.int64), np.zeros(targets.size)
    slot_gram, ladder_gram, column_counts = np.zeros((targets.size, k + 1, b + 3)), np.zeros((k, k)), np.zeros(k)
    n_used = ctypes.c_int64()
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, *middle, _capi.double_ptr(edges), b,
          _capi.double_ptr(slot_gram), _capi.double_ptr(ladder_gram), _capi.double_ptr(column_counts), _capi.double_ptr(mass),
          _capi.int64_ptr(counts), _capi.double_ptr(neff), ctypes.byref(n_used))
    return _profile_uncertainty_result(targets, edges, mass, counts, neff, slot_gram, ladder_gram, column_counts, n_used.value,
                                       inefficiency)


def validate_profile_inefficiency(inefficiency):
    """:func:`validate_mbar_inefficiency` for the profile's error bars, where the inefficiency is one scalar: anything with a
    shape is a ``ValueError`` too."""
    if np.ndim(inefficiency) != 0:
        raise ValueError("inefficiency must be a scalar")
    return validate_mbar_inefficiency(inefficiency)


def mbar_free_energy_profile_uncertainties(energies, rungs, temps, f, targets, values, edges, inefficiency=1.0, device=0):
    """:func:`mbar_free_energy_profile` with the asymptotic standard errors of its masses and of the free-energy profile
    (``me_mbar_histogram_gram_samples``; the engine form is ``MetropolisEngine.free_energy_profile_uncertainties``).  The bin
    indicators are columns of the MBAR weight matrix like any observable (Shirts & Chodera 2008, eqs. 8, D8), but DISJOINT ones:
    the Gram matrix of [ladder | state | one column per slot] follows from ``K + 1`` weighted histograms per temperature
    (csrc/me_mbar_hist_cov.hip), so any number of bins up to 256 costs no ``N x (K + 1 + B)`` matrix; and because those columns
    have no samples of their own the algebra reduces to ONE ``K x K`` pseudo-inverse per call and O(B K^2) products per
    temperature, in float64 here, the route :func:`mbar_free_energy_surface_uncertainties` takes for its cells.

    Returns every key of :func:`mbar_free_energy_profile`, bit for bit, and ``d_mass`` ``(T, B)``, ``d_below``, ``d_above``,
    ``d_not_a_number`` ``(T,)``: the standard errors ``p sqrt(Var ln p)`` of the masses; ``d_free_energy`` ``(T, B)``: ``T
    sqrt(Var ln p_b)``, the standard error of ``free_energy``; ``log_mass_cov`` ``(T, B, B)``: ``Cov(ln p_b, ln p_b')``, from
    which the error of any difference ``F_b - F_b'`` follows as ``T sqrt(C_bb + C_b'b' - 2 C_bb')``; ``lowest`` ``(T,)``: the
    bin of largest density; ``d_free_energy_from_lowest`` ``(T, B)``: the standard error of ``F_b - F_lowest`` (0 at
    ``lowest``); ``n_samples``: the samples with a finite energy.

    A slot whose mass is exactly 0 drops out of the algebra: its ``d_mass`` is 0, its ``d_free_energy``,
    ``d_free_energy_from_lowest`` and its row and column of ``log_mass_cov`` are NaN.  The rule goes by the MASS, not by
    ``counts``: at a cold target the weights of a bin that only hot rungs populate can all underflow.  The same holds, with
    ``d_mass`` NaN as well, for a slot whose mass is positive but below about 1.5e-154: the sum of its squared weights is no
    normal float64 any more and no error bar can be formed, although ``free_energy`` is still finite there.  Every other slot and
    temperature keeps its results, except that ``d_free_energy_from_lowest`` is NaN throughout a temperature whose ``lowest``
    bin is itself such a slot: there is nothing to take the differences from.

    The formula assumes INDEPENDENT samples: pass the statistical inefficiency of the series as ``inefficiency`` (a finite
    scalar ``>= 1``, ``ValueError`` otherwise) and every variance is multiplied by it."""
    g = validate_profile_inefficiency(inefficiency)
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    edges = validate_histogram_edges(edges)
    a = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel())
    if a.size != e.size:
        raise ValueError("values needs one entry per sample (%d), got %d" % (e.size, a.size))
    return _free_energy_profile_uncertainties(_capi.load().me_mbar_histogram_gram_samples, _host_samples(device, e, r, t), t.size, f,
                                              targets, (_capi.double_ptr(a),), edges, g)


def validate_surface_covariance(covariance):
    """The ``covariance`` switch of the surface's error bars: ``True`` or ``False`` (``bool`` or ``np.bool_``; ``ValueError``
    for anything else, so that a misplaced positional argument is not read as a truth value)."""
    if not isinstance(covariance, (bool, np.bool_)):
        raise ValueError("covariance must be True or False, not %r" % (covariance,))
    return bool(covariance)


def _surface_uncertainty_result(temps, edges_x, edges_y, mass, counts, neff, cell_gram, ladder_gram, column_counts, n_used,
                                inefficiency, covariance):
    """The dictionary of :func:`mbar_free_energy_surface_uncertainties` from what ``me_mbar_histogram_joint_gram`` returns
    (``mass`` ``(T, Bx + 3, By + 3)``, ``cell_gram`` ``(T, K + 1, S)``): :func:`_slot_uncertainties` over the ``S`` cells in
    their flat order ``slot_x (By + 3) + slot_y``, of which the ``Bx By`` cells of the inner grid are the inner ones.  The ``L x L``
    matrix over the live inner cells (9.5 MB per temperature at 33 x 33 bins) is formed with ``covariance`` alone."""
    out = _surface_result(temps, edges_x, edges_y, mass, counts, neff)
    nt, bx, by = temps.size, edges_x.size - 1, edges_y.size - 1
    inner = np.zeros((bx + 3, by + 3), dtype=bool)
    inner[:bx, :by] = True
    d_cell, d_free, low, d_lowest, d_outside, log_cov = _slot_uncertainties(
        temps, mass.reshape(nt, -1), out["density"].reshape(nt, -1), cell_gram, inner.ravel(), ladder_gram, column_counts,
        inefficiency, covariance)
    d_slots = d_cell.reshape(nt, bx + 3, by + 3)
    out.update({"d_mass": d_slots[:, :bx, :by].copy(), "d_mass_slots": d_slots, "d_outside": d_outside,
                "d_free_energy": d_free.reshape(nt, bx, by), "lowest": np.stack(np.unravel_index(low, (bx, by)), axis=1),
                "d_free_energy_from_lowest": d_lowest.reshape(nt, bx, by), "n_samples": int(n_used)})
    if covariance:
        out["log_mass_cov"] = log_cov
    return out


def _free_energy_surface_uncertainties(fn, lead, n_rungs, f, targets, middle_x, edges_x, middle_y, edges_y, inefficiency,
                                       covariance):
    """``middle_x`` / ``middle_y``: as in :func:`_free_energy_surface`."""
    bx, by, k = edges_x.size - 1, edges_y.size - 1, n_rungs
    mass, counts = np.zeros((targets.size, bx + 3, by + 3)), np.zeros((bx + 3, by + 3), dtype=np.int64)
    neff = np.zeros(targets.size)
    cell_gram = np.zeros((targets.size, k + 1, (bx + 3) * (by + 3)))
    ladder_gram, column_counts = np.zeros((k, k)), np.zeros(k)
    n_used = ctypes.c_int64()
    _call(fn, lead, _capi.double_ptr(f), _capi.double_ptr(targets), targets.size, *middle_x, _capi.double_ptr(edges_x), bx,
          *middle_y, _capi.double_ptr(edges_y), by, _capi.double_ptr(cell_gram), _capi.double_ptr(ladder_gram),
          _capi.double_ptr(column_counts), _capi.double_ptr(mass), _capi.int64_ptr(counts), _capi.double_ptr(neff),
          ctypes.byref(n_used))
    return _surface_uncertainty_result(targets, edges_x, edges_y, mass, counts, neff, cell_gram, ladder_gram, column_counts,
                                       n_used.value, inefficiency, covariance)


def mbar_free_energy_surface_uncertainties(energies, rungs, temps, f, targets, values_x, edges_x, values_y, edges_y,
                                           inefficiency=1.0, covariance=True, device=0):
    """:func:`mbar_free_energy_surface` with the asymptotic standard errors of its masses and of the free-energy surface
    (``me_mbar_histogram_joint_gram_samples``; the engine form is ``MetropolisEngine.free_energy_surface_uncertainties``).  The
    cell indicators are disjoint columns of the MBAR weight matrix, as the bins of
    :func:`mbar_free_energy_profile_uncertainties` are: ``K + 1`` weighted joint histograms per temperature
    (csrc/me_mbar_hist2d_cov.hip) hold everything their Gram matrix needs, and because those columns have no samples of their own
    the algebra reduces to ONE ``K x K`` pseudo-inverse and O(S K^2) products per temperature, in float64 here; no matrix over
    the up to 1296 cells is inverted.

    Returns every key of :func:`mbar_free_energy_surface`, bit for bit, and ``d_mass`` ``(T, Bx, By)``: the standard errors ``p
    sqrt(Var ln p)`` of the inner grid's masses; ``d_mass_slots`` ``(T, Bx + 3, By + 3)``: the same over all cells; ``d_outside``
    ``(T,)``: the error of ``outside``, from ``Var sum p_c = sum p_c p_c' C_cc'`` over the cells outside the inner grid;
    ``d_free_energy`` ``(T, Bx, By)``: ``T sqrt(Var ln p)``, the standard error of ``free_energy``; ``lowest`` ``(T, 2)``: the cell
    of largest density; ``d_free_energy_from_lowest`` ``(T, Bx, By)``: the standard error of ``F - F_lowest`` (0 at ``lowest``);
    ``n_samples``: the samples with a finite energy; and, with ``covariance=True``, ``log_mass_cov`` ``(T, Bx By, Bx By)``:
    ``Cov(ln p_c, ln p_c')`` with the cell index ``bx * By + by``, from which the error of any difference ``F_c - F_c'`` -- a
    saddle height -- follows as ``T sqrt(C_cc + C_c'c' - 2 C_cc')``.  At 33 x 33 bins that matrix is 9.5 MB per temperature:
    ``covariance=False`` leaves it out and forms no matrix over the cells at all; every other key is the same, bit for bit.

    A cell whose mass is exactly 0 drops out of the algebra: its ``d_mass`` is 0, its ``d_free_energy``,
    ``d_free_energy_from_lowest`` and its row and column of ``log_mass_cov`` are NaN.  The rule goes by the MASS, not by
    ``counts``: at a cold target the weights of a cell that only hot rungs populate can all underflow.  The same holds, with
    ``d_mass`` NaN as well, for a cell whose mass is positive but below about 1.5e-154: the sum of its squared weights is no
    normal float64 any more and no error bar can be formed, although ``free_energy`` is still finite there.  Every other cell and
    temperature keeps its results (``d_outside`` sums the cells that have an error bar).

    The formula assumes INDEPENDENT samples: pass the statistical inefficiency of the series as ``inefficiency`` (a finite
    scalar ``>= 1``, ``ValueError`` otherwise) and every variance is multiplied by it.  ``ValueError`` also for a ``covariance``
    that is not ``True`` or ``False``."""
    g = validate_profile_inefficiency(inefficiency)
    covariance = validate_surface_covariance(covariance)
    e, r, t = validate_mbar_samples(energies, rungs, temps)
    targets = validate_mbar_temps(targets, "targets")
    f = validate_mbar_f(f, t.size)
    edges_x, edges_y = validate_histogram2d_edges(edges_x, edges_y)
    a = np.ascontiguousarray(np.asarray(values_x, dtype=np.float64).ravel())
    b = np.ascontiguousarray(np.asarray(values_y, dtype=np.float64).ravel())
    if a.size != e.size or b.size != e.size:
        raise ValueError("values_x and values_y need one entry per sample (%d), got %d and %d" % (e.size, a.size, b.size))
    return _free_energy_surface_uncertainties(_capi.load().me_mbar_histogram_joint_gram_samples, _host_samples(device, e, r, t),
                                              t.size, f, targets, (_capi.double_ptr(a), _capi.double_ptr(b)), edges_x, (), edges_y,
                                              g, covariance)


def get_equilibration_points(df, device=None):
    """Per column ``[t0, g, Neff_max]``; constant columns are skipped and complex columns split into ``_real`` /
    ``_imag`` (statistics.py:25-48).  With ``device`` set, all columns go to the GPU in one batch."""
    names, rows = [], []
    for name in df.columns.values:
        column = df.loc[:, name]
        if column.nunique() <= 1:
            continue
        values = column.to_numpy()
        if np.iscomplexobj(values):
            names += [name + "_real", name + "_imag"]
            rows += [values.real, values.imag]
        else:
            names.append(name)
            rows.append(values.astype(np.float64))
    if device is not None and rows:
        t0, g, neff = detect_equilibration_batch(np.stack(rows), device=device)
        return {name: [int(t0[i]), float(g[i]), float(neff[i])] for i, name in enumerate(names)}
    return {name: list(detect_equilibration(row)) for name, row in zip(names, rows)}


def timeseries_from_csv(file_name, column_name=None):
    """Read a time-series file the reference writes (``df.to_csv``; layout of exampledata.csv: an index column, then
    observables, ``<term>_energy``, parameters and widths, complex values as ``(re+imj)`` strings) into
    ``{name: float array}``.  Like ``plottable_timeseries_from_csv`` (statistics.py:6-23) a non-float column becomes
    ``<name>_real`` plus, when its first entry has a non-zero imaginary part, ``<name>_imag``."""
    import pandas
    data = pandas.read_csv(file_name, index_col=0)
    names = data.columns if column_name is None else [column_name]
    out = {}
    for name in names:
        column = data[name]
        if column.dtype.kind == "f":
            out[name] = column.to_numpy(dtype=np.float64)
            continue
        values = np.array([complex(str(v).replace(" ", "")) for v in column], dtype=np.complex128)
        if values[0].imag != 0:
            out[name + "_imag"] = values.imag.copy()
        out[name + "_real"] = values.real.copy()
    return out


def get_equilibrated_means(df, cutoff=None):
    """Column means from row ``cutoff`` on (statistics.py:53-64; the reference's ``cutoff=None`` branch calls an
    undefined name, here it takes the largest ``t0``).  Returns ``(means, errors)``; like the reference, ``errors``
    stays empty."""
    if cutoff is None:
        points = get_equilibration_points(df)
        cutoff = max(t for t, _, _ in points.values()) if points else 0
    means = {name: np.average(df.loc[cutoff:, name]) for name in df.columns.values}
    return means, {}
