"""Long-double restatement of the pooled statistical inefficiency of csrc/me_series.hip (the multiple-series estimator of
Chodera et al., JCTC 3:26, 2007; include/metropolis_engine.h has the formulas), the AR(1) generator of its tests and the
calibration of the MBAR error bars on correlated records.  numpy only: no GPU, no library."""
import numpy as np

import mbar_uncertainty_reference as u

LD = np.longdouble
PHIS = (0.5, 0.8, 0.9, 0.97, 0.99)
SEED = 31
# (R, K, M) of the GPU tests: the minimum length; max_lag = 15 and 16, on either side of a lag tile; exactly two tiles and a
# remainder of the unrolled record loop; a block of four wavefronts that straddles rungs; walks that end in the first, second
# and fourth batch of 64 lags
SHAPES = ((3, 1, 64), (17, 2, 64), (18, 3, 192), (34, 2, 128), (200, 5, 192))


def ar1(rng, phis, n_records, n_chains):
    """``x[R][K][M]``: per rung k an AR(1) series of every chain with coefficient ``phis[k]`` and unit marginal variance."""
    phis = np.asarray(phis, dtype=np.float64)
    x = np.empty((n_records, phis.size, n_chains))
    x[0] = rng.standard_normal((phis.size, n_chains))
    for n in range(1, n_records):
        x[n] = phis[:, None] * x[n - 1] + np.sqrt(1.0 - phis[:, None] ** 2) * rng.standard_normal((phis.size, n_chains))
    return x


def shape_series(n_records, n_rungs, n_chains, seed=SEED):
    """The series of one entry of SHAPES as the device sees them, ``(R, K M)`` with rung ``c // M``."""
    return ar1(np.random.default_rng(seed), PHIS[:n_rungs], n_records, n_chains).reshape(n_records, n_rungs * n_chains)


def pooled_inefficiency(series, mintime=3, max_lag=None):
    """One column and one rung: ``series`` is ``(R, M)``.  ``{"g", "mean", "var", "stop_lag", "chains_used", "acf", "least_c"}``
    in long double (``acf`` has ``max_lag + 1`` entries, NaN beyond ``min(stop, max_lag)``); ``least_c`` is the least ``|C(t)|``
    met in the walk up to and including the stop lag."""
    a64 = np.asarray(series, dtype=np.float64)
    n_records = a64.shape[0]
    if max_lag is None:
        max_lag = n_records - 2
    assert n_records >= 3 and 1 <= max_lag <= n_records - 2 and mintime >= 0
    used = np.isfinite(a64).all(axis=0)
    m_u = int(used.sum())
    acf = np.full(max_lag + 1, np.nan, dtype=LD)
    out = {"g": LD(np.nan), "mean": LD(np.nan), "var": LD(np.nan), "stop_lag": 0, "chains_used": m_u, "acf": acf,
           "least_c": np.inf}
    if m_u == 0:
        return out
    a = a64[:, used].astype(LD)
    big_r = LD(n_records)
    out["mean"] = a.sum() / (LD(m_u) * big_r)
    d = a - out["mean"]
    p0 = (d * d).sum()
    out["var"] = p0 / (LD(m_u) * big_r)
    if p0 == 0:
        return out
    acf[0] = LD(1)
    g, stop, least = LD(1), max_lag + 1, np.inf
    for t in range(1, max_lag + 1):
        c = (d[:n_records - t] * d[t:]).sum() * big_r / (p0 * (big_r - LD(t)))
        acf[t] = c
        least = min(least, float(abs(c)))
        if c <= 0 and t > mintime:
            stop = t
            break
        g += LD(2) * c * (LD(1) - LD(t) / big_r)
    out.update(g=max(g, LD(1)), stop_lag=stop, least_c=least)
    return out


def grouped_inefficiency(series, group_chains, mintime=3, max_lag=None):
    """``series`` ``(R, n_series)`` in consecutive groups of ``group_chains``: the dictionary of :func:`pooled_inefficiency`
    with every entry stacked over the groups (``acf``: ``(groups, max_lag + 1)``)."""
    a = np.asarray(series, dtype=np.float64)
    parts = [pooled_inefficiency(a[:, k:k + group_chains], mintime, max_lag) for k in range(0, a.shape[1], group_chains)]
    return {key: np.array([p[key] for p in parts]) for key in parts[0]}


# ---- the calibration of the MBAR error bars on correlated records ------------------------------------------------------------
# The ladder of mbar_uncertainty_reference (CAL_TEMPS; E = (T / 2) sum of 4 squares, so E is Gamma(2, T) exactly), but the four
# components of a chain are AR(1) series with phi = 0.8 instead of independent draws: the marginals, and with them the exact
# free energies, stay what they were, while successive records are correlated with g = (1 + phi^2) / (1 - phi^2) = 4.56 (the
# autocorrelation of x^2 is phi^(2 t)).
CAL_PHI = 0.8
CAL_CHAINS, CAL_RECORDS, CAL_REPLICAS = 64, 32, 64
CAL_EXACT_G = (1.0 + CAL_PHI ** 2) / (1.0 - CAL_PHI ** 2)


def calibration_energies(seed=5):
    """The replicas' energy stores, each ``(CAL_RECORDS, K CAL_CHAINS)`` with rung ``c // CAL_CHAINS``."""
    rng = np.random.default_rng(seed)
    k = u.CAL_TEMPS.size
    out = []
    for _ in range(CAL_REPLICAS):
        x = ar1(rng, [CAL_PHI] * k, CAL_RECORDS, 4 * CAL_CHAINS).reshape(CAL_RECORDS, k, CAL_CHAINS, 4)
        e = 0.5 * u.CAL_TEMPS[None, :, None] * (x * x).sum(axis=3)
        out.append(e.reshape(CAL_RECORDS, k * CAL_CHAINS))
    return out


def calibration_rungs():
    return np.tile(np.repeat(np.arange(u.CAL_TEMPS.size), CAL_CHAINS), CAL_RECORDS).astype(np.int32)


def calibration_z(f, sigma):
    """Pooled root-mean-square z-score of ``f[:, 1:]`` (replicas x rungs) with the standard errors ``sigma`` of the same shape."""
    exact = u.calibration_exact()[0]
    return float(u.rms_z(np.asarray(f)[:, 1:], np.asarray(sigma)[:, 1:], exact[1:], pooled=True))
