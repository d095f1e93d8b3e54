"""The long-double reference of the pooled statistical inefficiency (tests/series_reference.py) against the host estimator, the
figures it was measured to give, and the calibration that the feature exists for: MBAR error bars of correlated records with
and without the pooled g.  No GPU, no library."""
import numpy as np

from metropolisengine_amd import statistics
import mbar_uncertainty_reference as u
import series_reference as sref


def test_one_series_is_the_host_estimator():
    rng = np.random.default_rng(7)
    for phi, n in ((0.5, 50), (0.9, 200), (0.97, 333), (0.0, 3), (0.3, 4)):
        x = sref.ar1(rng, [phi], n, 1)[:, 0, :]
        for mintime in (0, 3, 10):
            want = statistics.statistical_inefficiency(x[:, 0], mintime=mintime)
            got = sref.pooled_inefficiency(x, mintime=mintime)
            assert abs(float(got["g"]) - want) <= 1e-12 * want, (phi, n, mintime, float(got["g"]), want)
            assert got["chains_used"] == 1 and abs(float(got["mean"]) - x.mean()) <= 1e-15 + 1e-12 * abs(x.mean())
            assert abs(float(got["var"]) - x.var()) <= 1e-12 * x.var()


def test_measured_stop_lags_and_g():
    r, k, m = sref.SHAPES[-1]
    assert (r, k, m) == (200, 5, 192)
    got = sref.grouped_inefficiency(sref.shape_series(r, k, m), m)
    print("stop lags", got["stop_lag"], "g", got["g"].astype(np.float64))
    assert list(got["stop_lag"]) == [12, 18, 39, 125, 199]
    assert np.allclose(got["g"].astype(np.float64), [3.10, 8.39, 17.4, 59.9, 100.4], rtol=5e-3)
    # the walks end in the first, second and fourth batch of 64 lags
    assert sorted({int(s) // 64 for s in got["stop_lag"]}) == [0, 1, 3]


def test_no_stop_decision_sits_near_rounding():
    """The condition that lets the GPU test demand exact stop lags: every C(t) the walks meet is far from 0."""
    least = min(float(sref.grouped_inefficiency(sref.shape_series(r, k, m), m)["least_c"].min()) for r, k, m in sref.SHAPES)
    print("least |C(t)| up to the stop lags over all shapes: %.3e" % least)
    assert least >= 1e-6


def test_unused_chains_and_degenerate_columns():
    x = sref.shape_series(34, 1, 64)
    y = x.copy()
    y[5, 7] = np.nan
    y[0, 9] = np.inf
    got = sref.pooled_inefficiency(y)
    want = sref.pooled_inefficiency(np.delete(x, [7, 9], axis=1))
    assert got["chains_used"] == 62 and got["g"] == want["g"] and got["stop_lag"] == want["stop_lag"]
    none = sref.pooled_inefficiency(np.full((5, 64), np.nan))
    assert none["chains_used"] == 0 and np.isnan(none["g"]) and np.all(np.isnan(none["acf"]))
    flat = sref.pooled_inefficiency(np.full((5, 64), 2.5))
    assert flat["var"] == 0 and np.isnan(flat["g"]) and flat["stop_lag"] == 0
    clipped = sref.pooled_inefficiency(sref.shape_series(200, 5, 192)[:, 4 * 192:], max_lag=70)
    assert clipped["stop_lag"] == 71 and clipped["acf"].size == 71 and np.all(np.isfinite(clipped["acf"].astype(np.float64)))


def test_calibration_of_error_bars_on_correlated_records():
    """64 replicas of the AR(1) calibration ladder: the asymptotic error bars are too small by sqrt(g) with inefficiency = 1
    and honest (slightly conservative) with the largest pooled g over the rungs."""
    rungs = sref.calibration_rungs()
    k = u.CAL_TEMPS.size
    f_all, sig_1, sig_g, g_all = [], [], [], []
    for e in sref.calibration_energies():
        flat = e.ravel()
        f = u.solve(flat, rungs, u.CAL_TEMPS)
        w, counts, _, mean_e, shift = u.weight_matrix(flat, rungs, u.CAL_TEMPS, f)
        d_f = u.sigmas(u.theta_gram(u.gram(w), counts), k, 0, mean_e, shift)[0]
        g = sref.grouped_inefficiency(e, sref.CAL_CHAINS)["g"].astype(np.float64)
        f_all.append(f)
        sig_1.append(d_f)
        sig_g.append(d_f * np.sqrt(g.max()))
        g_all.append(g)
    z_1, z_g = sref.calibration_z(f_all, sig_1), sref.calibration_z(f_all, sig_g)
    g_mean = np.mean(g_all, axis=0)
    print("pooled RMS z of f[1:]: %.3f with inefficiency 1, %.3f with the largest pooled g; mean g per rung %s (exact %.2f)"
          % (z_1, z_g, np.round(g_mean, 2), sref.CAL_EXACT_G))
    assert z_1 > 1.5
    assert 0.7 <= z_g <= 1.2
    assert np.all(np.abs(g_mean - sref.CAL_EXACT_G) < 0.6)
