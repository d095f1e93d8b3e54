"""The yardstick of the asymptotic MBAR error bars, checked without a GPU: the two routes of tests/mbar_uncertainty_reference.py
agree, the package's host algebra (statistics.mbar_theta and the dictionary built from a Gram matrix) agrees with them, and
the standard errors are CALIBRATED -- on a problem whose free energies are known exactly the z-scores have unit variance."""
import numpy as np
import pytest

from metropolisengine_amd import statistics
import mbar_uncertainty_reference as ref

# How far two float64 routes to Theta may lie apart: ref.route_bound, 64 C 2^-53 / mu with mu the smallest eigenvalue of
# I - S V^T N V S above the cut of the pseudo-inverse (0.26 ... 0.27 here), 2e-13 ... 5e-13 for these cases.  Observed:
# 4e-15 ... 1.3e-14.  The comparison is relative to the largest entry of Theta, not entry by entry: the bound is one on the
# norm, and Theta has entries that are small by cancellation.  What is derived from Theta is compared entry by entry in
# test_result_dictionary_from_a_gram_matrix.


def _problem(k, n_targets, n=2048 + 5):
    temps, energies, rungs = ref.synthetic(k, n)
    f = ref.solve(energies, rungs, temps, tol=1e-13)
    targets = ref.targets_for(temps, n_targets)
    return temps, energies, rungs, f, targets


@pytest.mark.parametrize("k,n_targets", [(8, 0), (8, 3), (12, 2)])
def test_gram_and_svd_routes_agree(k, n_targets):
    temps, energies, rungs, f, targets = _problem(k, n_targets)
    w, counts, _, _, _ = ref.weight_matrix(energies, rungs, temps, f, targets)
    assert w.dtype == np.longdouble and float(w.min()) >= 0.0
    assert np.abs(w.sum(axis=0) - 1).max() < 1e-11                       # every column sums to 1 (f converged to 1e-13)
    assert np.abs(w @ counts - 1).max() < 1e-15                          # sum_j N_j W_nj = 1 for every sample
    g = ref.gram(w)
    a, b = ref.theta_gram(g, counts), ref.theta_svd(w, counts)
    rel = np.abs(a - b).max() / np.abs(b).max()
    bound = ref.route_bound(w, counts)
    mine = statistics.mbar_theta(np.asarray(g, dtype=np.float64), np.asarray(counts, dtype=np.float64))
    rel_mine = np.abs(mine - b).max() / np.abs(b).max()
    print("K = %d, %d targets: Gram route against SVD route %.2e, statistics.mbar_theta %.2e (bound %.2e)" % (k, n_targets, rel, rel_mine, bound))
    assert rel <= bound
    assert rel_mine <= bound


def test_result_dictionary_from_a_gram_matrix():
    temps, energies, rungs, f, targets = _problem(8, 3)
    w, counts, ln_z, mean_e, shift = ref.weight_matrix(energies, rungs, temps, f, targets)
    g64, c64 = np.asarray(ref.gram(w), dtype=np.float64), np.asarray(counts, dtype=np.float64)
    lz64, me64 = np.asarray(ln_z, dtype=np.float64), np.asarray(mean_e, dtype=np.float64)
    want = ref.sigmas(ref.theta_svd(w, counts), 8, 3, me64, shift)
    got = statistics._uncertainty_result(g64, c64, 8, targets, lz64, me64, energies.size, 1.0, float(shift))
    assert got["n_samples"] == energies.size and got["d_f"][0] == 0.0 and got["theta"].shape == (8, 8)
    # every variance (sigma^2) entry by entry: four entries of Theta each, so within 4 x the route bound x the largest entry
    theta_ref = ref.theta_svd(w, counts)
    bound = ref.route_bound(w, counts)
    var_ref, scale = ref.variances(theta_ref, 8, 3, me64, shift)
    for name, v, sc in zip(("d_f_matrix", "d_ln_z", "d_energy_mean"), var_ref, scale):
        err = np.abs(got[name] ** 2 - v) / sc
        if name == "d_f_matrix":
            err = err[~np.eye(8, dtype=bool)]
        print("%s: largest |sigma^2 - reference| / scale %.2e (bound %.2e), relative to sigma^2 itself %.2e"
              % (name, err.max(), 4.0 * bound, (np.abs(got[name] ** 2 - v)[v > 0] / v[v > 0]).max()))
        assert np.all(err <= 4.0 * bound), name
    assert np.array_equal(got["d_f"], got["d_f_matrix"][:, 0])
    for name, ref_value in zip(("d_f", "d_f_matrix", "d_ln_z", "d_energy_mean"), want):
        assert got[name].shape == np.shape(ref_value) and np.all(np.isfinite(got[name])), name
    four = statistics._uncertainty_result(g64, c64, 8, targets, lz64, me64, energies.size, 4.0, float(shift))
    for name in ("d_f", "d_f_matrix", "d_ln_z", "d_energy_mean"):
        assert np.array_equal(four[name], 2.0 * got[name]), name          # sqrt(4 v) = 2 sqrt(v) exactly
    assert np.array_equal(four["theta"], 4.0 * got["theta"])


@pytest.mark.parametrize("bad", [0.5, 0.0, -1.0, float("nan"), float("inf")])
def test_inefficiency_must_be_finite_and_at_least_one(bad):
    with pytest.raises(ValueError):
        statistics.validate_mbar_inefficiency(bad)
    with pytest.raises(ValueError):        # refused before the library is touched
        statistics.mbar_uncertainties([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], inefficiency=bad)


def test_standard_errors_are_calibrated():
    """64 independent replicas of a ladder over E ~ Gamma(2, T_k): f_k = -2 ln(T_k / T_0), <E>(T) = 2 T exactly.  The RMS
    z-score of each f_k, and of ln_z and of the mean energy over the two targets, lies in [0.75, 1.3]."""
    exact_f, exact_lnz, exact_mean = ref.calibration_exact()
    k, nt = ref.CAL_TEMPS.size, ref.CAL_TARGETS.size
    f_all, df_all, lz_all, dlz_all, mean_all, dmean_all = [], [], [], [], [], []
    for energies, rungs in ref.calibration_replicas():
        f = ref.solve(energies, rungs, ref.CAL_TEMPS, tol=1e-12)
        w, counts, ln_z, mean_e, shift = ref.weight_matrix(energies, rungs, ref.CAL_TEMPS, f, ref.CAL_TARGETS)
        d_f, _, d_lz, d_mean = ref.sigmas(ref.theta_gram(ref.gram(w), counts), k, nt, mean_e, shift)
        f_all.append(f[1:]), df_all.append(d_f[1:])
        lz_all.append(np.asarray(ln_z, dtype=np.float64)), dlz_all.append(d_lz)
        mean_all.append(np.asarray(mean_e, dtype=np.float64)), dmean_all.append(d_mean)
    lo, hi = ref.CAL_RMS_Z
    for name, rms in (("f", ref.rms_z(f_all, df_all, exact_f[1:])), ("ln_z", ref.rms_z(lz_all, dlz_all, exact_lnz, pooled=True)),
                      ("energy_mean", ref.rms_z(mean_all, dmean_all, exact_mean, pooled=True))):
        print("rms z of %s: %s" % (name, rms))
        assert np.all((rms >= lo) & (rms <= hi)), name
