"""The yardstick of the error bars of reweighted observables, checked without a GPU: three facts about the observable-weighted
columns of tests/mbar_observable_uncertainty_reference.py (the single-rung limit, shift invariance, calibration), the
package's host algebra on a reference Gram matrix, the argument checks and the two new exports."""
import os
import re

import numpy as np
import pytest

from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_observable_uncertainty_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_SHIFT_MOVE = 1.7e-11       # d_mean under a further shift of 100, SVD route on both sides, as measured


def test_single_rung_limit_is_the_plain_standard_error():
    """K = 1, target T = T_0, 4096 samples: every weight is 1 / N and d_mean = sqrt(var(A) / N)."""
    energies, rungs, cols = ref.iso_quadratic_subsets(seed=29, temps=[1.0], n_subsets=1, per_rung=4096)[0]
    cols = cols[:2]                                              # x_0 and |x_0|
    w, counts, _, mean, shifts = ref.weight_matrix_observables(energies, rungs, [1.0], [0.0], [1.0], cols)
    d_mean, _ = ref.sigmas(ref.theta_svd(w, counts), 1, 1, 2, mean, shifts)
    want = np.sqrt(np.var(cols, axis=1) / energies.size)
    rel = np.abs(d_mean[0] - want) / want
    print("K = 1: d_mean %s, sqrt(var / N) %s, relative difference %s" % (d_mean[0], want, rel))
    assert np.all(rel <= 1e-12)


def test_a_further_shift_does_not_move_the_error_bar():
    """S_q lowered by a further 100 (every factor stays >= 1): d_mean moves by at most ten times the 1.7e-11 measured."""
    energies, rungs, cols = ref.calibration_subsets()[0]
    f = ref.solve(energies, rungs, ref.LADDER8)
    nt, q = ref.PHYSICS_TARGETS.size, cols.shape[0]
    w, counts, _, mean, shifts = ref.weight_matrix_observables(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols)
    a, _ = ref.sigmas(ref.theta_svd(w, counts), 8, nt, q, mean, shifts)
    w2, counts2, _, mean2, shifts2 = ref.weight_matrix_observables(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols,
                                                                   shifts=np.asarray(shifts, dtype=np.float64) - 100.0)
    b, _ = ref.sigmas(ref.theta_svd(w2, counts2), 8, nt, q, mean2, shifts2)
    rel = np.abs(a - b) / a
    print("further shift of 100: largest relative move of d_mean %.3e" % rel.max())
    assert float(w.min()) >= 0.0 and float(w2.min()) >= 0.0 and rel.max() <= 10 * MEASURED_SHIFT_MOVE


def test_standard_errors_are_calibrated_and_the_host_algebra_agrees():
    """64 subsets of exact samples of E = |x|^2 on LADDER8: the RMS z-score of (mean - exact) / d_mean of x_0, |x_0|, x_0^2 at
    three temperatures lies in the project's band.  On subset 0 the package's dictionary from the reference's Gram matrix is
    compared with the SVD route by the rule of ``ref.covariances``; a poisoned column gives NaN in its own places only."""
    nt, q = ref.PHYSICS_TARGETS.size, 3
    means, d_means = [], []
    for n, (energies, rungs, cols) in enumerate(ref.calibration_subsets()):
        f = ref.solve(energies, rungs, ref.LADDER8)
        w, counts, ln_z, mean, shifts = ref.weight_matrix_observables(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols)
        g = ref.gram(w)
        d_mean, _ = ref.sigmas(ref.theta_gram(g, counts), 8, nt, q, mean, shifts)
        means.append(np.asarray(mean, dtype=np.float64)), d_means.append(d_mean)
        if n == 0:
            first = (w, counts, ln_z, mean, shifts, g, energies.size)
    rms = ref.calibration_rms_z(means, d_means)
    print("rms z of the means (targets x columns):\n%s" % rms)
    lo, hi = uref.CAL_RMS_Z
    assert rms.shape == (3, 3) and np.all((rms >= lo) & (rms <= hi))

    w, counts, ln_z, mean, shifts, g, n = first
    args = (np.asarray(g, dtype=np.float64), np.asarray(counts, dtype=np.float64), 8, ref.PHYSICS_TARGETS, ("a", "b", "c"),
            np.asarray(ln_z, dtype=np.float64), np.asarray(mean, dtype=np.float64), np.asarray(shifts, dtype=np.float64), n)
    got = statistics._observable_uncertainty_result(*args, np.ones(3))
    want, scale = ref.covariances(ref.theta_svd(w, counts), 8, nt, q, mean, shifts)
    bound = ref.route_bound(w, counts)
    err = np.abs(got["mean_cov"] - want) / scale
    diag = np.abs(got["d_mean"] ** 2 - np.diagonal(want, axis1=1, axis2=2)) / np.diagonal(scale, axis1=1, axis2=2)
    rel = np.abs(got["d_mean"] - np.sqrt(np.diagonal(want, axis1=1, axis2=2))) / got["d_mean"]
    print("subset 0: mean_cov against the SVD route %.2e, d_mean^2 %.2e (bound %.2e); d_mean itself, relative %.2e"
          % (err.max(), diag.max(), 4 * bound, rel.max()))
    assert err.max() <= 4 * bound and diag.max() <= 4 * bound
    assert got["names"] == ("a", "b", "c") and got["n_samples"] == n and got["d_ln_z"].shape == (3,)
    assert got["mean_cov"].shape == (3, 3, 3) and np.all(np.isfinite(got["d_mean"]))
    # per-column inefficiencies: d_mean by sqrt(g_q), mean_cov by sqrt(g_q g_r); 4 and 16 are exact
    four = statistics._observable_uncertainty_result(*args, np.array([4.0, 1.0, 16.0]))
    assert np.array_equal(four["d_mean"], got["d_mean"] * np.array([2.0, 1.0, 4.0])[None, :])
    assert np.array_equal(four["mean_cov"], got["mean_cov"] * np.outer([2.0, 1.0, 4.0], [2.0, 1.0, 4.0])[None])
    # a poisoned column: the rows and columns of G of |x_0| at the second target are NaN
    bad = args[0].copy()
    c = 8 + 1 * 4 + 1 + 1
    bad[c, :] = bad[:, c] = np.nan
    poisoned = statistics._observable_uncertainty_result(bad, *args[1:], np.ones(3))
    nan = np.isnan(poisoned["mean_cov"])
    expect = np.zeros((3, 3, 3), dtype=bool)
    expect[1, 1, :] = expect[1, :, 1] = True
    assert np.array_equal(nan, expect) and np.array_equal(np.isnan(poisoned["d_mean"]), np.diagonal(expect, axis1=1, axis2=2))
    others = np.abs(poisoned["mean_cov"] - got["mean_cov"])[~expect] / scale[~expect]
    print("poisoned column: the other entries move by %.2e of their scale (bound %.2e)" % (others.max(), 4 * bound))
    assert others.max() <= 4 * bound and np.all(np.isfinite(poisoned["d_ln_z"]))


@pytest.mark.parametrize("bad", [0.5, 0.0, -1.0, float("nan"), float("inf"), [1.0, 0.5], [1.0, 2.0, 3.0], [[1.0, 2.0]]])
def test_inefficiency_is_validated_per_entry(bad):
    with pytest.raises(ValueError):
        statistics.validate_mbar_observable_inefficiency(bad, 2)
    with pytest.raises(ValueError):        # refused before the library is touched
        statistics.mbar_observable_uncertainties([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], [1.5], np.ones((2, 2)), inefficiency=bad)


def test_inefficiency_scalar_and_per_column():
    assert np.array_equal(statistics.validate_mbar_observable_inefficiency(2.0, 3), [2.0, 2.0, 2.0])
    assert np.array_equal(statistics.validate_mbar_observable_inefficiency([1.0, 2.5], 2), [1.0, 2.5])


def test_observable_shape_and_targets_are_validated():
    e, r, t, f = [1.0, 2.0, 3.0], [0, 1, 0], [1.0, 2.0], [0.0, 0.1]
    for cols in (np.ones((17, 3)), np.ones((2, 4)), np.ones((0, 3)), 1.0):
        with pytest.raises(ValueError):
            statistics.mbar_observable_uncertainties(e, r, t, f, [1.5], cols)
    for targets in ([], [0.0], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            statistics.mbar_observable_uncertainties(e, r, t, f, targets, np.ones((2, 3)))
    with pytest.raises(ValueError):
        statistics.mbar_observable_uncertainties(e, r, t, [0.0], [1.5], np.ones((2, 3)))         # f per rung
    with pytest.raises(ValueError):
        statistics.mbar_observable_uncertainties(e, r, np.linspace(0.5, 3.0, 65), np.zeros(65), [1.5], np.ones((2, 3)))


def test_header_and_binding_list_the_new_exports():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^\s*int\s+(me_[a-z_]+)\s*\(", text, flags=re.M))
    for name in ("me_mbar_gram_observables", "me_mbar_gram_observables_samples"):
        assert name in declared and name in _capi.SYMBOLS, name
    assert "#define ME_ABI_VERSION 1" in text and _capi.ABI_VERSION == 1
