"""The yardstick of the error bars of reweighted variances and energy covariances, checked without a GPU: two facts about the
second-moment columns of tests/mbar_fluctuation_uncertainty_reference.py (the single-rung limit, calibration against exact
values), the package's host algebra on a reference Gram matrix, the argument checks and the two new exports."""
import os
import re

import numpy as np
import pytest

from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_fluctuation_uncertainty_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_single_rung_limit_is_the_plain_standard_error():
    """K = 1, target T = T_0, 4096 samples: every weight is 1 / N, and the delta method on the sample moments gives exactly the
    standard error of a mean of the linearised quantity: d_var = sqrt(var((A - <A>)^2) / N), d_cov = sqrt(var((A - <A>)(E -
    <E>)) / N), d_energy_var = sqrt(var((E - <E>)^2) / N)."""
    energies, rungs, cols = ref.iso_quadratic_subsets(seed=29, temps=[1.0], n_subsets=1, per_rung=4096)[0]
    w, counts, _, moments, _, _ = ref.weight_matrix_fluctuations(energies, rungs, [1.0], [0.0], [1.0], cols)
    got = ref.sigmas(ref.theta_svd(w, counts), 1, 1, 3, moments)
    n = energies.size
    de = energies - energies.mean()
    da = cols - cols.mean(axis=1, keepdims=True)
    want = {"d_energy_mean": np.sqrt(np.var(energies) / n), "d_energy_var": np.sqrt(np.var(de * de) / n),
            "d_mean": np.sqrt(np.var(cols, axis=1) / n), "d_var": np.sqrt(np.var(da * da, axis=1) / n),
            "d_cov_energy": np.sqrt(np.var(da * de[None, :], axis=1) / n)}
    for key in ref.KEYS:
        rel = np.abs(np.ravel(got[key]) - np.ravel(want[key])) / np.ravel(want[key])
        print("K = 1: %s %s, plain standard error %s, relative difference %s" % (key, np.ravel(got[key]), np.ravel(want[key]), rel))
        assert np.all(rel <= 1e-9), key


def _result(gram, counts, names, moments, n, inefficiency=1.0):
    """statistics._fluctuation_uncertainty_result on reference arrays; the values are derived from the moments."""
    t, q = ref.PHYSICS_TARGETS, len(names)
    m = np.asarray(moments, dtype=np.float64)
    var_e, var_a, cov = ref.values(m, q)
    return statistics._fluctuation_uncertainty_result(np.asarray(gram, dtype=np.float64), np.asarray(counts, dtype=np.float64), 8, t,
                                                      names, (m[:, 0], var_e), (m[:, 2::3], var_a, cov), m, n, inefficiency)


def test_standard_errors_are_calibrated_and_the_host_algebra_agrees():
    """64 subsets of exact samples of E = |x|^2 on LADDER8: the RMS z-score of (estimate - exact) / error of Var E, Var A_q and
    Cov(A_q, E) for x_0, |x_0|, x_0^2 at three temperatures, 21 quantities, lies in the project's band (the reference alone, its
    Gram route in float64).  On subset 0 the package's dictionary from the reference's Gram matrix is compared with the SVD route
    by the rule of ``ref.variances``; a poisoned observable gives NaN in its own places only."""
    nt, q = ref.PHYSICS_TARGETS.size, 3
    estimates, errors = [], []
    for n, (energies, rungs, cols) in enumerate(ref.calibration_subsets()):
        f = ref.solve(energies, rungs, ref.LADDER8)
        w, counts, _, moments, _, _ = ref.weight_matrix_fluctuations(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols)
        g = ref.gram(w)
        d = ref.sigmas(ref.theta_gram(g, counts), 8, nt, q, moments)
        estimates.append([np.asarray(v, dtype=np.float64) for v in ref.values(moments, q)])
        errors.append((d["d_energy_var"], d["d_var"], d["d_cov_energy"]))
        if n == 0:
            first = (w, counts, moments, g, energies.size)
    rms = ref.calibration_rms_z(estimates, errors)
    print("rms z (targets x [Var E, Var x_0, Var |x_0|, Var x_0^2, Cov(x_0, E), Cov(|x_0|, E), Cov(x_0^2, E)]):\n%s" % rms)
    lo, hi = uref.CAL_RMS_Z
    assert rms.shape == (3, 7) and np.all((rms >= lo) & (rms <= hi))

    w, counts, moments, g, n = first
    got = _result(g, counts, ("a", "b", "c"), moments, n)
    want, scale = ref.variances(ref.theta_svd(w, counts), 8, nt, q, moments)
    bound = ref.route_bound(w, counts)
    for key in ref.KEYS:
        err = np.abs(got[key] ** 2 - want[key]) / scale[key]
        rel = np.abs(got[key] - np.sqrt(want[key])) / got[key]
        print("subset 0: %s^2 against the SVD route %.2e of its scale (bound %.2e); %s itself, relative %.2e"
              % (key, err.max(), 4 * bound, key, rel.max()))
        assert got[key].shape == want[key].shape and np.all(np.isfinite(got[key])) and np.all(got[key] > 0)
        assert err.max() <= 4 * bound
    assert got["names"] == ("a", "b", "c") and got["n_samples"] == n
    t_sq = ref.PHYSICS_TARGETS ** 2
    assert np.array_equal(got["d_heat_capacity"], got["d_energy_var"] / t_sq)
    assert np.array_equal(got["heat_capacity"], got["energy_var"] / t_sq)
    assert np.array_equal(got["d_dmean_dT"], got["d_cov_energy"] / t_sq[:, None])
    assert np.array_equal(got["dmean_dT"], got["cov_energy"] / t_sq[:, None])
    # inefficiency 4 doubles every error exactly and moves no value
    four = _result(g, counts, ("a", "b", "c"), moments, n, 4.0)
    for key, v in got.items():
        if key.startswith("d_") and key != "dmean_dT":
            assert np.array_equal(four[key], 2.0 * v), key
        elif key not in ("names", "n_samples"):
            assert np.array_equal(four[key], v), key
    # a poisoned observable: the rows and columns of G of the three columns of |x_0| at the second target are NaN
    bad = np.asarray(g, dtype=np.float64).copy()
    c = 8 + 1 * 12 + 3 + 3 * 1
    bad[c:c + 3, :] = bad[:, c:c + 3] = np.nan
    poisoned = _result(bad, counts, ("a", "b", "c"), moments, n)
    expect = np.zeros((3, 3), dtype=bool)
    expect[1, 1] = True
    for key in ("d_mean", "d_var", "d_cov_energy", "d_dmean_dT"):
        assert np.array_equal(np.isnan(poisoned[key]), expect), key
    for key in ref.KEYS:
        keep = ~expect if poisoned[key].ndim == 2 else np.ones(3, dtype=bool)
        moved = np.abs(poisoned[key] ** 2 - got[key] ** 2)[keep] / scale[key][keep]
        print("poisoned column: %s^2 elsewhere moves by %.2e of its scale (bound %.2e)" % (key, moved.max(), 4 * bound))
        assert moved.max() <= 4 * bound


def test_without_observables_the_energy_keys_stand_alone():
    """Q = 0: C = K + 3 T; the energy errors agree with those among three observables (the extra columns have count 0 and do not
    enter Theta's other entries) within the route bound, and the observable keys are (T, 0)."""
    energies, rungs, cols = ref.calibration_subsets()[0]
    f = ref.solve(energies, rungs, ref.LADDER8)
    w0, counts0, _, m0, _, _ = ref.weight_matrix_fluctuations(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS)
    w3, counts3, _, m3, _, _ = ref.weight_matrix_fluctuations(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols)
    assert w0.shape[1] == 8 + 3 * 3 and w3.shape[1] == 8 + 3 * 12
    alone = _result(ref.gram(w0), counts0, (), m0, energies.size)
    among = _result(ref.gram(w3), counts3, (0, 1, 2), m3, energies.size)
    _, scale = ref.variances(ref.theta_svd(w3, counts3), 8, 3, 3, m3)
    bound = ref.route_bound(w3, counts3)
    for key in ("d_energy_mean", "d_energy_var"):
        err = np.abs(alone[key] ** 2 - among[key] ** 2) / scale[key]
        print("Q = 0 against Q = 3: %s^2 differs by %.2e of its scale (bound %.2e)" % (key, err.max(), 4 * bound))
        assert err.max() <= 4 * bound
    for key in ("mean", "d_mean", "var", "d_var", "cov_energy", "d_cov_energy", "dmean_dT", "d_dmean_dT"):
        assert alone[key].shape == (3, 0), key
    assert alone["names"] == ()


@pytest.mark.parametrize("bad", [0.5, 0.0, -1.0, float("nan"), float("inf"), [1.0, 1.0], "recorded"])
def test_inefficiency_is_a_finite_scalar_of_at_least_one(bad):
    with pytest.raises(ValueError):        # refused before the library is touched
        statistics.mbar_fluctuation_uncertainties([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], [1.5], np.ones((2, 2)), inefficiency=bad)


def test_observable_shape_and_targets_are_validated():
    e, r, t, f = [1.0, 2.0, 3.0], [0, 1, 0], [1.0, 2.0], [0.0, 0.1]
    for cols in (np.ones((17, 3)), np.ones((2, 4)), np.ones((0, 3)), 1.0):
        with pytest.raises(ValueError):
            statistics.mbar_fluctuation_uncertainties(e, r, t, f, [1.5], cols)
    for targets in ([], [0.0], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            statistics.mbar_fluctuation_uncertainties(e, r, t, f, targets, np.ones((2, 3)))
        with pytest.raises(ValueError):
            statistics.mbar_fluctuation_uncertainties(e, r, t, f, targets)
    with pytest.raises(ValueError):
        statistics.mbar_fluctuation_uncertainties(e, r, t, [0.0], [1.5])                          # f per rung
    with pytest.raises(ValueError):
        statistics.mbar_fluctuation_uncertainties(e, r, np.linspace(0.5, 3.0, 65), np.zeros(65), [1.5])
    assert statistics.validate_mbar_fluctuation_observables(None, 5).shape == (0, 5)


def test_header_and_binding_list_the_new_exports():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = dict(re.findall(r"^\s*int\s+(me_[a-z_0-9]+)\s*\(([^;]*)\);", text, flags=re.M | re.S))
    for name in ("me_mbar_gram_fluctuations", "me_mbar_gram_fluctuations_samples"):
        assert name in declared and name in _capi.SYMBOLS, name
        assert len(declared[name].split(",")) == len(_capi.SYMBOLS[name][1]), name
    assert "#define ME_ABI_VERSION 1" in text and _capi.ABI_VERSION == 1
