"""MBAR over a temperature ladder without a GPU: the numpy restatement (tests/mbar_reference.py) against the exact free
energies, means and variances of a quadratic energy, the fixed-point identity of the reweighting, the Python-side
argument validation, and the C ABI's new exports."""
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 16
N_SUBSETS = 16
NEW_EXPORTS = ["me_energy_samples_enable", "me_energy_samples_record", "me_energy_samples_count", "me_energy_samples_get",
               "me_energy_samples_set", "me_mbar_solve", "me_mbar_reweight", "me_mbar_solve_samples",
               "me_mbar_reweight_samples"]


def _rungs(n_rungs, n_per_rung):
    return np.repeat(np.arange(n_rungs), n_per_rung)


@pytest.mark.parametrize("n_per_rung", [32768, 16384])
def test_reference_recovers_the_exact_quadratic_ladder(n_per_rung):
    """16 strided subsets are 16 independent estimates: their mean lies within 5 standard errors (15 degrees of freedom,
    about 2e-4 per quantity; the seed is fixed) of ln Z(T_k)/Z(T_0) = (D/2) ln(T_k/T_0) at every rung, and of
    <E> = D T / 2 and Var E = D T^2 / 2 at three temperatures between rungs."""
    energies, temps = ref.gamma_ladder(n_per_rung, dim=DIM)
    targets = np.array([0.6, 1.0, 2.2])
    assert not np.any(np.isclose(targets[:, None], temps[None, :]))
    ln_z, mean, var = [], [], []
    for s in range(N_SUBSETS):
        sub = energies[:, s::N_SUBSETS]
        rungs = _rungs(temps.size, sub.shape[1])
        f, its, residual, counts = ref.solve(sub, rungs, temps, tol=1e-10)
        assert residual <= 1e-10 and its < 1000 and np.all(counts == sub.shape[1])
        ln_z.append(-f)
        out = ref.reweight(sub, rungs, temps, f, targets)
        mean.append(out[1])
        var.append(out[2])
    exact_ln_z, _, _ = ref.exact_gamma(temps, temps[0], DIM)
    _, exact_mean, exact_var = ref.exact_gamma(targets, temps[0], DIM)
    for name, est, exact in (("ln_z", ln_z, exact_ln_z), ("energy_mean", mean, exact_mean), ("energy_var", var, exact_var)):
        ok, m, se = ref.within_5_se(est, exact)
        print(name, "mean", m, "se", se, "deviation / se", np.abs(m - exact) / np.where(se > 0, se, 1.0))
        assert np.all(ok), name


def test_reweighting_to_a_rung_returns_minus_f():
    """The fixed-point identity: ln Z(T_k)/Z(T_0) from the reweighting equals -f_k up to the stopping error."""
    tol = 1e-10
    energies, temps = ref.gamma_ladder(2048, dim=DIM, seed=3)
    rungs = _rungs(temps.size, 2048)
    f, _, residual, _ = ref.solve(energies, rungs, temps, tol=tol)
    assert residual <= tol
    ln_z = ref.reweight(energies, rungs, temps, f, temps)[0]
    print("max |ln_z + f|", np.max(np.abs(ln_z + f)))
    assert np.max(np.abs(ln_z + f)) <= 2 * tol


def test_long_double_and_float64_references_agree():
    energies, temps = ref.gamma_ladder(1024, dim=DIM, seed=5)
    rungs = _rungs(temps.size, 1024)
    f64, it64, _, _ = ref.solve(energies, rungs, temps, tol=1e-12)
    fld, itld, _, _ = ref.solve(energies, rungs, temps, tol=1e-12, dtype=np.longdouble)
    assert abs(it64 - itld) <= 1 and np.max(np.abs(f64 - fld.astype(np.float64))) <= 1e-11


def test_non_finite_energies_are_skipped_by_the_reference():
    energies, temps = ref.gamma_ladder(512, dim=DIM, seed=7)
    rungs = _rungs(temps.size, 512)
    dirty = energies.copy()
    dirty[1, :5] = np.inf
    dirty[4, 7] = np.nan
    ok, counts = ref.used(dirty, rungs, temps.size)
    assert counts.tolist() == [512, 507, 512, 512, 511, 512, 512, 512]
    f_dirty, _, _, _ = ref.solve(dirty, rungs, temps)
    f_clean, _, _, _ = ref.solve(dirty.ravel()[ok], rungs[ok], temps)
    assert np.array_equal(f_dirty, f_clean)
    dirty[2] = -np.inf
    with pytest.raises(ValueError):
        ref.solve(dirty, rungs, temps)


# ---------------------------------------------------------------------------------------------------- host logic


def _no_device_engine():
    return me.MetropolisEngine.__new__(me.MetropolisEngine)     # no device: validation comes first


@pytest.mark.parametrize("capacity", [-1, -1000])
def test_negative_capacity_is_refused_before_the_library(capacity):
    with pytest.raises(ValueError):
        _no_device_engine().record_energies(capacity)


@pytest.mark.parametrize("temps", [[], [0.0], [1.0, -2.0], [np.nan], [np.inf, 1.0], [[1.0, 2.0]]])
def test_bad_target_temperatures_are_refused_before_the_library(temps):
    with pytest.raises(ValueError):
        _no_device_engine().reweight(temps)
    with pytest.raises(ValueError):
        statistics.mbar_reweight([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], temps)


@pytest.mark.parametrize("tol", [0.0, -1e-10, np.nan, np.inf])
def test_bad_tolerances_are_refused_before_the_library(tol):
    with pytest.raises(ValueError):
        _no_device_engine().ladder_free_energies(tol=tol)
    with pytest.raises(ValueError):
        statistics.mbar_free_energies([1.0, 2.0], [0, 1], [1.0, 2.0], tol=tol)


def test_bad_iteration_limits_and_samples_are_refused_before_the_library():
    with pytest.raises(ValueError):
        _no_device_engine().ladder_free_energies(max_iter=0)
    good = ([1.0, 2.0, 3.0], [0, 1, 1], [1.0, 2.0])
    for energies, rungs, temps in (([1.0, 2.0], [0, 1, 1], good[2]),        # lengths differ
                                   (good[0], [0, 1, 2], good[2]),            # a rung beyond the ladder
                                   (good[0], [0, -1, 1], good[2]),
                                   (good[0], [0.0, 1.0, 1.0], good[2]),      # rungs are not integers
                                   ([], [], good[2]),
                                   (good[0], good[1], [1.0, 0.0]),
                                   (good[0], good[1], []),
                                   (good[0], [0, 1, 1], np.arange(1.0, 67.0))):   # more than 64 rungs
        with pytest.raises(ValueError):
            statistics.mbar_free_energies(energies, rungs, temps)
    with pytest.raises(ValueError):
        statistics.mbar_reweight(*good, f=[0.0], targets=[1.0])
    with pytest.raises(ValueError):
        statistics.mbar_reweight(*good, f=[0.0, np.nan], targets=[1.0])
    e, r, t = statistics.validate_mbar_samples(np.ones((2, 3)), np.zeros((2, 3), dtype=np.int64), [1.0])
    assert e.shape == (6,) and r.dtype == np.int32 and t.tolist() == [1.0]


def test_result_dictionaries():
    f = np.array([0.0, -1.5])
    out = statistics._solve_result(f, 12, 5e-11, np.array([3, 4]), 1e-10)
    assert out["converged"] and out["iterations"] == 12 and np.array_equal(out["ln_z"], -f)
    assert not statistics._solve_result(f, 12, 2e-10, np.array([3, 4]), 1e-10)["converged"]
    t = np.array([0.5, 2.0])
    rw = statistics._reweight_result(t, np.zeros(2), np.ones(2), np.array([1.0, 8.0]), np.ones(2))
    assert np.array_equal(rw["heat_capacity"], [4.0, 2.0])


def test_header_and_binding_list_the_new_exports():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^\s*int\s+(me_[a-z_]+)\s*\(", text, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    assert "#define ME_ABI_VERSION 1" in text and _capi.ABI_VERSION == 1


def test_build_compiles_the_mbar_unit():
    from metropolisengine_amd import build
    with open(build.__file__) as fh:
        assert '"me_mbar"' in fh.read()
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar.hip"))
