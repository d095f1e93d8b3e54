"""Recorded observables and their MBAR reweighting without a GPU: the C ABI's new exports, the Python-side validation, the
numpy restatement (tests/mbar_observables_reference.py) against itself and against the exact moments of a quadratic energy
-- on the very inputs tests/test_gpu_mbar_observables.py gives the device."""
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref
import mbar_observables_reference as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["me_observable_samples_enable", "me_observable_samples_info", "me_observable_samples_get",
               "me_observable_samples_set", "me_mbar_reweight_observables", "me_mbar_reweight_observables_samples"]


def test_header_and_binding_list_the_new_exports():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^\s*int\s+(me_[a-z_]+)\s*\(", text, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    assert "#define ME_ABI_VERSION 1" in text and _capi.ABI_VERSION == 1
    assert "#define ME_MAX_RECORDED_OBSERVABLES 16" in text and statistics.MBAR_MAX_OBSERVABLES == 16


def test_build_compiles_the_observables_unit():
    from metropolisengine_amd import build
    with open(build.__file__) as fh:
        assert '"me_mbar_obs"' in fh.read()
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar_obs.hip"))


# ---------------------------------------------------------------------------------------------------- host logic


def _no_device_engine(nr=2, nc=1, terms=("total",)):
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)      # no device: validation comes first
    eng.num_real_params, eng.num_complex_params, eng.energy_term_names = nr, nc, list(terms)
    return eng


def test_catalogue_names_and_order():
    names = _no_device_engine(2, 1, ("quadratic", "quartic")).observable_names()
    assert names == ["real_0", "real_1", "re_0", "im_0", "abs_real_0", "abs_real_1", "abs_complex_0", "real_0_sq", "real_1_sq",
                     "energy_quadratic", "energy_quartic"]
    assert names == oref.catalogue_names(2, 1, ("quadratic", "quartic"))
    assert _no_device_engine(0, 2).observable_names() == ["re_0", "re_1", "im_0", "im_1", "abs_complex_0", "abs_complex_1",
                                                          "energy_total"]


def test_selections_are_validated_before_the_library():
    eng = _no_device_engine()
    names = eng.observable_names()
    idx = statistics.validate_observable_selection(["abs_real_1", 0, "abs_real_1", np.int64(9)], names)
    assert idx.dtype == np.int32 and idx.tolist() == [5, 0, 5, 9]
    assert statistics.validate_observable_selection("re_0", names).tolist() == [2]
    for bad in (["no_such"], [len(names)], [-1], [1.5], [True], ["real_0"] * 17, [None]):
        with pytest.raises(ValueError):
            eng.record_observables(bad)


@pytest.mark.parametrize("temps", [[], [0.0], [1.0, -2.0], [np.nan], [np.inf, 1.0], [[1.0, 2.0]]])
def test_bad_target_temperatures_are_refused_before_the_library(temps):
    with pytest.raises(ValueError):
        _no_device_engine().reweight_observables(temps)
    with pytest.raises(ValueError):
        statistics.mbar_reweight_observables([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], temps, [[0.5, 0.25]])


def test_bad_engine_less_arguments_are_refused_before_the_library():
    good = dict(energies=[1.0, 2.0, 3.0], rungs=[0, 1, 1], temps=[1.0, 2.0], f=[0.0, 0.1], targets=[1.5],
                observables=np.ones((2, 3)))
    for key, value in (("observables", np.ones((2, 4))),           # a column of another length
                       ("observables", np.ones((17, 3))),          # a 17th column
                       ("observables", np.ones((0, 3))),
                       ("observables", 1.0),
                       ("f", [0.0]), ("f", [0.0, np.nan]),
                       ("rungs", [0, 1, 2]), ("rungs", [0.0, 1.0, 1.0]), ("energies", [1.0, 2.0]), ("temps", [1.0, 0.0])):
        with pytest.raises(ValueError):
            statistics.mbar_reweight_observables(**dict(good, **{key: value}))
    a = statistics.validate_mbar_observables([1.0, np.nan, np.inf], 3)       # one column; values may be non-finite
    assert a.shape == (1, 3) and a.flags.c_contiguous
    assert statistics.validate_mbar_observables(np.ones((2, 3, 4)), 12).shape == (2, 12)


def test_result_dictionary():
    t = np.array([0.5, 2.0])
    cov = np.array([[1.0, 2.0], [4.0, 8.0]])
    out = statistics._observable_result(t, ["a", "b"], np.zeros((2, 2)), np.ones((2, 2)), cov, np.ones(2))
    assert out["names"] == ("a", "b") and np.array_equal(out["dmean_dT"], [[4.0, 8.0], [1.0, 2.0]])
    assert set(out) == {"temps", "names", "mean", "var", "cov_energy", "dmean_dT", "neff_fraction"}


# ---------------------------------------------------------------------------------------------------- the reference


def test_reference_restates_the_energy_reweighting_and_skips_unused_samples():
    energies, temps = ref.gamma_ladder(512, dim=16, seed=7)
    rungs = np.repeat(np.arange(temps.size), 512)
    e = energies.ravel().copy()
    rng = np.random.default_rng(3)
    cols = np.stack([e, rng.standard_normal(e.size), e * e])
    f, _, _, _ = ref.solve(e, rungs, temps)
    targets = [0.6, temps[3], 2.2]
    mean, var, cov, neff = oref.reweight_observables(e, rungs, temps, f, targets, cols)
    want = ref.reweight(e, rungs, temps, f, targets)
    assert np.allclose(mean[:, 0], want[1], rtol=1e-13) and np.allclose(var[:, 0], want[2], rtol=1e-12)
    assert np.allclose(cov[:, 0], var[:, 0], rtol=1e-13) and np.allclose(neff, want[3], rtol=1e-13)
    dirty, dirty_cols = e.copy(), cols.copy()
    dirty[[5, 700, 3000]] = [np.nan, np.inf, -np.inf]
    dirty_cols[1, 700] = np.nan                                  # of an unused sample: never seen
    keep = np.isfinite(dirty)
    a = oref.reweight_observables(dirty, rungs, temps, f, targets, dirty_cols)
    b = oref.reweight_observables(dirty[keep], rungs[keep], temps, f, targets, dirty_cols[:, keep])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    ld = oref.reweight_observables(e, rungs, temps, f, targets, cols, dtype=np.longdouble)
    for x, y in zip((mean, var, cov, neff), ld):
        assert np.allclose(x, y.astype(np.float64), rtol=1e-11)


def test_catalogue_values_of_the_reference():
    params = np.array([[0.5, -2.0, 3.0, -4.0], [-0.25, 1.0, 0.0, 0.0]])       # (2 real, 1 complex)
    ledger = np.array([[1.0, 2.0], [3.0, 4.0]])
    got = oref.catalogue_values(params, ledger, 2, 1)
    assert got.shape == (11, 2)
    assert got[:, 0].tolist() == [0.5, -2.0, 3.0, -4.0, 0.5, 2.0, 5.0, 0.25, 4.0, 1.0, 2.0]
    assert got[:, 1].tolist() == [-0.25, 1.0, 0.0, 0.0, 0.25, 1.0, 0.0, 0.0625, 1.0, 3.0, 4.0]


def test_reference_meets_the_statistical_condition_of_the_gpu_test():
    """The GPU test asks that the device's estimates from oref.iso_quadratic_subsets() -- 16 independent subsets of exact
    samples of E = |x|^2 in 4 dimensions on LADDER8 -- lie within 5 standard errors of the exact means of x_0, |x_0|, x_0^2
    and of d<x_0^2>/dT at three temperatures between rungs: twelve comparisons.  The reference meets all twelve on the same
    inputs (same generator, same seed)."""
    results = []
    for e, rungs, cols in oref.iso_quadratic_subsets():
        f, _, residual, _ = ref.solve(e, rungs, oref.LADDER8, tol=1e-10)
        assert residual <= 1e-10
        mean, _, cov, _ = oref.reweight_observables(e, rungs, oref.LADDER8, f, oref.PHYSICS_TARGETS, cols)
        results.append((mean, cov))
    n = 0
    for name, (est, exact) in oref.physics_estimates(results).items():
        ok, m, se = ref.within_5_se(est, exact)
        print(name, "mean", m, "exact", exact, "se", se, "deviation / se", np.abs(m - exact) / se)
        assert np.all(ok), name
        n += ok.size
    assert n == 12
