"""Reweighting to perturbed energies without a GPU: the C ABI's new exports, the Python-side validation, and the numpy
restatement (tests/mbar_perturbed_reference.py) against closed forms -- on the very inputs and with the very harness
tests/test_gpu_mbar_perturbed.py gives the device."""
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref
import mbar_observables_reference as oref
import mbar_perturbed_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_build_list_the_new_unit():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        declared = set(re.findall(r"^\s*int\s+(me_[a-z_]+)\s*\(", fh.read(), flags=re.M))
    for name in ("me_mbar_reweight_perturbed", "me_mbar_reweight_perturbed_samples"):
        assert name in declared and name in _capi.SYMBOLS, name
    from metropolisengine_amd import build
    assert "me_mbar_perturbed" in [name for name, _ in build.HOST_UNITS]
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar_perturbed.hip"))


# ------------------------------------------------------------------------------------------ 1. physics of the reference


def test_reference_meets_the_closed_forms_of_the_gpu_test():
    """oref.iso_quadratic_subsets() unchanged -- 16 subsets of 8 x 1024 exact samples of E = |x|^2 in 4 dimensions, columns
    x_0, |x_0|, x_0^2 -- reweighted to the eight (T, lambda) of pref.PHYSICS_TARGETS: ln_z(T, lambda) - ln_z(T, 0), <x_0>,
    <x_0^2> and Var x_0 against their closed forms, 32 values within 5 standard errors.  Measured: the float64 reference
    lies within 2.2 standard errors at all 32, and its neff_fraction is >= 0.55."""
    results, neff = [], []
    for e, rungs, cols in oref.iso_quadratic_subsets():
        f, _, residual, _ = ref.solve(e, rungs, oref.LADDER8, tol=1e-10)
        assert residual <= 1e-10
        out = pref.reweight_perturbed(e, rungs, oref.LADDER8, f, pref.PHYSICS_TEMPS, pref.PHYSICS_COUPLINGS, cols)
        results.append(out)
        neff.append(out["neff_fraction"])
    worst = pref.check_physics(results)
    print("largest deviation in standard errors", worst, "least neff_fraction", np.min(neff))
    assert worst <= 2.2 and np.min(neff) >= 0.55


def test_reference_with_zero_couplings_is_the_temperature_reweighting():
    energies, temps = ref.gamma_ladder(512, dim=16, seed=7)
    rungs = np.repeat(np.arange(temps.size), 512)
    e = energies.ravel()
    cols = np.stack([e, np.random.default_rng(3).standard_normal(e.size)])
    f, _, _, _ = ref.solve(e, rungs, temps)
    targets = [0.6, temps[3], 2.2]
    out = pref.reweight_perturbed(e, rungs, temps, f, targets, np.zeros((3, 2)), cols)
    ln_z, mean_e, var_e, neff = ref.reweight(e, rungs, temps, f, targets)
    mean, var, cov, _ = oref.reweight_observables(e, rungs, temps, f, targets, cols)
    for got, want in ((out["ln_z"], ln_z), (out["hamiltonian_mean"], mean_e), (out["hamiltonian_var"], var_e),
                      (out["neff_fraction"], neff), (out["mean"], mean), (out["var"], var), (out["cov_hamiltonian"], cov)):
        assert np.array_equal(got, want)
    # a coupling to the energy column is a temperature: lambda on column 0 at T is T / (1 + lambda)
    lam = 0.25
    a = pref.reweight_perturbed(e, rungs, temps, f, targets, [[lam, 0.0]] * 3, cols)
    b = ref.reweight(e, rungs, temps, f, np.asarray(targets) / (1 + lam))
    assert np.allclose(a["ln_z"], b[0], rtol=1e-12) and np.allclose(a["hamiltonian_mean"], (1 + lam) * b[1], rtol=1e-12)
    # a NaN of an uncoupled column stays out of the bias
    dirty = cols.copy()
    dirty[1, 17] = np.nan
    c = pref.reweight_perturbed(e, rungs, temps, f, targets, [[lam, 0.0]] * 3, dirty)
    assert np.array_equal(c["ln_z"], a["ln_z"]) and np.array_equal(c["mean"][:, 0], a["mean"][:, 0])
    assert not np.any(np.isfinite(c["mean"][:, 1]))


def test_case_couplings_mix_zero_and_nonzero_entries():
    lam = pref.case_couplings(9, 5)
    assert lam.shape == (9, 5) and lam[1, 0] == -0.05 and lam[0, 1] == -0.025 and lam[0, 0] == 0.0 and lam[1, 1] == 0.0
    assert np.all((lam != 0).any(axis=1)) and np.all((lam == 0).any(axis=1))
    assert pref.case_couplings(1, 1).tolist() == [[0.05]]


# --------------------------------------------------------------------------------------------------- 2. the validators

NAMES = ("real_0", "abs_real_0", "real_0_sq")


def test_couplings_as_arrays_and_dictionaries():
    v = statistics.validate_mbar_couplings
    lam = v([[1.0, 0.0, 2.0], [0.0, 0.5, 0.0]], 2, NAMES)
    assert lam.shape == (2, 3) and lam.dtype == np.float64 and lam.flags.c_contiguous
    assert v([1.0, 0.0, 2.0], 2, NAMES).tolist() == [[1.0, 0.0, 2.0]] * 2            # one row for every target
    assert v({"real_0": -0.3, "real_0_sq": [0.0, 0.2, 0.4]}, 3, NAMES).tolist() == [[-0.3, 0.0, 0.0], [-0.3, 0.0, 0.2],
                                                                                     [-0.3, 0.0, 0.4]]
    assert v({2: 1.5, np.int64(0): [1.0, 2.0]}, 2, NAMES).tolist() == [[1.0, 0.0, 1.5], [2.0, 0.0, 1.5]]
    assert v({}, 2, NAMES).tolist() == [[0.0] * 3] * 2
    assert v({0: 1.0}, 1, (0, 1)).tolist() == [[1.0, 0.0]]                            # the engine-less form: numbers as names


@pytest.mark.parametrize("bad, n_targets", [
    ([[1.0, 0.0]], 1), ([[1.0, 0.0, 0.0]], 2), ([1.0, 0.0], 2), (1.0, 1), (np.zeros((1, 1, 3)), 1),      # shapes
    ({"real_1": 1.0}, 1), ({3: 1.0}, 1), ({-1: 1.0}, 1), ({1.5: 1.0}, 1), ({True: 1.0}, 1),              # unknown columns
    ({"real_0": 1.0, 0: 2.0}, 1),                                                                        # a column named twice
    ({"real_0": [1.0, 2.0]}, 3), ({"real_0": [[1.0]]}, 1),                                               # values of another length
    ([[np.nan, 0.0, 0.0]], 1), ({"real_0": np.inf}, 1), ({"real_0_sq": [0.0, -np.inf]}, 2)])             # non-finite
def test_bad_couplings_are_refused_before_the_library(bad, n_targets):
    with pytest.raises(ValueError):
        statistics.validate_mbar_couplings(bad, n_targets, NAMES)


def test_a_scalar_temperature_serves_every_target():
    b = statistics.broadcast_mbar_targets
    assert b(1.5, np.zeros((4, 3))).tolist() == [1.5] * 4
    assert b([1.5], {"real_0": [0.0, 0.1, 0.2], "real_0_sq": 1.0}).tolist() == [1.5] * 3
    assert b(1.5, {"real_0": 1.0}).tolist() == [1.5] and b(1.5, [0.0, 1.0, 0.0]).tolist() == [1.5]
    assert b([1.0, 2.0], np.zeros((4, 3))).tolist() == [1.0, 2.0]       # (the mismatch is validate_mbar_couplings' to refuse)
    for temps in ([], 0.0, [1.0, -2.0], np.nan, [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            b(temps, np.zeros((1, 3)))


def test_bad_arguments_are_refused_before_the_library():
    good = dict(energies=[1.0, 2.0, 3.0], rungs=[0, 1, 1], temps=[1.0, 2.0], f=[0.0, 0.1], targets=[1.5, 2.5],
                couplings=np.zeros((2, 2)), observables=np.ones((2, 3)))
    for key, value in (("couplings", np.zeros((2, 3))), ("couplings", np.zeros((3, 2))), ("couplings", {2: 1.0}),
                       ("couplings", {"real_0": 1.0}), ("couplings", [[np.nan, 0.0]] * 2), ("targets", [1.0, 0.0]),
                       ("observables", np.ones((2, 4))), ("observables", np.ones((17, 3))), ("f", [0.0]), ("rungs", [0, 1, 2])):
        with pytest.raises(ValueError):
            statistics.mbar_reweight_perturbed(**dict(good, **{key: value}))
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)      # no device: the temperatures come first
    for temps in ([], [0.0], [np.nan]):
        with pytest.raises(ValueError):
            eng.reweight_perturbed(temps, {"real_0": 1.0})


def test_result_dictionary():
    t = np.array([0.5, 2.0])
    lam = np.array([[1.0, 0.0], [0.0, -2.0]])
    mean = np.array([[3.0, np.nan], [np.nan, 5.0]])             # (an uncoupled column's mean is not read)
    cov = np.array([[1.0, 2.0], [4.0, 8.0]])
    out = statistics._perturbed_result(t, lam, ["a", "b"], np.zeros(2), np.ones(2), np.array([1.0, 8.0]), mean, np.ones((2, 2)), cov,
                                       np.ones(2))
    assert set(out) == {"temps", "couplings", "names", "ln_z", "hamiltonian_mean", "hamiltonian_var", "heat_capacity",
                        "perturbation_mean", "mean", "var", "cov_hamiltonian", "dmean_dT", "neff_fraction"}
    assert out["names"] == ("a", "b") and out["heat_capacity"].tolist() == [4.0, 2.0]
    assert out["perturbation_mean"].tolist() == [3.0, -10.0] and np.array_equal(out["dmean_dT"], [[4.0, 8.0], [1.0, 2.0]])
