"""Reweighted histograms and free-energy profiles without a GPU: the C ABI's new exports, the Python-side validation, the
slot rule and the masses of the numpy restatement (tests/mbar_profile_reference.py), and that restatement against the exact
bin probabilities of a quadratic energy -- on the very inputs tests/test_gpu_mbar_profile.py gives the device."""
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
from metropolisengine_amd.statistics import validate_histogram_edges       # (every test of this file goes through it)
import mbar_reference as ref
import mbar_observables_reference as oref
import mbar_profile_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["me_mbar_histogram", "me_mbar_histogram_samples"]
UNEVEN = [-2.0, -0.5, -0.25, 0.0, 0.125, 1.0, 4.0]


def test_header_binding_and_build_list_the_new_unit():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^\s*int\s+(me_[a-z_]+)\s*\(", text, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    assert "#define ME_MAX_HISTOGRAM_BINS 256" in text and statistics.MBAR_MAX_HISTOGRAM_BINS == 256
    assert validate_histogram_edges(np.arange(257.0)).size == 257
    from metropolisengine_amd import build
    assert "me_mbar_hist" in [name for name, _ in build.HOST_UNITS]
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar_hist.hip"))


# ---------------------------------------------------------------------------------------------------- host logic


def _no_device_engine():
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)      # no device: validation comes first
    eng.num_real_params, eng.num_complex_params, eng.energy_term_names = 2, 1, ["total"]
    return eng


@pytest.mark.parametrize("edges", [[0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf], [-np.inf, 0.0], [1.0], [],
                                   np.arange(258.0), [[0.0, 1.0]], 1.0])
def test_bad_edges_are_refused_before_the_library(edges):
    with pytest.raises(ValueError):
        validate_histogram_edges(edges)
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_profile("energy", edges, [1.0])
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], [1.5], [0.5, 0.25], edges)


@pytest.mark.parametrize("temps", [[], [0.0], [1.0, -2.0], [np.nan], [np.inf, 1.0], [[1.0, 2.0]]])
def test_bad_target_temperatures_are_refused_before_the_library(temps):
    edges = validate_histogram_edges([0.0, 1.0])
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_profile("energy", edges, temps)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1], temps, [0.5, 0.25], edges)


def test_bad_engine_less_arguments_are_refused_before_the_library():
    good = dict(energies=[1.0, 2.0, 3.0], rungs=[0, 1, 1], temps=[1.0, 2.0], f=[0.0, 0.1], targets=[1.5],
                values=[0.1, 0.2, 0.3], edges=validate_histogram_edges([0.0, 1.0]))
    for key, value in (("values", [0.1, 0.2]), ("values", np.ones((2, 3))), ("f", [0.0]), ("f", [0.0, np.nan]),
                       ("rungs", [0, 1, 2]), ("energies", [1.0, 2.0]), ("temps", [1.0, 0.0])):
        with pytest.raises(ValueError):
            statistics.mbar_free_energy_profile(**dict(good, **{key: value}))


def test_result_dictionary():
    edges = validate_histogram_edges([0.0, 1.0, 3.0])
    t = np.array([0.5, 2.0])
    mass = np.array([[0.25, 0.5, 0.125, 0.0625, 0.0625], [0.0, 1.0, 0.0, 0.0, 0.0]])
    counts = np.array([3, 9, 2, 1, 1], dtype=np.int64)
    out = statistics._profile_result(t, edges, mass, counts, np.ones(2))
    assert set(out) == {"temps", "edges", "centers", "widths", "mass", "below", "above", "not_a_number", "density", "free_energy",
                        "counts", "counts_outside", "neff_fraction"}
    assert out["centers"].tolist() == [0.5, 2.0] and out["widths"].tolist() == [1.0, 2.0]
    assert out["mass"].tolist() == [[0.25, 0.5], [0.0, 1.0]] and out["below"].tolist() == [0.125, 0.0]
    assert out["above"].tolist() == [0.0625, 0.0] and out["not_a_number"].tolist() == [0.0625, 0.0]
    assert out["density"].tolist() == [[0.25, 0.25], [0.0, 0.5]]
    assert out["counts"].tolist() == [3, 9] and out["counts_outside"].tolist() == [2, 1, 1]
    assert np.array_equal(out["free_energy"], [[-0.5 * np.log(0.25)] * 2, [np.inf, -2.0 * np.log(0.5)]])


# ---------------------------------------------------------------------------------------------------- the slot rule


def test_slot_rule_on_edges_infinities_and_nan():
    edges = validate_histogram_edges(UNEVEN)                     # 6 bins of uneven widths: below = 6, above = 7, NaN = 8
    b = edges.size - 1
    assert pref.slots(edges, edges).tolist() == [0, 1, 2, 3, 4, 5, b + 1]           # a value ON the last edge lies above
    assert pref.slots(np.nextafter(edges, -np.inf), edges).tolist() == [b, 0, 1, 2, 3, 4, 5]
    assert pref.slots(np.nextafter(edges, np.inf), edges).tolist() == [0, 1, 2, 3, 4, 5, b + 1]
    assert pref.slots([-np.inf, np.inf, np.nan, -0.0, 0.0, 3.999], edges).tolist() == [b, b + 1, b + 2, 3, 3, 5]
    rng = np.random.default_rng(1)
    a = rng.uniform(-3.0, 5.0, size=4000)
    want = np.searchsorted(edges, a, side="right") - 1
    got = pref.slots(a, edges)
    inside = (want >= 0) & (want < b)
    assert np.array_equal(got[inside], want[inside]) and np.all(got[want < 0] == b) and np.all(got[want >= b] == b + 1)


def test_slot_rule_with_one_bin():
    edges = validate_histogram_edges([-1.0, 1.0])
    assert pref.slots([-1.0, 0.0, 1.0, -1.5, 2.0, np.nan, -np.inf, np.inf], edges).tolist() == [0, 0, 2, 1, 2, 3, 1, 2]


# ---------------------------------------------------------------------------------------------------- the masses


def _gamma_problem(n_per_rung=512, seed=7):
    energies, temps = ref.gamma_ladder(n_per_rung, dim=16, seed=seed)
    rungs = np.repeat(np.arange(temps.size), n_per_rung)
    e = energies.ravel().copy()
    f, _, _, _ = ref.solve(e, rungs, temps)
    return e, rungs, temps, f


def test_masses_sum_to_one_and_agree_with_np_histogram_inside():
    e, rungs, temps, f = _gamma_problem()
    rng = np.random.default_rng(3)
    a = 0.2 * e - 1.5 + 0.3 * rng.standard_normal(e.size)
    a[[7, 100]] = [np.nan, np.inf]
    edges = validate_histogram_edges(UNEVEN)
    b = edges.size - 1
    targets = [0.6, temps[3], 2.2]
    mass, counts, neff = pref.histogram(e, rungs, temps, f, targets, a, edges)
    assert mass.shape == (3, b + 3) and counts.shape == (b + 3,) and counts.dtype == np.int64
    assert np.max(np.abs(mass.sum(axis=1) - 1.0)) <= 1e-13
    assert counts.sum() == e.size and counts[b + 2] == 1 and np.all(counts[:b] > 0)
    assert np.allclose(neff, ref.reweight(e, rungs, temps, f, targets)[3], rtol=1e-13)
    inner = a[np.isfinite(a) & (a < edges[-1])]                  # (np.histogram closes its last bin: keep the last edge out)
    assert np.array_equal(counts[:b], np.histogram(inner, bins=edges)[0])
    for i, t in enumerate(targets):
        l = -e / t - np.log(np.exp(np.log(np.bincount(rungs))[None, :] + f[None, :] - e[:, None] / temps[None, :]).sum(axis=1))
        w = np.exp(l - l.max())
        w /= w.sum()
        keep = np.isfinite(a) & (a < edges[-1])
        want = np.histogram(a[keep], bins=edges, weights=w[keep])[0]
        assert np.allclose(mass[i, :b], want, rtol=1e-11, atol=0)
    ld = pref.histogram(e, rungs, temps, f, targets, a, edges, dtype=np.longdouble)
    assert np.allclose(mass, ld[0].astype(np.float64), rtol=1e-11) and np.array_equal(counts, ld[1])


def test_samples_with_non_finite_energies_are_not_used():
    e, rungs, temps, f = _gamma_problem()
    a = np.sqrt(e)
    edges = validate_histogram_edges(np.linspace(0.5, 4.0, 9))
    dirty, dirty_a = e.copy(), a.copy()
    dirty[[5, 700, 3000]] = [np.nan, np.inf, -np.inf]
    dirty_a[700] = np.nan                                        # of an unused sample: never seen
    keep = np.isfinite(dirty)
    x = pref.histogram(dirty, rungs, temps, f, [0.7, 1.9], dirty_a, edges)
    y = pref.histogram(dirty[keep], rungs[keep], temps, f, [0.7, 1.9], dirty_a[keep], edges)
    for p, q in zip(x, y):
        assert np.array_equal(p, q)
    assert x[1].sum() == keep.sum() and x[1][-1] == 0


def test_exact_probabilities_of_the_quadratic_energy():
    edges = validate_histogram_edges(pref.PROFILE_EDGES)
    for t in oref.PHYSICS_TARGETS:
        p = pref.exact_x0_masses(edges, t)
        assert p.shape == (14,) and abs(p.sum() - 1.0) <= 1e-15 and np.allclose(p[:12], p[:12][::-1], rtol=1e-12)
        x = np.linspace(-1.5, 1.5, 12 * 2000 + 1)               # Simpson against the density sqrt(a / pi T) exp(-a x^2 / T)
        dens = np.exp(-x * x / t) / np.sqrt(np.pi * t)
        h = x[1] - x[0]
        simpson = (h / 3.0) * (dens[0:-1:2] + 4.0 * dens[1::2] + dens[2::2]).reshape(12, 1000).sum(axis=1)
        assert np.allclose(p[:12], simpson, rtol=1e-10)


def test_reference_meets_the_statistical_condition_of_the_gpu_test():
    """The GPU test asks that the device's masses of x_0 from oref.iso_quadratic_subsets() -- 16 independent subsets of exact
    samples of E = |x|^2 in 4 dimensions on LADDER8 -- in the 12 bins of linspace(-1.5, 1.5, 13), below and above lie within 5
    standard errors of the exact probabilities at three temperatures between rungs: 3 x 14 comparisons.  The reference meets
    all of them on the same inputs (same generator, same seed)."""
    edges = validate_histogram_edges(pref.PROFILE_EDGES)
    results = []
    for e, rungs, cols in oref.iso_quadratic_subsets():
        f, _, residual, _ = ref.solve(e, rungs, oref.LADDER8, tol=1e-10)
        assert residual <= 1e-10
        results.append(pref.histogram(e, rungs, oref.LADDER8, f, oref.PHYSICS_TARGETS, cols[0], edges)[0])
    est, exact = pref.physics_masses(results, oref.PHYSICS_TARGETS)
    ok, m, se = ref.within_5_se(est, exact)
    dev = np.abs(m - exact) / se
    print("largest deviation / se", dev.max(), "\n", dev)
    assert ok.shape == (3, 14) and np.all(ok)
