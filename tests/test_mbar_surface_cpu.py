"""Joint reweighted histograms and free-energy surfaces without a GPU: the C ABI's new exports, the Python-side validation,
the result dictionary, the numpy restatement (tests/mbar_surface_reference.py) against np.histogram2d and against the 1-D
restatement, and that restatement against the exact cell probabilities of a quadratic energy -- on the very inputs
tests/test_gpu_mbar_surface.py gives the device."""
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref
import mbar_observables_reference as oref
import mbar_profile_reference as pref
import mbar_surface_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["me_mbar_histogram_joint", "me_mbar_histogram_joint_samples"]
UNEVEN = [-2.0, -0.5, -0.25, 0.0, 0.125, 1.0, 4.0]
GOOD = [0.0, 1.0, 2.0]
HOST = dict(energies=[1.0, 2.0, 3.0], rungs=[0, 1, 1], temps=[1.0, 2.0], f=[0.0, 0.1], targets=[1.5], values_x=[0.1, 0.2, 0.3],
            edges_x=GOOD, values_y=[0.5, 1.5, 2.5], edges_y=GOOD)


def test_header_binding_and_build_list_the_new_unit():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^\s*int\s+(me_[a-z_0-9]+)\s*\(", text, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    assert "#define ME_MAX_HISTOGRAM2D_SLOTS 1296" in text and statistics.MBAR_MAX_HISTOGRAM2D_SLOTS == 1296
    assert len(_capi.SYMBOLS["me_mbar_histogram_joint"][1]) == 13 and len(_capi.SYMBOLS["me_mbar_histogram_joint_samples"][1]) == 18
    from metropolisengine_amd import build
    assert "me_mbar_hist2d" in [name for name, _ in build.HOST_UNITS]
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar_hist2d.hip"))


# ---------------------------------------------------------------------------------------------------- host logic


def _no_device_engine():
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)      # no device: validation comes first
    eng.num_real_params, eng.num_complex_params, eng.energy_term_names = 2, 1, ["total"]
    return eng


@pytest.mark.parametrize("edges", [[0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, np.inf], [-np.inf, 0.0], [1.0], [],
                                   np.arange(258.0), [[0.0, 1.0]], 1.0])
@pytest.mark.parametrize("axis", ["x", "y"])
def test_bad_edges_on_either_axis_are_refused_before_the_library(edges, axis):
    ex, ey = (edges, GOOD) if axis == "x" else (GOOD, edges)
    with pytest.raises(ValueError):
        statistics.validate_histogram2d_edges(ex, ey)
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_surface("energy", ex, "energy", ey, [1.0])
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface(**dict(HOST, edges_x=ex, edges_y=ey))


def test_the_slot_cap_is_refused_before_the_library():
    ex, ey = statistics.validate_histogram2d_edges(np.arange(34.0), np.arange(34.0))         # 33 x 33 bins: 36 x 36 cells
    assert ex.size == ey.size == 34
    assert statistics.validate_histogram2d_edges(np.arange(257.0), [0.0, 1.0, 2.0])[0].size == 257   # 259 x 5 = 1295 cells
    for bx, by in ((34, 33), (33, 34), (256, 3), (3, 256), (256, 256)):
        with pytest.raises(ValueError, match="at most 1296 cells"):
            statistics.validate_histogram2d_edges(np.arange(bx + 1.0), np.arange(by + 1.0))
        with pytest.raises(ValueError, match="at most 1296 cells"):
            _no_device_engine().free_energy_surface("energy", np.arange(bx + 1.0), "energy", np.arange(by + 1.0), [1.0])
        with pytest.raises(ValueError, match="at most 1296 cells"):
            statistics.mbar_free_energy_surface(**dict(HOST, edges_x=np.arange(bx + 1.0), edges_y=np.arange(by + 1.0)))


@pytest.mark.parametrize("temps", [[], [0.0], [1.0, -2.0], [np.nan], [np.inf, 1.0], [[1.0, 2.0]]])
def test_bad_target_temperatures_are_refused_before_the_library(temps):
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_surface("energy", GOOD, "energy", GOOD, temps)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface(**dict(HOST, targets=temps))


def test_bad_engine_less_arguments_are_refused_before_the_library():
    for key, value in (("values_x", [0.1, 0.2]), ("values_y", [0.1, 0.2]), ("values_x", np.ones((2, 3))), ("values_y", np.ones(4)),
                       ("f", [0.0]), ("f", [0.0, np.nan]), ("rungs", [0, 1, 2]), ("energies", [1.0, 2.0]), ("temps", [1.0, 0.0])):
        with pytest.raises(ValueError):
            statistics.mbar_free_energy_surface(**dict(HOST, **{key: value}))


def test_result_dictionary():
    ex, ey = statistics.validate_histogram2d_edges([0.0, 1.0, 3.0], [-1.0, 3.0])         # 2 x 1 bins: a 5 x 4 table
    t = np.array([0.5, 2.0])
    first = np.array([[0.25, 0.03125, 0.0, 0.0], [0.5, 0.0, 0.0625, 0.0], [0.0, 0.03125, 0.0, 0.0], [0.0625, 0.0, 0.03125, 0.0],
                      [0.015625, 0.0, 0.0, 0.015625]])
    second = np.zeros((5, 4))
    second[1, 0] = 1.0
    mass = np.stack([first, second])
    assert mass.sum(axis=(1, 2)).tolist() == [1.0, 1.0]
    counts = np.arange(20, dtype=np.int64).reshape(5, 4)
    out = statistics._surface_result(t, ex, ey, mass, counts, np.ones(2))
    assert set(out) == {"temps", "edges_x", "edges_y", "centers_x", "centers_y", "widths_x", "widths_y", "mass", "density",
                        "free_energy", "mass_slots", "outside", "counts", "counts_slots", "neff_fraction"}
    assert out["centers_x"].tolist() == [0.5, 2.0] and out["widths_x"].tolist() == [1.0, 2.0]
    assert out["centers_y"].tolist() == [1.0] and out["widths_y"].tolist() == [4.0]
    assert out["mass"].shape == (2, 2, 1) and out["mass"].tolist() == [[[0.25], [0.5]], [[0.0], [1.0]]]
    assert out["density"].shape == (2, 2, 1) and out["density"].tolist() == [[[0.0625], [0.0625]], [[0.0], [0.125]]]
    assert out["free_energy"].shape == (2, 2, 1)
    assert np.array_equal(out["free_energy"], [[[-0.5 * np.log(0.0625)]] * 2, [[np.inf], [-2.0 * np.log(0.125)]]])
    assert out["mass_slots"].shape == (2, 5, 4) and np.array_equal(out["mass_slots"], mass)
    assert out["outside"].shape == (2,) and out["outside"].tolist() == [0.25, 0.0]
    assert out["counts"].shape == (2, 1) and out["counts"].dtype == np.int64 and out["counts"].tolist() == [[0], [4]]
    assert out["counts_slots"].shape == (5, 4) and out["counts_slots"].dtype == np.int64 and np.array_equal(out["counts_slots"], counts)
    assert out["neff_fraction"].shape == (2,) and out["temps"] is t and out["edges_x"] is ex and out["edges_y"] is ey
    # the sums of the table over an axis are the 1-D tables of the other, outer slots included
    assert out["mass_slots"][0].sum(axis=1).tolist() == [0.28125, 0.5625, 0.03125, 0.09375, 0.03125]
    assert out["mass_slots"][0].sum(axis=0).tolist() == [0.828125, 0.0625, 0.09375, 0.015625]


# ---------------------------------------------------------------------------------------------------- the reference


def _gamma_problem(n_per_rung=512, seed=7):
    energies, temps = ref.gamma_ladder(n_per_rung, dim=16, seed=seed)
    rungs = np.repeat(np.arange(temps.size), n_per_rung)
    e = energies.ravel().copy()
    f, _, _, _ = ref.solve(e, rungs, temps)
    rng = np.random.default_rng(3)
    a = 0.2 * e - 1.5 + 0.3 * rng.standard_normal(e.size)
    b = np.sqrt(e) + 0.25 * rng.standard_normal(e.size)
    a[[7, 100, 900]] = [np.nan, np.inf, np.nan]
    b[[9, 100, 900, 1200]] = [np.nan, -np.inf, np.nan, np.inf]
    return e, rungs, temps, f, a, b


EDGES_B = np.array([0.5, 1.5, 2.0, 2.75, 3.0, 4.5])


def test_reference_agrees_with_np_histogram2d_inside():
    e, rungs, temps, f, a, b = _gamma_problem()
    ex, ey = statistics.validate_histogram2d_edges(UNEVEN, EDGES_B)
    bx, by = ex.size - 1, ey.size - 1
    targets = [0.6, temps[3], 2.2]
    mass, counts, neff = sref.histogram2d(e, rungs, temps, f, targets, a, ex, b, ey)
    assert mass.shape == (3, bx + 3, by + 3) and counts.shape == (bx + 3, by + 3) and counts.dtype == np.int64
    assert np.max(np.abs(mass.reshape(3, -1).sum(axis=1) - 1.0)) <= 1e-13
    assert counts.sum() == e.size and counts[bx + 2, by + 2] == 1 and counts[bx + 2].sum() == 2 and counts[:, by + 2].sum() == 2
    assert counts[bx + 1, by] == 1                              # (+inf, -inf)
    assert np.all(mass[:, counts == 0] == 0.0) and np.all(mass[:, counts > 0] > 0.0)
    assert np.allclose(neff, ref.reweight(e, rungs, temps, f, targets)[3], rtol=1e-13)
    # np.histogram2d closes its last bins: keep the last edges out
    keep = np.isfinite(a) & np.isfinite(b) & (a < ex[-1]) & (b < ey[-1])
    assert np.array_equal(counts[:bx, :by], np.histogram2d(a[keep], b[keep], bins=[ex, ey])[0].astype(np.int64))
    for i, t in enumerate(targets):
        l = -e / t - np.log(np.exp(np.log(np.bincount(rungs))[None, :] + f[None, :] - e[:, None] / temps[None, :]).sum(axis=1))
        w = np.exp(l - l.max())
        w /= w.sum()
        want = np.histogram2d(a[keep], b[keep], bins=[ex, ey], weights=w[keep])[0]
        assert np.allclose(mass[i, :bx, :by], want, rtol=1e-11, atol=0)
    ld = sref.histogram2d(e, rungs, temps, f, targets, a, ex, b, ey, dtype=np.longdouble)
    assert ld[0].dtype == np.longdouble
    assert np.allclose(mass, ld[0].astype(np.float64), rtol=1e-11, atol=0) and np.array_equal(counts, ld[1])


def test_sums_over_an_axis_are_the_one_dimensional_reference():
    e, rungs, temps, f, a, b = _gamma_problem()
    e = e.copy()
    e[[5, 700]] = [np.nan, np.inf]                              # unused samples
    targets = [0.6, temps[3], 2.2]
    mass, counts, neff = sref.histogram2d(e, rungs, temps, f, targets, a, UNEVEN, b, EDGES_B)
    assert counts.sum() == e.size - 2
    for axis, values, edges in ((2, a, UNEVEN), (1, b, EDGES_B)):
        one = pref.histogram(e, rungs, temps, f, targets, values, edges)
        assert np.array_equal(counts.sum(axis=axis - 1), one[1])
        assert np.max(np.abs(mass.sum(axis=axis) - one[0])) <= 1e-13 and np.array_equal(neff, one[2])
    # the same column twice fills the diagonal only
    twice = sref.histogram2d(e, rungs, temps, f, targets, a, UNEVEN, a, UNEVEN)
    one = pref.histogram(e, rungs, temps, f, targets, a, UNEVEN)
    assert np.array_equal(np.diagonal(twice[1]), one[1]) and twice[1].sum() == one[1].sum()
    assert np.max(np.abs(np.diagonal(twice[0], axis1=1, axis2=2) - one[0])) <= 1e-13


def test_reference_meets_the_statistical_condition_of_the_gpu_test():
    """The GPU test asks that the device's masses of (x_0, x_1) from sref.xy_quadratic_subsets() -- 16 independent subsets of
    exact samples of E = |x|^2 in 4 dimensions on LADDER8 -- in the 4 x 4 bins of SURFACE_EDGES_X and SURFACE_EDGES_Y, below
    and above on both axes lie within 5 standard errors of the exact probabilities (products of the 1-D ones: x_0 and x_1 are
    independent) at three temperatures between rungs: 3 x 6 x 6 comparisons.  The reference meets all of them on the same inputs
    (same generator, same seed); different edges per axis make a transposed table fail."""
    results = []
    for e, rungs, cols in sref.xy_quadratic_subsets():
        f, _, residual, _ = ref.solve(e, rungs, oref.LADDER8, tol=1e-10)
        assert residual <= 1e-10
        results.append(sref.histogram2d(e, rungs, oref.LADDER8, f, oref.PHYSICS_TARGETS, cols[0], sref.SURFACE_EDGES_X, cols[1],
                                        sref.SURFACE_EDGES_Y)[0])
    est, exact = sref.physics_masses(results, oref.PHYSICS_TARGETS)
    assert np.max(np.abs(exact.sum(axis=(1, 2)) - 1.0)) <= 1e-15
    ok, m, se = ref.within_5_se(est, exact)
    dev = np.abs(m - exact) / se
    print("largest deviation / se", dev.max(), "least exact mass", exact.min(), "\n", dev)
    assert ok.shape == (3, 6, 6) and np.all(ok)
    wrong, _, _ = ref.within_5_se(est.transpose(0, 1, 3, 2), exact)
    assert not np.all(wrong)
