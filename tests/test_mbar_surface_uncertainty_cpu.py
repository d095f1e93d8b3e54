"""Error bars of joint reweighted histograms and free-energy surfaces without a GPU: the C ABI's new exports, the Python-side
validation, the reduced K x K host algebra of metropolisengine_amd/statistics.py on the long-double cell Gram sums against the
SVD route of the explicit weight matrix [ladder | state | one column per live cell], the result dictionary, and the calibration
of the reference's error bars against exact cell probabilities -- on the very inputs
tests/test_gpu_mbar_surface_uncertainty.py gives the device."""
import functools
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_observable_uncertainty_reference as oref
import mbar_surface_reference as sref
import mbar_surface_uncertainty_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["me_mbar_histogram_joint_gram", "me_mbar_histogram_joint_gram_samples"]
NEW_KEYS = {"d_mass", "d_mass_slots", "d_outside", "d_free_energy", "lowest", "d_free_energy_from_lowest", "log_mass_cov", "n_samples"}
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
        assert hasattr(_capi.load(), name), name
    # the twins take the arguments of me_mbar_histogram_joint[_samples] with cell_gram, ladder_gram, column_counts before the
    # outputs and n_used behind them
    for old, new in (("me_mbar_histogram_joint", NEW_EXPORTS[0]), ("me_mbar_histogram_joint_samples", NEW_EXPORTS[1])):
        a, b = _capi.SYMBOLS[old][1], _capi.SYMBOLS[new][1]
        assert len(b) == len(a) + 4 and b[:len(a) - 3] == a[:-3] and b[-4:-1] == a[-3:]
    from metropolisengine_amd import build
    units = [name for name, _ in build.HOST_UNITS]
    assert units.index("me_mbar_hist2d_cov") == units.index("me_mbar_hist2d") + 1
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar_hist2d_cov.hip"))
    assert hasattr(me.MetropolisEngine, "free_energy_surface_uncertainties")
    assert hasattr(statistics, "mbar_free_energy_surface_uncertainties")


def test_the_rows_rule_of_the_test_grids():
    """The table of grids that tests/test_gpu_mbar_surface_uncertainty.py runs, against ref.rule_rows, this suite's own
    restatement of the rule: every R has a grid, and the restatement has the thresholds that csrc/me_mbar_hist2d_cov.hip pins
    with static_asserts.  It guards the table, not the library: the kernel's choice of R is pinned by those static_asserts
    alone, so this test passes without the feature too."""
    for name, rows in ref.ROWS.items():
        ex, ey = ref.GRIDS[name]
        assert ref.rule_rows((ex.size + 2) * (ey.size + 2)) == rows, name
    assert sorted(set(ref.ROWS.values())) == [1, 2, 4, 8, 16]
    assert [ref.rule_rows(s) for s in (106, 107, 211, 212, 420, 421, 827, 828, 1296)] == [16, 8, 8, 4, 4, 2, 2, 1, 1]


# ---------------------------------------------------------------------------------------------------- validation
def _no_device_engine():
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)      # no device: validation comes first
    eng.num_real_params, eng.num_complex_params, eng.energy_term_names = 2, 1, ["total"]
    return eng


@pytest.mark.parametrize("edges", [[0.0, 1.0, 1.0], [0.0, np.nan, 1.0], [1.0], np.arange(258.0)])
@pytest.mark.parametrize("axis", ["x", "y"])
def test_bad_edges_are_refused_before_the_library(edges, axis):
    ex, ey = (edges, GOOD) if axis == "x" else (GOOD, edges)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface_uncertainties(**dict(HOST, edges_x=ex, edges_y=ey))
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_surface_uncertainties("energy", ex, "energy", ey, [1.0])


def test_the_cell_cap_is_refused_before_the_library():
    for bx, by in ((34, 33), (33, 34), (256, 3)):
        ex, ey = np.arange(bx + 1.0), np.arange(by + 1.0)
        with pytest.raises(ValueError, match="at most 1296 cells"):
            statistics.mbar_free_energy_surface_uncertainties(**dict(HOST, edges_x=ex, edges_y=ey))
        with pytest.raises(ValueError, match="at most 1296 cells"):
            _no_device_engine().free_energy_surface_uncertainties("energy", ex, "energy", ey, [1.0])


@pytest.mark.parametrize("temps", [[], [0.0], [np.nan], [[1.0, 2.0]]])
def test_bad_targets_and_values_are_refused_before_the_library(temps):
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface_uncertainties(**dict(HOST, targets=temps))
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_surface_uncertainties("energy", GOOD, "energy", GOOD, temps)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface_uncertainties(**dict(HOST, values_y=[0.5, 1.5]))


@pytest.mark.parametrize("inefficiency", [0.99, -2.0, np.nan, np.inf, [1.0, 2.0], np.ones((1, 1))])
def test_bad_inefficiency_is_refused_before_the_library(inefficiency):
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface_uncertainties(**HOST, inefficiency=inefficiency)
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_surface_uncertainties("energy", GOOD, "energy", GOOD, [1.0], inefficiency=inefficiency)


@pytest.mark.parametrize("covariance", [None, 1, 0, "yes", 1.0, [True], np.array([True])])
def test_a_covariance_that_is_no_bool_is_refused_before_the_library(covariance):
    with pytest.raises(ValueError, match="covariance must be True or False"):
        statistics.mbar_free_energy_surface_uncertainties(**HOST, covariance=covariance)
    with pytest.raises(ValueError, match="covariance must be True or False"):
        _no_device_engine().free_energy_surface_uncertainties("energy", GOOD, "energy", GOOD, [1.0], covariance=covariance)
    assert statistics.validate_surface_covariance(np.bool_(False)) is False and statistics.validate_surface_covariance(True) is True


# ---------------------------------------------------------------- the reduced algebra against the explicit weight matrix
@functools.lru_cache(maxsize=None)
def _case(k, grid):
    """One target inside the ladder; everything in long double, computed once."""
    temps, energies, rungs = uref.synthetic(k)
    f = uref.solve(energies, rungs, temps)
    targets = uref.targets_for(temps, 1)
    x = ref.synthetic_values(energies, temps, rungs)
    y = ref.synthetic_values_y(energies, x)
    ex, ey = ref.GRIDS[grid]
    h, mass, counts, w, ladder_counts = ref.cell_gram(energies, rungs, temps, f, targets, x, ex, y, ey)
    explicit, live = ref.explicit_weight_matrix(w, k, 0, ref.cells_of(x, ex, y, ey), mass[0])
    cc = ref.column_counts(ladder_counts, live.size)
    theta = ref.theta_svd(explicit, cc)
    return dict(k=k, targets=targets, ex=ex, ey=ey, h=h, mass=mass, counts=counts, w=w, ladder_counts=ladder_counts,
                ladder=w[:, :k].T @ w[:, :k], live=live, explicit=explicit, cc=cc, theta=theta)


def _result(case, inefficiency=1.0, covariance=True):
    f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
    bx, by = case["ex"].size - 1, case["ey"].size - 1
    return statistics._surface_uncertainty_result(case["targets"], case["ex"], case["ey"], f64(case["mass"]).reshape(1, bx + 3, by + 3),
                                                  case["counts"].reshape(bx + 3, by + 3), np.ones(1), f64(case["h"]),
                                                  f64(case["ladder"]), f64(case["ladder_counts"]), uref.N_GRAM, inefficiency,
                                                  covariance)


@pytest.mark.parametrize("k,grid", [(8, "7x5"), (8, "13x9"), (33, "4x3"), (33, "12x7")])
def test_reduced_algebra_against_theta_of_the_explicit_weight_matrix(k, grid):
    """statistics._surface_uncertainty_result (one K x K pseudo-inverse, no matrix over the cells inverted) on the long-double
    sums rounded to float64, against ref.derived on Theta by the SVD route of the explicit (K + 1 + live)-column weight matrix.
    Every variance and covariance is a sum of four entries of Theta with coefficients of magnitude 1: within 4 b max |Theta|,
    b = ref.route_bound, the project's rule for two float64 routes.  7 x 5 holds most samples in its outer cells, 13 x 9 has
    empty cells."""
    case = _case(k, grid)
    ex, ey, t = case["ex"], case["ey"], case["targets"][0]
    bx, by = ex.size - 1, ey.size - 1
    out = _result(case)
    want = ref.derived(case["theta"], k, case["live"], case["mass"][0], t, ex, ey)
    top = np.abs(case["theta"]).max()
    bound = 4.0 * ref.route_bound(case["explicit"], case["cc"]) * top
    p = np.asarray(case["mass"][0], dtype=np.float64).reshape(bx + 3, by + 3)
    live = p > 0
    if grid == "13x9":
        assert (~live[:bx, :by]).sum() >= 4
    if grid == "7x5":
        assert live[bx:, :].sum() + live[:bx, by:].sum() >= 10 and out["outside"][0] > 0.3
    assert np.array_equal(out["lowest"][0], want["lowest"]) and out["d_free_energy_from_lowest"][0][tuple(want["lowest"])] == 0.0
    got = out["d_mass_slots"][0]
    err_var = np.abs((got[live] / p[live]) ** 2 - (want["d_slots"][live] / p[live]) ** 2).max()
    err_cov = np.nanmax(np.abs(out["log_mass_cov"][0] - want["log_mass_cov"]))
    err_low = np.nanmax(np.abs((out["d_free_energy_from_lowest"][0] / t) ** 2 - (want["d_free_energy_from_lowest"] / t) ** 2))
    err_free = np.nanmax(np.abs((out["d_free_energy"][0] / t) ** 2 - (want["d_free_energy"] / t) ** 2))
    # Var sum p_c = sum p_c p_c' C_cc' with sum p_c <= 1: the same four entries of Theta, weighted by at most 1
    err_out = abs(out["d_outside"][0] ** 2 - want["var_outside"])
    print("K = %d, %s (%d live cells): Var ln p %.3e, Cov %.3e, Var(ln p - ln p*) %.3e, Var outside %.3e (bound %.3e; max |Theta| %.3e)"
          % (k, grid, case["live"].size, err_var, err_cov, err_low, err_out, bound, top))
    assert max(err_var, err_cov, err_low, err_free, err_out) <= bound


@pytest.mark.parametrize("k,grid", [(8, "13x9"), (8, "7x5")])
def test_result_dictionary_shapes_nan_pattern_and_the_covariance_switch(k, grid):
    case = _case(k, grid)
    ex, ey = case["ex"], case["ey"]
    bx, by = ex.size - 1, ey.size - 1
    out, four, lean = _result(case), _result(case, 4.0), _result(case, 1.0, False)
    f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
    plain = statistics._surface_result(case["targets"], ex, ey, f64(case["mass"]).reshape(1, bx + 3, by + 3),
                                       case["counts"].reshape(bx + 3, by + 3), np.ones(1))
    assert set(out) == set(plain) | NEW_KEYS and set(lean) == set(out) - {"log_mass_cov"} and out["n_samples"] == uref.N_GRAM
    for key in plain:
        assert np.array_equal(out[key], plain[key]), key
    for key in lean:                                    # covariance=False: every other key bit for bit
        assert np.array_equal(np.asarray(lean[key]), np.asarray(out[key]), equal_nan=True), key
    assert out["d_mass"].shape == out["d_free_energy"].shape == out["d_free_energy_from_lowest"].shape == (1, bx, by)
    assert out["d_mass_slots"].shape == (1, bx + 3, by + 3) and out["d_outside"].shape == (1,)
    assert out["lowest"].shape == (1, 2) and out["log_mass_cov"].shape == (1, bx * by, bx * by)
    assert np.array_equal(out["d_mass"], out["d_mass_slots"][:, :bx, :by])
    for key in ("d_mass", "d_mass_slots", "d_outside", "d_free_energy", "d_free_energy_from_lowest"):
        assert np.array_equal(four[key], 2.0 * out[key], equal_nan=True), key
    assert np.array_equal(four["log_mass_cov"], 4.0 * out["log_mass_cov"], equal_nan=True)
    p = out["mass_slots"][0]
    empty = (p == 0)
    empty_inner = empty[:bx, :by]
    assert np.all(out["d_mass_slots"][0][empty] == 0) and np.all(np.isfinite(out["d_mass_slots"][0][~empty]))
    assert np.all(out["d_mass_slots"][0][~empty] > 0)
    assert np.array_equal(np.isnan(out["d_free_energy"][0]), empty_inner)
    assert np.array_equal(np.isnan(out["d_free_energy_from_lowest"][0]), empty_inner)
    flat = empty_inner.ravel()
    assert np.array_equal(np.isnan(out["log_mass_cov"][0]), flat[:, None] | flat[None, :])
    # the diagonal of log_mass_cov is (d_free_energy / T)^2, and d_free_energy = T d_mass / p: the same root
    t = case["targets"][0]
    diag = np.diag(out["log_mass_cov"][0]).reshape(bx, by)
    assert np.allclose(diag[~empty_inner], (out["d_free_energy"][0][~empty_inner] / t) ** 2, rtol=1e-9, atol=1e-12 * np.nanmax(diag))
    assert np.allclose(out["d_free_energy"][0][~empty_inner], t * out["d_mass"][0][~empty_inner] / p[:bx, :by][~empty_inner],
                       rtol=4 * 2.0 ** -52, atol=0)
    # the error of a difference from log_mass_cov is d_free_energy_from_lowest
    low = int(out["lowest"][0, 0]) * by + int(out["lowest"][0, 1])
    c = out["log_mass_cov"][0]
    var = np.diag(c) + c[low, low] - 2.0 * c[:, low]
    scale = np.nanmax(np.abs(c))
    assert np.nanmax(np.abs(var.reshape(bx, by) - (out["d_free_energy_from_lowest"][0] / t) ** 2)) <= 1e-9 * scale


@pytest.mark.parametrize("k,grid", [(8, "13x9"), (8, "7x5")])
def test_the_error_bars_are_bit_for_bit_those_recorded_before_the_algebra_was_shared(k, grid):
    """tests/golden/mbar_surface_uncertainty_result.npz holds what statistics._surface_uncertainty_result returned for these two
    cases (_result: this file's synthetic long-double sums rounded to float64, inefficiency 1, with the covariance) when it
    still carried the reduced algebra itself, before the profile's error bars moved onto it: the same operations in the same
    order, so every new key is equal on its bits, NaNs included."""
    with np.load(os.path.join(ROOT, "tests", "golden", "mbar_surface_uncertainty_result.npz")) as recorded:
        out = _result(_case(k, grid))
        for key in sorted(NEW_KEYS - {"n_samples"}):
            want = recorded["K=%d %s %s" % (k, grid, key)]
            assert out[key].shape == want.shape and out[key].dtype == want.dtype, key
            assert np.array_equal(out[key], want, equal_nan=True), key
            if want.dtype == np.float64:
                assert np.array_equal(np.signbit(out[key]), np.signbit(want)), key


def test_unresolved_cells_lose_their_error_bars_and_nothing_else():
    """A cell with positive mass whose sum of squared weights is no normal float64: NaN in d_mass too; an emptied cell: 0 and
    NaN; every other entry is what the input gives with both cells emptied, bit for bit (the algebra never sees them)."""
    case = _case(8, "7x5")
    ex, ey = case["ex"], case["ey"]
    bx, by = ex.size - 1, ey.size - 1
    f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
    mass, h = f64(case["mass"]).reshape(1, bx + 3, by + 3).copy(), f64(case["h"]).copy()
    a, b = (2, 1), (4, 3)
    ca, cb = a[0] * (by + 3) + a[1], b[0] * (by + 3) + b[1]
    assert mass[0][a] > 0 and mass[0][b] > 0
    mass[0][a], h[0, :, ca] = 1e-170, 0.0               # mass left, the squared weights underflowed
    h[0, :8, ca] = 1e-175
    mass[0][b], h[0, :, cb] = 0.0, 0.0                  # everything underflowed
    args = (case["targets"], ex, ey, mass, case["counts"].reshape(bx + 3, by + 3), np.ones(1), h, f64(case["ladder"]),
            f64(case["ladder_counts"]), uref.N_GRAM, 1.0, True)
    out = statistics._surface_uncertainty_result(*args)
    assert np.isnan(out["d_mass"][0][a]) and out["d_mass"][0][b] == 0.0
    for key in ("d_free_energy", "d_free_energy_from_lowest"):
        assert np.isnan(out[key][0][a]) and np.isnan(out[key][0][b]), key
    gone = np.zeros((bx, by), dtype=bool)
    gone[a] = gone[b] = True
    assert np.array_equal(np.isnan(out["d_free_energy"][0]), gone) and np.isfinite(out["free_energy"][0][a])
    emptied_mass, emptied_h = mass.copy(), h.copy()
    emptied_mass[0][a] = 0.0
    emptied_h[0, :, ca] = 0.0
    want = statistics._surface_uncertainty_result(args[0], ex, ey, emptied_mass, args[4], args[5], emptied_h, *args[7:])
    for key in ("d_mass", "d_free_energy", "d_free_energy_from_lowest"):
        assert np.array_equal(out[key][0][~gone], want[key][0][~gone]), key
    assert np.array_equal(out["d_outside"], want["d_outside"]) and np.array_equal(out["lowest"], want["lowest"])
    kept = ~gone.ravel()
    assert np.array_equal(out["log_mass_cov"][0][np.ix_(kept, kept)], want["log_mass_cov"][0][np.ix_(kept, kept)])


# ------------------------------------------------------------------------------------------------------- calibration
def calibration_included(targets):
    """The cells of the calibration: those whose EXACT probability is at least ref.CAL_MIN_PROBABILITY, ``(T, Bx + 2, By + 2)``
    booleans over the bins, below and above of both axes."""
    _, exact = sref.physics_masses([], targets, ref.CAL_EDGES_X, ref.CAL_EDGES_Y)
    return exact >= ref.CAL_MIN_PROBABILITY, exact


def test_reference_error_bars_are_calibrated():
    """64 independent subsets of 8 x 512 exact samples of E = |x|^2 on LADDER8, (x_0, x_1) on the 4 x 4 calibration grid at
    PHYSICS_TARGETS: the RMS over the subsets of (mass - exact) / d_mass of every cell whose exact probability is at least
    ref.CAL_MIN_PROBABILITY lies inside the project's CAL_RMS_Z; at least 12 cells per temperature qualify."""
    ex, ey, targets, k = ref.CAL_EDGES_X, ref.CAL_EDGES_Y, oref.PHYSICS_TARGETS, 8
    included, exact = calibration_included(targets)
    assert np.all(included.reshape(targets.size, -1).sum(axis=1) >= 12)
    z = []
    for e, rungs, cols in ref.calibration_subsets():
        f = uref.solve(e, rungs, oref.LADDER8)
        h, mass, counts, w, ladder_counts = ref.cell_gram(e, rungs, oref.LADDER8, f, targets, cols[0], ex, cols[1], ey)
        f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
        out = statistics._surface_uncertainty_result(targets, ex, ey, f64(mass).reshape(targets.size, 7, 7), counts.reshape(7, 7),
                                                     np.ones(targets.size), f64(h), f64(w[:, :k].T @ w[:, :k]), f64(ladder_counts),
                                                     e.size, 1.0, False)
        with np.errstate(divide="ignore", invalid="ignore"):
            z.append((out["mass_slots"][:, :6, :6] - exact) / out["d_mass_slots"][:, :6, :6])
    z = np.array(z)
    rms = np.sqrt((z[:, included] ** 2).mean(axis=0))
    lo, hi = uref.CAL_RMS_Z
    print("rms z of the %d included cell masses (per temperature %s): %.3f ... %.3f" %
          (rms.size, included.reshape(targets.size, -1).sum(axis=1), rms.min(), rms.max()))
    assert np.all(np.isfinite(rms)) and np.all((rms >= lo) & (rms <= hi))
