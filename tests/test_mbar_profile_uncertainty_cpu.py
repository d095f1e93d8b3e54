"""Error bars of reweighted histograms and free-energy profiles without a GPU: the C ABI's new exports, the Python-side
validation, the block assembly of the Gram matrix [ladder | state | one column per slot] from slot Gram sums against the
explicit weight matrix, the host algebra of metropolisengine_amd/statistics.py on the long-double sums, and the calibration of
the error bars against exact bin probabilities -- on the very inputs tests/test_gpu_mbar_profile_uncertainty.py gives the
device."""
import functools
import os
import re

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_observable_uncertainty_reference as oref
import mbar_profile_reference as pref
import mbar_profile_uncertainty_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["me_mbar_histogram_gram", "me_mbar_histogram_gram_samples"]
NEW_KEYS = {"d_mass", "d_below", "d_above", "d_not_a_number", "d_free_energy", "log_mass_cov", "d_free_energy_from_lowest", "lowest",
            "n_samples"}


def test_header_binding_and_build_list_the_new_unit():
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"^\s*int\s+(me_[a-z_]+)\s*\(", text, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _capi.SYMBOLS, name
    # the twins take the arguments of me_mbar_histogram[_samples] with slot_gram, ladder_gram, column_counts before the outputs
    # and n_used behind them
    for old, new in (("me_mbar_histogram", NEW_EXPORTS[0]), ("me_mbar_histogram_samples", NEW_EXPORTS[1])):
        a, b = _capi.SYMBOLS[old][1], _capi.SYMBOLS[new][1]
        assert len(b) == len(a) + 4 and b[:len(a) - 3] == a[:-3] and b[-4:-1] == a[-3:]
    from metropolisengine_amd import build
    assert "me_mbar_hist_cov" in [name for name, _ in build.HOST_UNITS]
    assert os.path.exists(os.path.join(build.CSRC, "me_mbar_hist_cov.hip"))
    assert hasattr(me.MetropolisEngine, "free_energy_profile_uncertainties")


# ---------------------------------------------------------------------------------------------------- validation
def _no_device_engine():
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)      # no device: validation comes first
    eng.num_real_params, eng.num_complex_params, eng.energy_term_names = 2, 1, ["total"]
    return eng


SAMPLES = ([1.0, 2.0], [0, 1], [1.0, 2.0], [0.0, 0.1])


@pytest.mark.parametrize("inefficiency", [0.99, -2.0, np.nan, np.inf, [1.0, 2.0], np.ones((1, 1))])
def test_bad_inefficiency_is_refused_before_the_library(inefficiency):
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile_uncertainties(*SAMPLES, [1.5], [0.5, 0.25], [0.0, 1.0], inefficiency=inefficiency)
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_profile_uncertainties("energy", [0.0, 1.0], [1.0], inefficiency=inefficiency)


@pytest.mark.parametrize("edges", [[0.0, 1.0, 1.0], [0.0, np.nan, 1.0], [1.0], np.arange(258.0)])
def test_bad_edges_are_refused_before_the_library(edges):
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile_uncertainties(*SAMPLES, [1.5], [0.5, 0.25], edges)
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_profile_uncertainties("energy", edges, [1.0])


@pytest.mark.parametrize("temps", [[], [0.0], [np.nan], [[1.0, 2.0]]])
def test_bad_targets_and_values_are_refused_before_the_library(temps):
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile_uncertainties(*SAMPLES, temps, [0.5, 0.25], [0.0, 1.0])
    with pytest.raises(ValueError):
        _no_device_engine().free_energy_profile_uncertainties("energy", [0.0, 1.0], temps)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile_uncertainties(*SAMPLES, [1.5], [0.5, 0.25, 0.1], [0.0, 1.0])


# ------------------------------------------------------------------------------- the block assembly against the explicit W
@functools.lru_cache(maxsize=None)
def _case(k, bins):
    """One target inside the ladder; everything in long double, computed once."""
    temps, energies, rungs = uref.synthetic(k)
    f = uref.solve(energies, rungs, temps)
    targets = uref.targets_for(temps, 1)
    values, edges = ref.synthetic_values(energies, temps, rungs), ref.edges_of(bins)
    h, mass, counts, w, ladder_counts = ref.slot_gram(energies, rungs, temps, f, targets, values, edges)
    ladder = w[:, :k].T @ w[:, :k]
    g, live = ref.block_gram(h[0], mass[0], ladder)
    explicit, live_w = ref.explicit_weight_matrix(w, k, 0, values, edges, mass[0])
    assert np.array_equal(live, live_w)
    return dict(k=k, temps=temps, targets=targets, edges=edges, values=values, h=h, mass=mass, counts=counts, w=w,
                ladder_counts=ladder_counts, ladder=ladder, g=g, live=live, explicit=explicit,
                column_counts=ref.column_counts(ladder_counts, live.size))


@pytest.mark.parametrize("k,bins", ref.ASSEMBLY_CASES)
def test_block_assembled_gram_and_theta_against_the_explicit_weight_matrix(k, bins):
    """(a) G assembled from the slot sums IS W^T W of the explicit matrix: both long double, so they agree to N 2^-63 of an
    entry (an entry between two different slot columns is exactly 0 on both sides).  (b) Theta from the assembled G (Gram
    route) against Theta by the SVD route of the explicit W, within ref.route_bound of max |Theta|."""
    case = _case(k, bins)
    g, explicit = case["g"], case["explicit"]
    want = ref.gram(explicit)
    assert g.shape == want.shape and int((case["mass"][0] == 0).sum()) == case["mass"].shape[1] - case["live"].size
    if bins == "fine":
        assert (case["counts"][:256] == 0).sum() >= 8           # empty bins are part of this case
    nz = want != 0
    assert np.all(g[~nz] == 0)
    rel = float((np.abs(g - want)[nz] / want[nz]).max())
    theta_a = ref.theta_gram(g, case["column_counts"])
    theta_b = ref.theta_svd(explicit, case["column_counts"])
    bound = ref.route_bound(explicit, case["column_counts"])
    err = np.abs(theta_a - theta_b).max() / np.abs(theta_b).max()
    print("K = %d, %s bins (%d live slots): G assembled against W^T W %.3e; Theta %.3e of max |Theta| (route bound %.3e)"
          % (k, bins, case["live"].size, rel, err, bound))
    assert rel <= uref.N_GRAM * 2.0 ** -63
    assert err <= bound


def test_joint_matrix_against_the_single_bin_matrix():
    """Var ln p_s of a bin from the joint matrix over all slots against the (K + 2)-column matrix [ladder | state | that bin]:
    two float64 routes to four entries of Theta, so within 4 (b_joint + b_single) max |Theta| (ref.log_covariance)."""
    case = _case(8, "uneven")
    k, w, live = 8, case["w"], case["live"]
    theta = ref.theta_gram(case["g"], case["column_counts"])
    cov, scale = ref.log_covariance(theta, k)
    b_joint = ref.route_bound(case["explicit"], case["column_counts"])
    worst = 0.0
    for i, s in enumerate(live):
        single = np.stack([w[:, j] for j in range(k)] + [case["explicit"][:, k], case["explicit"][:, k + 1 + i]], axis=1)
        counts = ref.column_counts(case["ladder_counts"], 1)
        th = ref.theta_svd(single, counts)
        var = th[k + 1, k + 1] + th[k, k] - 2.0 * th[k + 1, k]
        b = b_joint + ref.route_bound(single, counts)
        err = abs(var - cov[i, i]) / max(scale, np.abs(th).max())
        worst = max(worst, err / (4.0 * b))
        assert err <= 4.0 * b, s
    print("joint against single-bin Var ln p: worst error / bound %.3e" % worst)


# ------------------------------------------------------------------------------- the host algebra of statistics.py
@pytest.mark.parametrize("k,bins", ref.ASSEMBLY_CASES)
def test_host_algebra_against_the_reference(k, bins):
    """statistics._profile_uncertainty_result (the reduced algebra: one K x K pseudo-inverse, the largest at K = 64) on the
    long-double sums (rounded to float64) against ref.derived on the SVD route of the explicit (K + 1 + live)-column weight
    matrix: variances within 4 b max |Theta|, b = ref.route_bound; the conventions for empty slots; inefficiency = 4 doubles
    every d_* exactly; the keys of free_energy_profile come through unchanged."""
    case = _case(k, bins)
    edges, targets = case["edges"], case["targets"]
    b = edges.size - 1
    f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
    args = (targets, edges, f64(case["mass"]), case["counts"], np.ones(1), f64(case["h"]), f64(case["ladder"]),
            f64(case["ladder_counts"]), uref.N_GRAM)
    out = statistics._profile_uncertainty_result(*args, 1.0)
    four = statistics._profile_uncertainty_result(*args, 4.0)
    plain = statistics._profile_result(targets, edges, f64(case["mass"]), case["counts"], np.ones(1))
    assert set(out) == set(plain) | NEW_KEYS and out["n_samples"] == uref.N_GRAM
    for key in plain:
        assert np.array_equal(out[key], plain[key]), key
    for key in ("d_mass", "d_below", "d_above", "d_not_a_number", "d_free_energy", "d_free_energy_from_lowest"):
        assert np.array_equal(four[key], 2.0 * out[key], equal_nan=True), key
    assert np.array_equal(four["log_mass_cov"], 4.0 * out["log_mass_cov"], equal_nan=True)
    theta = ref.theta_svd(case["explicit"], case["column_counts"])
    want = ref.derived(theta, k, case["live"], case["mass"][0], targets[0], edges)
    bound = 4.0 * ref.route_bound(case["explicit"], case["column_counts"]) * np.abs(theta).max()
    p = f64(case["mass"][0])
    got_slots = np.concatenate([out["d_mass"][0], [out["d_below"][0], out["d_above"][0], out["d_not_a_number"][0]]])
    live = p > 0
    empty_bins = ~live[:b]
    assert np.all(got_slots[~live] == 0) and np.all(np.isnan(out["d_free_energy"][0][empty_bins]))
    assert np.all(np.isnan(out["d_free_energy_from_lowest"][0][empty_bins]))
    assert np.array_equal(np.isnan(out["log_mass_cov"][0]), empty_bins[:, None] | empty_bins[None, :])
    assert out["lowest"][0] == want["lowest"] and out["d_free_energy_from_lowest"][0][want["lowest"]] == 0.0
    err_slots = np.abs((got_slots[live] / p[live]) ** 2 - (want["d_slots"][live] / p[live]) ** 2).max()
    err_cov = np.nanmax(np.abs(out["log_mass_cov"][0] - want["log_mass_cov"]))
    t = targets[0]
    err_low = np.nanmax(np.abs((out["d_free_energy_from_lowest"][0] / t) ** 2 - (want["d_free_energy_from_lowest"] / t) ** 2))
    print("K = %d, %s bins: Var ln p %.3e, Cov %.3e, Var(ln p - ln p*) %.3e (bound %.3e)" % (k, bins, err_slots, err_cov, err_low, bound))
    assert max(err_slots, err_cov, err_low) <= bound
    # d_free_energy = T sqrt(Var ln p) and d_mass = p sqrt(Var ln p): the same root, two roundings apart
    assert np.allclose(out["d_free_energy"][0][~empty_bins], t * out["d_mass"][0][~empty_bins] / p[:b][~empty_bins], rtol=4 * 2.0 ** -52,
                       atol=0)


def _scaled_slots(factors):
    """A consistent input of _profile_uncertainty_result in float64: K = 3, 4 bins on [-1, 1] of synthetic_values, one target,
    with the state weights of the samples of bin ``s`` multiplied by ``factors[s]`` before the sums are taken (in long double,
    whose range holds them; the rounding to float64 is the device's underflow)."""
    k = 3
    temps, energies, rungs = uref.synthetic(k, n=2053)
    f = uref.solve(energies, rungs, temps)
    targets = uref.targets_for(temps, 1)
    edges = np.linspace(-1.0, 1.0, 5)
    w, counts, _, _, _ = uref.weight_matrix(energies, rungs, temps, f, targets)
    slot = pref.slots(ref.synthetic_values(energies, temps, rungs), edges)
    state = w[:, k].copy()
    for s, factor in factors.items():
        state[slot == s] *= ref.LD(factor)
    h, mass = np.zeros((1, k + 1, 7), dtype=ref.LD), np.zeros((1, 7), dtype=ref.LD)
    for s in np.unique(slot):
        rows = slot == s
        h[0, :k, s] = (w[rows, :k] * state[rows, None]).sum(axis=0)
        h[0, k, s] = (state[rows] ** 2).sum()
        mass[0, s] = state[rows].sum() / state.sum()
    f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
    return (targets, edges, f64(mass), np.bincount(slot, minlength=7).astype(np.int64), np.ones(1), f64(h),
            f64(w[:, :k].T @ w[:, :k]), f64(counts[:k]), 2053)


def test_masses_whose_squared_weights_underflow_lose_their_error_bars_and_nothing_else():
    """A cold target and a bin that only the hot rungs populate: masses of 1e-170 and 1e-300 are ordinary floats and
    free_energy is finite there, but the sums of the squared weights, H[K][s], are 0.  Such a slot is left out (d_mass,
    d_free_energy and its row and column of log_mass_cov are NaN); every other entry is what the same input gives with the two
    bins emptied, bit for bit, because the algebra never sees them.  A mass of 1e-100 (H[K] = 1e-200) keeps its error bar."""
    args = _scaled_slots({0: 1e-170, 3: 1e-300, 2: 1e-100})
    mass, counts, h = args[2], args[3], args[5]
    assert 0 < mass[0, 3] < 1e-290 and 0 < mass[0, 0] < 1e-160 and np.all(h[0, 3, [0, 3]] == 0) and np.all(counts[:4] > 0)
    assert 0 < h[0, 3, 2] < 1e-190
    out = statistics._profile_uncertainty_result(*args, 1.0)
    gone = np.array([True, False, False, True])
    assert np.all(np.isfinite(out["free_energy"])) and np.all(np.isnan(out["d_mass"][0][gone]))
    assert np.all(np.isnan(out["d_free_energy"][0][gone])) and np.all(np.isnan(out["d_free_energy_from_lowest"][0][gone]))
    assert np.array_equal(np.isnan(out["log_mass_cov"][0]), gone[:, None] | gone[None, :])
    kept = ~gone
    assert np.all(np.isfinite(out["d_mass"][0][kept])) and np.all(out["d_mass"][0][kept] > 0)
    assert np.all(np.isfinite(out["d_free_energy"][0][kept])) and np.isfinite(out["d_below"][0]) and np.isfinite(out["d_above"][0])
    emptied_mass, emptied_h = mass.copy(), h.copy()
    emptied_mass[0, [0, 3]] = 0.0
    emptied_h[0, :, [0, 3]] = 0.0
    want = statistics._profile_uncertainty_result(args[0], args[1], emptied_mass, counts, args[4], emptied_h, *args[6:], 1.0)
    for key in ("d_mass", "d_free_energy", "d_free_energy_from_lowest"):
        assert np.array_equal(out[key][0][kept], want[key][0][kept]), key
        assert np.all(want["d_mass"][0][gone] == 0)
    for key in ("d_below", "d_above", "d_not_a_number", "lowest"):
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(out["log_mass_cov"][0][np.ix_(kept, kept)], want["log_mass_cov"][0][np.ix_(kept, kept)])


def test_an_unresolved_lowest_bin_leaves_the_differences_from_it_undefined():
    """The bin of largest density with a mass but no sum of squared weights (it cannot happen to a bin that dominates, so it is
    forced here): there is nothing to take F_b - F_lowest from, and d_free_energy_from_lowest is NaN for that temperature, as on
    a surface, instead of silently referring to a neighbouring bin.  lowest still names the bin; every other key is what the
    same input gives with the bin emptied, bit for bit, as for any unresolved bin."""
    args = _scaled_slots({})
    mass, h = args[2], args[5].copy()
    low = int(np.argmax(mass[0, :4] / np.diff(args[1])))
    h[0, :3, low], h[0, 3, low] = 1e-175, 0.0
    out = statistics._profile_uncertainty_result(*args[:5], h, *args[6:], 1.0)
    assert out["lowest"][0] == low and np.all(np.isnan(out["d_free_energy_from_lowest"][0]))
    assert np.isnan(out["d_mass"][0][low]) and np.isnan(out["d_free_energy"][0][low]) and np.isfinite(out["free_energy"][0][low])
    emptied_mass, emptied_h = mass.copy(), h.copy()
    emptied_mass[0, low] = 0.0
    emptied_h[0, :, low] = 0.0
    want = statistics._profile_uncertainty_result(args[0], args[1], emptied_mass, args[3], args[4], emptied_h, *args[6:], 1.0)
    kept = np.arange(4) != low
    assert want["lowest"][0] != low and np.all(np.isfinite(want["d_free_energy_from_lowest"][0][kept]))
    for key in ("d_mass", "d_free_energy"):
        assert np.all(np.isfinite(out[key][0][kept])) and np.array_equal(out[key][0][kept], want[key][0][kept]), key
    for key in ("d_below", "d_above", "d_not_a_number"):
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(np.isnan(out["log_mass_cov"][0]), ~kept[:, None] | ~kept[None, :])
    assert np.array_equal(out["log_mass_cov"][0][np.ix_(kept, kept)], want["log_mass_cov"][0][np.ix_(kept, kept)])


@pytest.mark.parametrize("k,bins", [(8, "uneven"), (8, "fine")])
def test_a_profile_is_the_surface_of_a_single_y_bin(k, bins):
    """The B + 3 slots of a profile embedded in the (B + 3) x 4 cells of a grid whose one y bin encloses every value: the same
    slot sums and masses at cell (slot_x, 0), zeros elsewhere.  statistics._surface_uncertainty_result on them against
    statistics._profile_uncertainty_result: the NaN and zero patterns and lowest exactly; Var ln p, Cov(ln p, ln p') and
    Var(ln p - ln p_lowest) within 4 b max |Theta|, b = ref.route_bound of the explicit 1-D weight matrix (the bound of
    test_a_single_y_bin_is_the_one_dimensional_unit_bit_for_bit on the device).  Both are layers over one algebra and differ in
    the order of their sums over the slots alone: the difference printed is a few units in the last place."""
    case = _case(k, bins)
    edges, targets = case["edges"], case["targets"]
    b = edges.size - 1
    f64 = lambda a: np.asarray(a, dtype=np.float64)     # noqa: E731
    mass, h = f64(case["mass"]), f64(case["h"])
    mass2, counts2, h2 = np.zeros((1, b + 3, 4)), np.zeros((b + 3, 4), dtype=np.int64), np.zeros((1, k + 1, b + 3, 4))
    mass2[:, :, 0], counts2[:, 0], h2[:, :, :, 0] = mass, case["counts"], h
    tail = (f64(case["ladder"]), f64(case["ladder_counts"]), uref.N_GRAM, 1.0)
    one = statistics._profile_uncertainty_result(targets, edges, mass, case["counts"], np.ones(1), h, *tail)
    two = statistics._surface_uncertainty_result(targets, edges, np.array([-100.0, 100.0]), mass2, counts2, np.ones(1),
                                                 h2.reshape(1, k + 1, -1), *tail, True)
    bound = 4.0 * ref.route_bound(case["explicit"], case["column_counts"]) * np.abs(ref.theta_svd(case["explicit"], case["column_counts"])).max()
    assert np.array_equal(two["lowest"][:, 0], one["lowest"]) and np.all(two["lowest"][:, 1] == 0)
    assert np.array_equal(two["d_mass_slots"][:, :, 0] == 0, mass == 0) and np.all(two["d_mass_slots"][:, :, 1:] == 0)
    assert np.array_equal(one["d_mass"] == 0, mass[:, :b] == 0)
    t, p = targets[0], mass[0, :b]
    worst = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        pairs = [((two["d_mass"][0, :, 0] / p) ** 2, (one["d_mass"][0] / p) ** 2),
                 ((two["d_free_energy"][0, :, 0] / t) ** 2, (one["d_free_energy"][0] / t) ** 2),
                 ((two["d_free_energy_from_lowest"][0, :, 0] / t) ** 2, (one["d_free_energy_from_lowest"][0] / t) ** 2),
                 (two["log_mass_cov"][0], one["log_mass_cov"][0])]
    outer, live = np.array([one["d_below"][0], one["d_above"][0], one["d_not_a_number"][0]]), mass[0, b:] > 0
    assert np.array_equal(outer == 0, ~live) and live.any()
    pairs.append(((two["d_mass_slots"][0, b:, 0][live] / mass[0, b:][live]) ** 2, (outer[live] / mass[0, b:][live]) ** 2))
    for got, want in pairs:
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0, want == 0)
        worst = max(worst, float(np.nanmax(np.abs(got - want))))
    print("K = %d, %s bins: profile against the embedded surface, largest difference of a variance %.3e (bound %.3e, max |Var ln p| %.3e)"
          % (k, bins, worst, bound, np.nanmax(np.abs(one["log_mass_cov"][0]))))
    assert worst <= bound


def test_indicator_columns_through_the_observable_route_give_the_same_errors():
    """The cross-check the GPU test runs against mbar_observable_uncertainties, here between the two references: the 12
    indicator columns as observables (tests/mbar_observable_uncertainty_reference.py: W_na (A - S) / (mean - S) with S = -1)
    against the slot route.  Cov of the masses = p_b p_b' Cov(ln p_b, ln p_b').  Tolerance: the two routes' route_bounds added,
    under the 4 b scale rule.  The scale is that of the observable route, max |Theta| (p_b + 1)(p_b' + 1): its columns are
    normalised by mean - S = p + 1, so that is the size of the terms its covariance is a difference of, and of its rounding.
    It is up to 1 / p^2 looser than max |Theta| p_b p_b' for a small bin; d_mass itself is compared relatively below, under a
    bound that follows from the same figures."""
    case = _case(8, "uneven")
    k, edges, p = 8, case["edges"], np.asarray(case["mass"][0], dtype=np.float64)
    temps, energies, rungs = uref.synthetic(k)
    f = uref.solve(energies, rungs, temps)
    slot = pref.slots(case["values"], edges)
    indicators = np.stack([(slot == s).astype(np.float64) for s in range(12)])
    w_obs, counts_obs, _, mean, shifts = oref.weight_matrix_observables(energies, rungs, temps, f, case["targets"], indicators)
    theta_obs = oref.theta_svd(w_obs, counts_obs)
    cov_obs, _ = oref.covariances(theta_obs, k, 1, 12, mean, shifts)
    theta = ref.theta_gram(case["g"], case["column_counts"])
    log_cov, top = ref.log_covariance(theta, k)
    assert np.array_equal(case["live"][:12], np.arange(12))
    cov_slots = p[:12, None] * p[None, :12] * log_cov[:12, :12]
    bound = ref.route_bound(w_obs, counts_obs) + ref.route_bound(case["explicit"], case["column_counts"])
    # the observable columns are normalised by mean + 1, the slot columns by mean: the same covariance, other Theta entries
    scale = max(top, np.abs(theta_obs).max()) * (p[:12, None] + 1.0) * (p[None, :12] + 1.0)
    err = (np.abs(cov_obs[0] - cov_slots) / scale).max()
    rel = (np.abs(np.sqrt(np.diag(cov_obs[0])) - np.sqrt(np.diag(cov_slots))) / np.sqrt(np.diag(cov_slots))).max()
    # d_mass = sqrt(cov_bb): an error e of the variance moves it by e / (2 d_mass^2) relative
    rel_bound = (4.0 * bound * np.diag(scale) / (2.0 * np.diag(cov_slots))).max()
    print("indicator observables against the slot route: %.3e of the scale (bound %.3e); d_mass relative %.3e (bound %.3e)"
          % (err, 4 * bound, rel, rel_bound))
    assert err <= 4.0 * bound and rel <= rel_bound


# ------------------------------------------------------------------------------------------------------- calibration
def test_reference_error_bars_are_calibrated():
    """64 independent subsets of 8 x 512 exact samples of E = |x|^2 on LADDER8, x_0 in PROFILE_EDGES at PHYSICS_TARGETS: the
    RMS over the subsets of (mass - exact) / d_mass of each of the 3 x 14 masses (12 bins, below, above) lies inside the
    project's CAL_RMS_Z, about +-3 standard errors of the RMS of 64 unit normals."""
    edges, targets, k = pref.PROFILE_EDGES, oref.PHYSICS_TARGETS, 8
    z = []
    for e, rungs, cols in oref.calibration_subsets():
        f = uref.solve(e, rungs, oref.LADDER8)
        h, mass, _, w, ladder_counts = ref.slot_gram(e, rungs, oref.LADDER8, f, targets, cols[0], edges)
        ladder = w[:, :k].T @ w[:, :k]
        rows = []
        for t in range(targets.size):
            g, live = ref.block_gram(h[t], mass[t], ladder)
            theta = ref.theta_gram(g, ref.column_counts(ladder_counts, live.size))
            d = ref.derived(theta, k, live, mass[t], targets[t], edges)["d_slots"][:14]
            rows.append((np.asarray(mass[t][:14], dtype=np.float64) - pref.exact_x0_masses(edges, targets[t])) / d)
        z.append(rows)
    rms = np.sqrt((np.array(z) ** 2).mean(axis=0))
    lo, hi = uref.CAL_RMS_Z
    print("rms z of the 3 x 14 masses: %.3f ... %.3f\n%s" % (rms.min(), rms.max(), rms))
    assert rms.shape == (3, 14) and np.all((rms >= lo) & (rms <= hi))
