"""Error bars of reweighted histograms and free-energy profiles on the GPU (csrc/me_mbar_hist_cov.hip: the slot Gram sums;
metropolisengine_amd/statistics.py: the algebra) against the long-double restatement in
tests/mbar_profile_uncertainty_reference.py, against identities that need no reference, against the existing observable route
and against exact bin probabilities.  Every figure is printed before it is asserted (run with -s);
profiles/mbar_profile_uncertainty.txt holds the values measured on the MI355X."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_observable_uncertainty_reference as oref
import mbar_profile_reference as pref
import mbar_profile_uncertainty_reference as ref
from test_gpu_mbar_profile import ENERGY_EDGES, F_BOUND, UNEVEN12, _store_problem, _targets
from test_gpu_mbar_uncertainty import TERM_ROUNDING, _gram_samples

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, IP, LP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
N = uref.N_GRAM                 # three tiles and a ragged fourth
LARGE = 2048 * 2048 + 5         # more tiles than blocks: a block walks several tiles
# (K, bins, targets).  K + 1 = 9, 34, 65 rows are no multiple of any R the kernel uses; 12 and 64 bins run R = 16, 100 bins
# R = 8, 256 bins R = 4 (csrc/me_mbar_hist_cov.hip, rows_per_pass); 5 targets: more than one pass per row chunk
CASES = [(8, "uneven", 1), (8, "fine", 5), (33, "uneven", 5), (64, "even64", 1), (8, "even100", 1), (33, "fine", 1)]
NEW_KEYS = {"d_mass", "d_below", "d_above", "d_not_a_number", "d_free_energy", "log_mass_cov", "d_free_energy_from_lowest", "lowest",
            "n_samples"}
# A term of H is a product of two exponentials: 3 * 2^-53 each (exp_nonpos, tests/test_gpu_mbar_uncertainty.py) and the
# product, so TERM_ROUNDING (which also pays for a division that is not there) covers it.
GRAM_BOUND = (N + TERM_ROUNDING) * 2.0 ** -53


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


def _hist_gram(energies, rungs, temps, f, targets, values, edges):
    """me_mbar_histogram_gram_samples: (slot_gram, ladder_gram, column_counts, mass, counts, neff_fraction, n_used)."""
    e = np.ascontiguousarray(energies, dtype=np.float64).ravel()
    r = np.ascontiguousarray(rungs, dtype=np.int32).ravel()
    t = np.ascontiguousarray(temps, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    a = np.ascontiguousarray(values, dtype=np.float64).ravel()
    ed = np.ascontiguousarray(edges, dtype=np.float64)
    k, b = t.size, ed.size - 1
    h, ladder, cc = np.zeros((tg.size, k + 1, b + 3)), np.zeros((k, k)), np.zeros(k)
    mass, counts, neff = np.zeros((tg.size, b + 3)), np.zeros(b + 3, dtype=np.int64), np.zeros(tg.size)
    n_used = ctypes.c_int64()
    _capi.check(_capi.load().me_mbar_histogram_gram_samples(
        0, e.ctypes.data_as(DP), r.ctypes.data_as(IP), e.size, t.ctypes.data_as(DP), k, f.ctypes.data_as(DP), tg.ctypes.data_as(DP),
        tg.size, a.ctypes.data_as(DP), ed.ctypes.data_as(DP), b, h.ctypes.data_as(DP), ladder.ctypes.data_as(DP), cc.ctypes.data_as(DP),
        mass.ctypes.data_as(DP), counts.ctypes.data_as(LP), neff.ctypes.data_as(DP), ctypes.byref(n_used)))
    return h, ladder, cc, mass, counts, neff, n_used.value


@functools.lru_cache(maxsize=None)
def _inputs(k):
    temps, energies, rungs = uref.synthetic(k)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-13)["f"]
    return temps, energies, rungs, f, ref.synthetic_values(energies, temps, rungs)


@functools.lru_cache(maxsize=None)
def _case(k, bins, n_targets):
    """Inputs, the device's sums and the long-double reference of one case, computed once and left unchanged."""
    temps, energies, rungs, f, values = _inputs(k)
    edges, targets = ref.edges_of(bins), uref.targets_for(temps, n_targets)
    dev = _hist_gram(energies, rungs, temps, f, targets, values, edges)
    h, mass, counts, w, ladder_counts = ref.slot_gram(energies, rungs, temps, f, targets, values, edges)
    return dict(k=k, temps=temps, energies=energies, rungs=rungs, f=f, values=values, edges=edges, targets=targets, dev=dev, h=h,
                mass=mass, counts=counts, w=w, ladder_counts=ladder_counts)


def _h_error(h_dev, h_ref):
    """Largest |H_dev - H_ref| / H_ref over the entries with H_ref != 0; the others must be exactly 0."""
    seen = h_ref != 0
    assert np.all(h_dev[~seen] == 0.0)
    return float((np.abs(h_dev.astype(ref.LD) - h_ref)[seen] / h_ref[seen]).max())


# ---------------------------------------------------------------------------------------- 1. H against the long-double H
@pytest.mark.parametrize("k,bins,n_targets", CASES)
def test_slot_gram_against_the_long_double_reference(k, bins, n_targets):
    """Entrywise |H_dev - H_ref| <= (N + c) 2^-53 H_ref: every term is >= 0, so N 2^-53 covers ANY summation order, c =
    TERM_ROUNDING.  Empty slots exactly 0, counts exact, masses those of mbar_free_energy_profile bit for bit, the ladder block
    that of me_mbar_gram_samples with no targets bit for bit."""
    case = _case(k, bins, n_targets)
    h, ladder, cc, mass, counts, neff, n_used = case["dev"]
    err = _h_error(h, case["h"])
    print("K = %d, %s bins, %d targets: largest relative error of H %.3e (bound %.3e); %d of %d slots filled"
          % (k, bins, n_targets, err, GRAM_BOUND, int((case["counts"] > 0).sum()), case["counts"].size))
    assert n_used == N and np.array_equal(counts, case["counts"]) and counts.dtype == np.int64
    assert np.all(h[:, :, case["counts"] == 0] == 0.0) and np.all(h[:, :, case["counts"] > 0] > 0.0)
    assert np.array_equal(cc, np.asarray(case["ladder_counts"], dtype=np.float64))
    prof = statistics.mbar_free_energy_profile(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"],
                                               case["values"], case["edges"])
    b = case["edges"].size - 1
    whole = np.concatenate([prof["mass"], prof["below"][:, None], prof["above"][:, None], prof["not_a_number"][:, None]], axis=1)
    assert _bitwise(mass, whole) and _bitwise(neff, prof["neff_fraction"])
    assert np.array_equal(counts, np.concatenate([prof["counts"], prof["counts_outside"]])) and mass.shape == (n_targets, b + 3)
    plain = _gram_samples(case["energies"], case["rungs"], case["temps"], case["f"], np.zeros(0))
    assert _bitwise(ladder, plain[0]) and np.array_equal(cc, plain[1])
    assert err <= GRAM_BOUND


# ------------------------------------------------------------------------------ 2. identities that need no reference
def _identities(label, n, k, energies, rungs, temps, f, targets, values, edges):
    """(a) sum_s H[t][j][s] = G[j, K + 2 t] and (b) sum_s H[t][K][s] = G[K + 2 t, K + 2 t] of me_mbar_gram_samples; (c) sum_k N_k
    H[t][k][s] = sum_{n in s} w_nt = mass[t][s] (sum_k N_k W_nk = 1, and the histogram's total is 1).  Each side is a sum of
    at most n non-negative terms: (n + c) 2^-53 of its value, the two sides' bounds added.  c: TERM_ROUNDING per term of H or G;
    the host's sum over the B + 3 slots adds B + 3; in (c) the K products and additions of the left side add 2 K, and a term
    of a mass is one exponential and the division by the total, 4."""
    h, _, cc, mass, _, _, _ = _hist_gram(energies, rungs, temps, f, targets, values, edges)
    gram = _gram_samples(energies, rungs, temps, f, targets)[0]
    n_slots, u = h.shape[2], 2.0 ** -53
    worst = {}
    for t in range(len(targets)):
        a = k + 2 * t
        lhs = h[t].sum(axis=1)
        bound_ab = ((n + TERM_ROUNDING + n_slots) + (n + TERM_ROUNDING)) * u
        err_a = np.abs(lhs[:k] - gram[:k, a]) / gram[:k, a]
        err_b = abs(lhs[k] - gram[a, a]) / gram[a, a]
        weighted = cc @ h[t, :k]
        bound_c = ((n + TERM_ROUNDING + 2 * k) + (n + 4)) * u
        seen = mass[t] != 0
        assert np.all(weighted[~seen] == 0.0)
        err_c = np.abs(weighted[seen] - mass[t][seen]) / mass[t][seen]
        for name, err, bound in (("a", err_a.max(), bound_ab), ("b", err_b, bound_ab), ("c", err_c.max(), bound_c)):
            worst[name] = max(worst.get(name, 0.0), float(err) / bound)
    print("%s: largest error / bound of (a) ladder x state %.3e, (b) state x state %.3e, (c) sum_k N_k H against the mass %.3e"
          % (label, worst["a"], worst["b"], worst["c"]))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("k,bins,n_targets", [(8, "uneven", 1), (33, "uneven", 5), (8, "fine", 5)])
def test_identities_with_the_gram_matrix_and_the_masses(k, bins, n_targets):
    case = _case(k, bins, n_targets)
    _identities("K = %d, %s bins, %d targets" % (k, bins, n_targets), N, k, case["energies"], case["rungs"], case["temps"],
                case["f"], case["targets"], case["values"], case["edges"])


def test_identities_where_a_block_walks_several_tiles():
    """2048 * 2048 + 5 samples: 2049 tiles on 2048 blocks."""
    temps, energies, rungs = uref.synthetic(8, n=LARGE)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-8)["f"]
    values = ref.synthetic_values(energies, temps, rungs)
    _identities("n = %d, K = 8, 12 bins, 1 target" % LARGE, LARGE, 8, energies, rungs, temps, f, uref.targets_for(temps, 1), values,
                ref.uneven_edges())


# ------------------------------------------------------------------------------------------- 3. the derived quantities
@pytest.mark.parametrize("k,bins,n_targets", [(8, "uneven", 1), (8, "fine", 5), (33, "uneven", 5)])
def test_uncertainties_against_the_reference(k, bins, n_targets):
    """mbar_free_energy_profile_uncertainties (the device's H, the library's algebra) against ref.derived on the SVD route of the
    explicit long-double weight matrix.  Variances are compared: each is a sum of four entries of Theta, so two Thetas that
    differ by b max |Theta| give variances within 4 b max |Theta|; b = ref.route_bound (two float64 routes) + GRAM_BOUND (the
    device's H against the long-double H), capped at the project's F_BOUND."""
    case = _case(k, bins, n_targets)
    edges, targets = case["edges"], case["targets"]
    b = edges.size - 1
    out = statistics.mbar_free_energy_profile_uncertainties(case["energies"], case["rungs"], case["temps"], case["f"], targets,
                                                            case["values"], edges)
    prof = statistics.mbar_free_energy_profile(case["energies"], case["rungs"], case["temps"], case["f"], targets, case["values"], edges)
    assert set(out) == set(prof) | NEW_KEYS and out["n_samples"] == N
    for key in prof:
        assert _bitwise(out[key], prof[key]) if out[key].dtype == np.float64 else np.array_equal(out[key], prof[key]), key
    assert out["d_mass"].shape == out["d_free_energy"].shape == out["d_free_energy_from_lowest"].shape == (n_targets, b)
    assert out["log_mass_cov"].shape == (n_targets, b, b) and out["lowest"].shape == (n_targets,)
    used = case["values"]
    worst = 0.0
    for t in range(n_targets):
        explicit, live = ref.explicit_weight_matrix(case["w"], k, t, used, edges, case["mass"][t])
        cc = ref.column_counts(case["ladder_counts"], live.size)
        theta = ref.theta_svd(explicit, cc)
        want = ref.derived(theta, k, live, case["mass"][t], targets[t], edges)
        bound = min(4.0 * (ref.route_bound(explicit, cc) + GRAM_BOUND), F_BOUND) * np.abs(theta).max()
        p = np.asarray(case["mass"][t], dtype=np.float64)
        got = np.concatenate([out["d_mass"][t], [out["d_below"][t], out["d_above"][t], out["d_not_a_number"][t]]])
        full = p > 0
        empty_bins = ~full[:b]
        assert np.all(got[~full] == 0.0) and np.all(np.isnan(out["d_free_energy"][t][empty_bins]))
        assert np.all(np.isfinite(out["d_free_energy"][t][~empty_bins])) and np.all(np.isnan(out["d_free_energy_from_lowest"][t][empty_bins]))
        assert np.array_equal(np.isnan(out["log_mass_cov"][t]), empty_bins[:, None] | empty_bins[None, :])
        assert out["lowest"][t] == want["lowest"] and out["d_free_energy_from_lowest"][t][want["lowest"]] == 0.0
        tt = targets[t]
        err = max(np.abs((got[full] / p[full]) ** 2 - (want["d_slots"][full] / p[full]) ** 2).max(),
                  np.nanmax(np.abs(out["log_mass_cov"][t] - want["log_mass_cov"])),
                  np.nanmax(np.abs((out["d_free_energy"][t] / tt) ** 2 - (want["d_free_energy"] / tt) ** 2)),
                  np.nanmax(np.abs((out["d_free_energy_from_lowest"][t] / tt) ** 2 - (want["d_free_energy_from_lowest"] / tt) ** 2)))
        print("K = %d, %s bins, target %d: largest error of a variance %.3e (bound %.3e); largest d ln p %.3e"
              % (k, bins, t, err, bound, np.nanmax(got[full] / p[full])))
        worst = max(worst, err / bound)
        assert err <= bound
    print("    worst error / bound %.3e" % worst)


# ----------------------------------------------------------------------------------- 4. against the existing public route
def test_indicator_observables_give_the_same_error_bars():
    """The 12 bin indicators as observable columns through mbar_observable_uncertainties (the matrix cores) against the slot
    route: d_mean = d_mass and mean_cov = p_b p_b' log_mass_cov.  Tolerance: the two routes' route_bounds added, under the 4 b
    scale rule; the observable columns are normalised by mean - S = p + 1 (S = -1), so their entries of mean_cov carry (p_b +
    1)(p_b' + 1) max |Theta| (tests/mbar_observable_uncertainty_reference.py, covariances), the scale used here for both.  It
    is up to 1 / p^2 looser than the slot route's own, so d_mass is also held relatively: an error e of a variance moves its
    root by e / (2 d_mass^2)."""
    case = _case(8, "uneven", 1)
    k, edges, t = 8, case["edges"], case["targets"]
    args = (case["energies"], case["rungs"], case["temps"], case["f"], t)
    slot = pref.slots(case["values"], edges)
    indicators = np.stack([(slot == s).astype(np.float64) for s in range(12)])
    obs = statistics.mbar_observable_uncertainties(*args, indicators)
    out = statistics.mbar_free_energy_profile_uncertainties(*args, case["values"], edges)
    p = out["mass"][0]
    w_obs, counts_obs, _, _, _ = oref.weight_matrix_observables(*args, indicators)
    explicit, live = ref.explicit_weight_matrix(case["w"], k, 0, case["values"], edges, case["mass"][0])
    cc = ref.column_counts(case["ladder_counts"], live.size)
    bound = oref.route_bound(w_obs, counts_obs) + ref.route_bound(explicit, cc)
    top = max(np.abs(oref.theta_svd(w_obs, counts_obs)).max(), np.abs(ref.theta_svd(explicit, cc)).max())
    scale = top * (p[:, None] + 1.0) * (p[None, :] + 1.0)
    cov = p[:, None] * p[None, :] * out["log_mass_cov"][0]
    err = (np.abs(obs["mean_cov"][0] - cov) / scale).max()
    err_d = (np.abs(obs["d_mean"][0] ** 2 - out["d_mass"][0] ** 2) / np.diag(scale)).max()
    rel = (np.abs(obs["d_mean"][0] - out["d_mass"][0]) / out["d_mass"][0]).max()
    print("indicator observables against the slot route: mean_cov %.3e, d_mass^2 %.3e of the scale (bound %.3e); d_mass relative %.3e"
          % (err, err_d, 4 * bound, rel))
    assert np.allclose(obs["mean"][0], p, rtol=1e-12, atol=0)
    rel_bound = (4.0 * bound * np.diag(scale) / (2.0 * out["d_mass"][0] ** 2)).max()
    print("    bound of the relative figure %.3e" % rel_bound)
    assert err <= 4.0 * bound and err_d <= 4.0 * bound and rel <= rel_bound


# ------------------------------------------------------------------------------------------- 5. bitwise reproducibility
def test_two_calls_and_one_target_among_five_agree_bit_for_bit():
    case = _case(33, "uneven", 5)
    args = (case["energies"], case["rungs"], case["temps"], case["f"])
    again = _hist_gram(*args, case["targets"], case["values"], case["edges"])
    for a, b in zip(again[:6], case["dev"][:6]):
        assert _bitwise(a, b) if a.dtype == np.float64 else np.array_equal(a, b)
    for t in (0, 3, 4):
        alone = _hist_gram(*args, case["targets"][t:t + 1], case["values"], case["edges"])
        assert _bitwise(alone[0][0], case["dev"][0][t]) and _bitwise(alone[3][0], case["dev"][3][t]), t
        assert _bitwise(alone[1], case["dev"][1])
    fine = _case(8, "fine", 5)
    alone = _hist_gram(fine["energies"], fine["rungs"], fine["temps"], fine["f"], fine["targets"][2:3], fine["values"], fine["edges"])
    assert _bitwise(alone[0][0], fine["dev"][0][2])


def test_engine_form_equals_the_engine_less_form_bit_for_bit():
    """An 8 x 64-chain store with 5 records and 3 columns, column 1, then the energy itself."""
    eng, temps, e, rungs, cols = _store_problem(8, 64, 5, 3, 1)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, 5)
    keys = ("mass", "below", "above", "not_a_number", "density", "free_energy", "neff_fraction", "d_mass", "d_below", "d_above",
            "d_not_a_number", "d_free_energy", "log_mass_cov", "d_free_energy_from_lowest")
    for which, values, edges in ((eng.observable_names()[1], cols[:, 1].ravel(), UNEVEN12), ("energy", e.ravel(), ENERGY_EDGES)):
        got = eng.free_energy_profile_uncertainties(which, edges, targets, f)
        less = statistics.mbar_free_energy_profile_uncertainties(e, rungs, temps, f, targets, values, edges)
        assert got["name"] == which and set(got) == set(less) | {"name"}
        for key in keys:
            assert _bitwise(got[key], less[key]), (which, key)
        for key in ("counts", "counts_outside", "lowest"):
            assert np.array_equal(got[key], less[key]), (which, key)
        assert got["n_samples"] == less["n_samples"] == e.size
        # ... and the raw sums through the C ABI
        column = -1 if which == "energy" else 1
        b = len(edges) - 1
        h = np.zeros((5, 9, b + 3))
        ed = np.ascontiguousarray(edges, dtype=np.float64)
        eng._check(eng._lib.me_mbar_histogram_gram(eng._handle, f.ctypes.data_as(DP), targets.ctypes.data_as(DP), 5, column,
                                                   ed.ctypes.data_as(DP), b, h.ctypes.data_as(DP), None, None, None, None, None, None))
        assert _bitwise(h, _hist_gram(e, rungs, temps, f, targets, values, edges)[0])
        plain = eng.free_energy_profile(which, edges, targets, f)
        for key in plain:
            assert np.array_equal(plain[key], got[key]) if key != "free_energy" else _bitwise(plain[key], got[key]), key


# ------------------------------------------------------------------------------------------------ 6. non-finite energies
def test_non_finite_energies_are_left_out():
    case = _case(8, "uneven", 1)
    rng = np.random.default_rng(3)
    energies, values = case["energies"].copy(), case["values"].copy()
    bad = rng.choice(energies.size, energies.size // 100, replace=False)
    energies[bad] = np.resize([np.inf, -np.inf, np.nan], bad.size)
    keep = np.isfinite(energies)
    values[bad[0]] = np.nan                                    # of an unused sample: never seen
    first_used = int(np.flatnonzero(keep)[17])
    values[first_used] = np.nan                                # of a used sample: the NaN slot
    args = (energies, case["rungs"], case["temps"], case["f"], case["targets"], values, case["edges"])
    h, _, cc, mass, counts, _, n_used = _hist_gram(*args)
    h_ref, _, counts_ref, _, ladder_counts = ref.slot_gram(*args)
    err = _h_error(h, h_ref)
    bound = (int(keep.sum()) + TERM_ROUNDING) * 2.0 ** -53
    print("1 %% non-finite energies: largest relative error of H on the used samples %.3e (bound %.3e)" % (err, bound))
    assert n_used == int(keep.sum()) == counts.sum() and np.array_equal(counts, counts_ref) and counts[-1] == 1
    assert np.array_equal(cc, np.asarray(ladder_counts, dtype=np.float64)) and err <= bound
    out = statistics.mbar_free_energy_profile_uncertainties(*args)
    assert out["n_samples"] == int(keep.sum()) and out["counts_outside"][2] == 1
    print("    not_a_number %.3e +- %.3e" % (out["not_a_number"][0], out["d_not_a_number"][0]))
    assert out["not_a_number"][0] > 0 and np.isfinite(out["d_not_a_number"][0]) and out["d_not_a_number"][0] > 0
    assert np.all(np.isfinite(out["d_mass"])) and np.all(np.isfinite(out["d_free_energy"]))


def test_a_cold_target_whose_far_bins_underflow_keeps_every_other_error_bar():
    """The energy histogram at T = 0.02 under a ladder that starts at 0.5: the weights of the upper bins are below 1e-154, so
    their squared sums (and further up the masses themselves) are 0 although the bins hold samples.  The call succeeds; a slot
    whose H[K] is no normal float64 has d_free_energy NaN and d_mass NaN (mass > 0) or 0 (mass exactly 0); every other slot has
    a finite error bar; and the second target's row is bit for bit what it is alone."""
    case = _case(8, "uneven", 1)
    args = (case["energies"], case["rungs"], case["temps"], case["f"])
    edges = np.linspace(0.0, 80.0, 41)
    targets = np.array([0.02, case["targets"][0]])
    out = statistics.mbar_free_energy_profile_uncertainties(*args, targets, case["energies"], edges)
    h, _, _, mass, counts, _, _ = _hist_gram(*args, targets, case["energies"], edges)
    resolved = h[:, 8, :40] >= np.finfo(np.float64).tiny
    p = mass[:, :40]
    lost = ~resolved[0] & (counts[:40] > 0)
    print("T = 0.02: %d bins hold samples, %d of them without a resolved sum of squares (%d with mass exactly 0); least resolved "
          "mass %.3e" % (int((counts[:40] > 0).sum()), int(lost.sum()), int((lost & (p[0] == 0)).sum()), p[0][resolved[0]].min()))
    assert lost.sum() >= 2 and np.array_equal(resolved[1], counts[:40] > 0)
    # (>= 0, not > 0: the bin that holds all but 1e-26 of the mass has Var ln p = 0 up to the rounding of four entries of Theta)
    assert np.all(np.isfinite(out["d_mass"][resolved])) and np.all(out["d_mass"][resolved] >= 0)
    assert np.all(out["d_mass"][1][resolved[1]] > 0)
    assert np.all(np.isfinite(out["d_free_energy"][resolved])) and np.all(np.isnan(out["d_free_energy"][~resolved]))
    assert np.all(np.isnan(out["d_mass"][~resolved & (p > 0)])) and np.all(out["d_mass"][~resolved & (p == 0)] == 0)
    assert np.array_equal(np.isfinite(out["free_energy"]), p > 0)
    alone = statistics.mbar_free_energy_profile_uncertainties(*args, targets[1:], case["energies"], edges)
    for key in ("mass", "d_mass", "d_free_energy", "log_mass_cov", "d_free_energy_from_lowest", "d_below", "d_above"):
        assert _bitwise(out[key][1], alone[key][0]), key


# ------------------------------------------------------------------------------------------------------- 7. calibration
def test_calibration_on_the_device():
    """The subsets of tests/test_mbar_profile_uncertainty_cpu.py through the GPU; the same condition on the RMS z-scores."""
    edges, targets = pref.PROFILE_EDGES, oref.PHYSICS_TARGETS
    z = []
    for e, rungs, cols in oref.calibration_subsets():
        f = statistics.mbar_free_energies(e, rungs, oref.LADDER8, tol=1e-12)["f"]
        out = statistics.mbar_free_energy_profile_uncertainties(e, rungs, oref.LADDER8, f, targets, cols[0], edges)
        est = np.concatenate([out["mass"], out["below"][:, None], out["above"][:, None]], axis=1)
        d = np.concatenate([out["d_mass"], out["d_below"][:, None], out["d_above"][:, None]], axis=1)
        exact = np.array([pref.exact_x0_masses(edges, t) for t in targets])
        z.append((est - exact) / d)
    rms = np.sqrt((np.array(z) ** 2).mean(axis=0))
    lo, hi = uref.CAL_RMS_Z
    print("rms z of the 3 x 14 masses on the device: %.3f ... %.3f\n%s" % (rms.min(), rms.max(), rms))
    assert rms.shape == (3, 14) and np.all((rms >= lo) & (rms <= hi))


# ------------------------------------------------------------------------------------------------------------ 8. errors
def _ptr(a):
    return _capi.double_ptr(np.ascontiguousarray(a, dtype=np.float64))


def test_error_cases():
    """Those of tests/test_gpu_mbar_profile.py's test_error_cases through the new entry points, and the inefficiency."""
    eng, temps, e, rungs, cols = _store_problem(8, 64, 2, 3, 1)
    f = eng.ladder_free_energies()["f"]
    good = np.array([1.0, 2.0, 3.0])
    values = cols[:, 1].ravel().copy()
    for edges in ([1.0, 2.0, 2.0], [1.0, 3.0, 2.0], [1.0, np.nan, 3.0], [1.0], np.arange(258.0)):
        with pytest.raises(ValueError):
            eng.free_energy_profile_uncertainties("real_1", edges, [1.0], f)
        with pytest.raises(ValueError):
            statistics.mbar_free_energy_profile_uncertainties(e, rungs, temps, f, [1.0], values, edges)
    with pytest.raises(ValueError, match="unknown recorded observable"):
        eng.free_energy_profile_uncertainties("real_3", good, [1.0], f)
    with pytest.raises(ValueError, match="outside the 3 recorded columns"):
        eng.free_energy_profile_uncertainties(3, good, [1.0], f)
    for bad in ([0.0], [1.0, -1.0], [np.nan], []):
        with pytest.raises(ValueError):
            eng.free_energy_profile_uncertainties("real_1", good, bad, f)
    for bad in (0.99, -2.0, np.nan, np.inf, [1.0, 2.0], np.ones(3)):
        with pytest.raises(ValueError):
            eng.free_energy_profile_uncertainties("real_1", good, [1.0], f, inefficiency=bad)
        with pytest.raises(ValueError):
            statistics.mbar_free_energy_profile_uncertainties(e, rungs, temps, f, [1.0], values, good, inefficiency=bad)
    one = eng.free_energy_profile_uncertainties("real_1", UNEVEN12, [0.7, 1.9], f)
    four = eng.free_energy_profile_uncertainties("real_1", UNEVEN12, [0.7, 1.9], f, inefficiency=4.0)
    for key in ("d_mass", "d_below", "d_above", "d_not_a_number", "d_free_energy", "d_free_energy_from_lowest"):
        assert np.array_equal(four[key], 2.0 * one[key], equal_nan=True), key
    assert np.array_equal(four["log_mass_cov"], 4.0 * one["log_mass_cov"], equal_nan=True) and _bitwise(four["mass"], one["mass"])
    # the same through the C ABI
    lib, h = eng._lib, eng._handle
    fp, tp = _ptr(f), _ptr([1.0])
    call = lambda column, edges, n_bins, temps_ptr=tp: lib.me_mbar_histogram_gram(     # noqa: E731
        h, fp, temps_ptr, 1, column, _ptr(edges), n_bins, None, None, None, None, None, None, None)
    assert call(1, good, 2) == _capi.ME_OK                        # every output may be null
    assert call(-1, good, 2) == _capi.ME_OK
    assert call(1, [1.0, 2.0, 2.0], 2) == _capi.ME_ERR_INVALID
    assert call(1, [1.0, 3.0, 2.0], 2) == _capi.ME_ERR_INVALID
    assert call(1, [1.0, np.nan, 3.0], 2) == _capi.ME_ERR_INVALID
    assert call(1, [1.0, np.inf], 1) == _capi.ME_ERR_INVALID
    assert call(1, good, 0) == _capi.ME_ERR_INVALID
    assert call(1, np.arange(258.0), 257) == _capi.ME_ERR_INVALID
    assert call(1, np.arange(257.0), 256) == _capi.ME_OK
    assert call(3, good, 2) == _capi.ME_ERR_INVALID               # column index >= recorded columns
    assert call(-2, good, 2) == _capi.ME_ERR_INVALID
    assert call(1, good, 2, _ptr([0.0])) == _capi.ME_ERR_INVALID  # temperature <= 0
    assert call(1, good, 2, _ptr([-1.0])) == _capi.ME_ERR_INVALID
    r32 = np.ascontiguousarray(rungs, dtype=np.int32)
    less = lambda edges, n_bins: lib.me_mbar_histogram_gram_samples(     # noqa: E731
        0, _ptr(e), _capi.int32_ptr(r32), e.size, _ptr(temps), 8, fp, tp, 1, _capi.double_ptr(values), _ptr(edges), n_bins, None, None,
        None, None, None, None, None)
    assert less(good, 2) == _capi.ME_OK
    assert less([1.0, 1.0, 3.0], 2) == _capi.ME_ERR_INVALID and less(good, 0) == _capi.ME_ERR_INVALID
    assert less(np.arange(258.0), 257) == _capi.ME_ERR_INVALID
    # more than 64 rungs: the Python layer refuses (ValueError), the C ABI as me_mbar_histogram_samples does
    temps65 = np.linspace(0.5, 3.0, 65)
    r65 = (np.arange(e.size) % 65).astype(np.int32)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_profile_uncertainties(e, r65, temps65, np.zeros(65), [1.0], values, good)
    f65 = _ptr(np.zeros(65))
    old = lib.me_mbar_histogram_samples(0, _ptr(e), _capi.int32_ptr(r65), e.size, _ptr(temps65), 65, f65, tp, 1,
                                        _capi.double_ptr(values), _ptr(good), 2, None, None, None)
    new = lib.me_mbar_histogram_gram_samples(0, _ptr(e), _capi.int32_ptr(r65), e.size, _ptr(temps65), 65, f65, tp, 1,
                                             _capi.double_ptr(values), _ptr(good), 2, None, None, None, None, None, None, None)
    assert old == new != _capi.ME_OK
    eng.record_observables(None)                                  # no observable store
    assert call(0, good, 2) == _capi.ME_ERR_STATE
    assert call(-1, good, 2) == _capi.ME_OK                       # ... which the energy does not need
    with pytest.raises(ValueError, match="no observable store"):
        eng.free_energy_profile_uncertainties(0, good, [1.0], f)
    eng.record_energies(0)                                        # no energy store
    assert call(-1, good, 2) == _capi.ME_ERR_STATE
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples"):
        eng.free_energy_profile_uncertainties("energy", good, [1.0], f)
    # a scalar-temp engine without a ladder: as free_energy_profile
    scalar = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=128, temp=1.0)
    scalar.record_energies(2)
    scalar.record_observables(["real_0"])
    scalar.record_energy()
    for which in ("real_0", "energy"):
        with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
            scalar.free_energy_profile_uncertainties(which, good, [1.0], f=[0.0])


# -------------------------------------------------------------------------------------------------------- 9. end to end
def test_double_well_ladder_end_to_end():
    """demo.QUICK (8 rungs x 256 chains, 16 records of the coordinate): an error bar wherever a bin has a sample, and at the
    coldest demo temperature a barrier height that its error bar resolves."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import demo_free_energy_profile as demo
    finally:
        sys.path.pop(0)
    eng = demo.sample(**demo.QUICK)
    f = eng.ladder_free_energies()["f"]
    out = eng.free_energy_profile_uncertainties("real_0", demo.EDGES, demo.TEMPS, f)
    plain = eng.free_energy_profile("real_0", demo.EDGES, demo.TEMPS, f)
    for key in plain:
        assert np.array_equal(plain[key], out[key]), key
    seen = out["counts"] > 0
    assert np.all(np.isfinite(out["d_free_energy"][:, seen])) and np.all(out["d_free_energy"][:, seen] > 0)
    assert np.all(np.isnan(out["d_free_energy"][:, ~seen])) and out["n_samples"] == eng.energy_samples().size
    for i, t in enumerate(demo.TEMPS):
        height, error, top, well = demo.barrier_height(out, i)
        print("T = %.2f: barrier height F(%.2f) - F(%.2f) = %.4f +- %.4f; d_free_energy_from_lowest at the top %.4f"
              % (t, out["centers"][top], out["centers"][well], height, error, out["d_free_energy_from_lowest"][i, top]))
        assert abs(error - out["d_free_energy_from_lowest"][i, top]) <= 1e-12 * max(error, 1.0)
    height, error, _, _ = demo.barrier_height(out, 0)             # the coldest demo temperature
    assert 0.0 < error < height
