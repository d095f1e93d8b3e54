"""Reweighted histograms and free-energy profiles on the GPU (csrc/me_mbar_hist.hip) against the long-double reference of
tests/mbar_profile_reference.py, the validated reweighting kernels and exact results.  Every figure is printed before it is
asserted (run with -s); profiles/mbar_profile.txt holds the values measured on the MI355X.

Sample counts as in test_gpu_mbar_observables.py: the ragged 2048 * 3 + 5 goes through the engine-less form, the engine's
stores take 512 x 33 and 2112 x 6 samples."""
import os
import subprocess
import sys

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref
import mbar_observables_reference as oref
import mbar_profile_reference as pref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_BOUND = 1e-8          # the project's bound for float64 quantities that pass through iterated arithmetic
# Largest relative error of a mass against the long-double reference over tests 1-3 (slots whose reference mass is not zero)
# as measured on the MI355X (profiles/mbar_profile.txt); the tests assert ten times this, capped at 1e-8.
MEASURED_MASS_ERROR = 1.40e-14
BOUND = min(10 * MEASURED_MASS_ERROR, F_BOUND)
RAGGED = 2048 * 3 + 5
LARGE = 2048 * 2048 + 5         # more tiles than blocks: a block walks more than one tile
CORNER = 2048 + 64
UNEVEN12 = 1.0 + np.concatenate([[0.0], np.cumsum([0.3, 0.2, 0.5, 0.1, 0.4, 0.6, 0.25, 0.35, 0.8, 0.15, 0.45, 0.9])])   # 1 ... 6
ENERGY_EDGES = np.linspace(0.0, 40.0, 17)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


def _flat_problem(k, n, seed=17):
    """Engine-less inputs from ref.gamma_ladder (the D = 16 quadratic form on 0.5 ... 0.5 * 1.3^7 in ``k`` rungs): ``n``
    samples, rung i % k; the values are sqrt(E) plus noise from a generator of their own, mostly inside [1, 6]."""
    per_rung = -(-n // k)
    energies, temps = ref.gamma_ladder(per_rung, n_rungs=k, seed=seed, ratio=(1.3 ** 7) ** (1.0 / (k - 1)))
    e = energies.T.ravel()[:n].copy()
    rungs = (np.arange(n) % k).astype(np.int32)
    values = np.sqrt(e) + 0.25 * np.random.default_rng(seed + 100).standard_normal(n)
    return temps, e, rungs, values


def _store_problem(k, m, records, q, column, seed=19):
    """The same as an engine's stores: ``(engine, temps, energies (records, k m), rungs, columns (records, q, k m))``; column
    ``column`` holds the values of _flat_problem's kind, the others noise."""
    energies, temps = ref.gamma_ladder(m * records, n_rungs=k, seed=seed, ratio=(1.3 ** 7) ** (1.0 / (k - 1)))
    e = energies.reshape(k, records, m).transpose(1, 0, 2).reshape(records, k * m).copy()
    rng = np.random.default_rng(seed + 100)
    cols = rng.standard_normal((records, q, k * m))
    cols[:, column] = np.sqrt(e) + 0.25 * cols[:, column]
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, [0.1j] * 4, n_chains=k * m, seed=5, dtype="f64",
                              temperatures=temps)
    eng.record_energies(records)
    eng.record_observables(list(range(q)))
    eng.set_energy_samples(e)
    eng.set_observable_samples(cols)
    return eng, temps, e, np.tile(np.repeat(np.arange(k), m), records).astype(np.int32), cols


def _targets(temps, n):
    """``n`` target temperatures: both ends of the ladder first, then rungs and points between rungs."""
    k = temps.size
    pool = [temps[0], temps[-1], 0.57, temps[k // 2], 0.8, temps[1], 1.5, temps[3 * k // 4], 2.6]
    return np.array([0.9]) if n == 1 else np.array(pool[:n])


def _check(label, out, want, bound=None):
    """``out`` (a result dictionary) against the long-double ``want = (mass, counts, neff)`` of the reference: the counts exactly,
    empty slots exactly 0, the others within the bound.  Returns the largest relative error of a mass (printed)."""
    bound = BOUND if bound is None else bound
    mass, counts, _ = want
    got = np.concatenate([out["mass"], out["below"][:, None], out["above"][:, None], out["not_a_number"][:, None]], axis=1)
    got_counts = np.concatenate([out["counts"], out["counts_outside"]])
    assert got_counts.dtype == np.int64 and np.array_equal(got_counts, counts), label
    assert np.all(got[:, counts == 0] == 0.0), label
    seen = mass != 0
    rel = float(np.max(np.abs(got.astype(np.longdouble)[seen] - mass[seen]) / mass[seen]))
    total = float(np.max(np.abs(got.sum(axis=1) - 1.0)))
    print("%s: largest relative error of a mass against long double %.3e (bound %.1e); |sum - 1| %.2e; slots filled %d of %d"
          % (label, rel, bound, total, int((counts > 0).sum()), counts.size))
    assert rel <= bound, (label, rel, bound)
    assert total <= 1e-13, label
    return rel


# --------------------------------------------------------------------- 1-3. the kernels against the long-double reference


@pytest.mark.parametrize("k, edges, n_targets", [(8, UNEVEN12, 9), (33, np.linspace(0.5, 7.0, 257), 4)])
def test_ragged_tile_matches_the_long_double_reference(k, edges, n_targets):
    temps, e, rungs, values = _flat_problem(k, RAGGED)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, n_targets)
    got = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, values, edges)
    b = len(edges) - 1
    assert got["mass"].shape == (n_targets, b) and got["counts"].shape == (b,) and got["counts_outside"].shape == (3,)
    assert got["below"].shape == got["above"].shape == got["not_a_number"].shape == got["neff_fraction"].shape == (n_targets,)
    assert "name" not in got
    want = pref.histogram(e, rungs, temps, f, targets, values, edges, dtype=np.longdouble)
    _check("engine-less n=%d K=%d bins=%d T=%d" % (RAGGED, k, b, n_targets), got, want)
    assert np.array_equal(got["density"], got["mass"] / np.diff(edges)[None, :])


@pytest.mark.parametrize("k, m, records, q, column", [(8, 64, 33, 16, 5), (33, 64, 6, 1, 0)])
def test_stores_match_the_reference_and_the_engine_less_form_bit_for_bit(k, m, records, q, column):
    eng, temps, e, rungs, cols = _store_problem(k, m, records, q, column)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, 5)
    label = "store %dx%d K=%d Q=%d column %d" % (records, k * m, k, q, column)
    name = eng.observable_names()[column]
    got = eng.free_energy_profile(name, UNEVEN12, targets, f)
    assert got["name"] == name
    flat = cols[:, column].ravel()
    _check(label, got, pref.histogram(e, rungs, temps, f, targets, flat, UNEVEN12, dtype=np.longdouble))
    by_index = eng.free_energy_profile(column, UNEVEN12, targets, f)
    less = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, flat, UNEVEN12)
    for key in ("mass", "below", "above", "not_a_number", "density", "free_energy", "neff_fraction"):
        assert _bitwise(got[key], less[key]) and _bitwise(got[key], by_index[key]), key
    assert np.array_equal(got["counts"], less["counts"]) and np.array_equal(got["counts_outside"], less["counts_outside"])
    # the energy itself, with the observable store and without it
    energy = eng.free_energy_profile("energy", ENERGY_EDGES, targets, f)
    assert energy["name"] == "energy"
    _check(label + ", energy", energy, pref.histogram(e, rungs, temps, f, targets, e, ENERGY_EDGES, dtype=np.longdouble))
    less = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, e, ENERGY_EDGES)
    eng.record_observables(None)                              # frees the observable store; the energy records stay
    alone = eng.free_energy_profile("energy", ENERGY_EDGES, targets, f)
    for key in ("mass", "below", "above", "not_a_number", "neff_fraction"):
        assert _bitwise(energy[key], less[key]) and _bitwise(energy[key], alone[key]), key
    assert np.array_equal(energy["counts"], alone["counts"])
    with pytest.raises(ValueError, match="no observable store"):
        eng.free_energy_profile(0, UNEVEN12, targets, f)


def test_a_block_that_walks_several_tiles_matches_the_long_double_reference():
    """2048 * 2048 + 5 samples: 2049 tiles on 2048 blocks, through the engine-less form."""
    temps, e, rungs, values = _flat_problem(8, LARGE)
    f = statistics.mbar_free_energies(e, rungs, temps, tol=1e-8)["f"]
    edges = np.linspace(1.0, 6.0, 17)
    got = statistics.mbar_free_energy_profile(e, rungs, temps, f, [1.1], values, edges)
    want = pref.histogram(e, rungs, temps, f, [1.1], values, edges, dtype=np.longdouble)
    _check("engine-less n=%d K=8 bins=16 T=1" % LARGE, got, want)


# -------------------------------------------------------------------------------------------------- 4. binning corner cases


def _corner_values(case, rng):
    """``(values, edges)`` of a corner case for CORNER samples."""
    i = np.arange(CORNER)
    if case == "one bin":                       # a wavefront's 64 lanes in one slot: one match round
        return 2.0 + 0.4 * rng.random(CORNER), UNEVEN12 + 0.5
    if case == "64 distinct":                   # consecutive samples cycle through 64 bins: every wavefront sees 64 slots
        edges = np.linspace(0.0, 8.0, 81)
        return 0.05 + 0.1 * ((i * 37) % 64 + 8), edges
    if case == "n_bins = 1":
        return 3.0 * rng.random(CORNER) + 1.0, np.array([1.5, 3.0])
    if case == "on the edges":                  # exactly on the first, an inner and the last edge, and just beside them
        pick = np.array([UNEVEN12[0], UNEVEN12[5], UNEVEN12[-1], np.nextafter(UNEVEN12[0], -np.inf),
                         np.nextafter(UNEVEN12[5], -np.inf), np.nextafter(UNEVEN12[-1], -np.inf), 2.2])
        return pick[(i * 5) % pick.size], UNEVEN12
    assert case == "inf and nan"
    values = 1.0 + 5.0 * rng.random(CORNER)
    values[::7] = np.inf
    values[3::11] = -np.inf
    values[5::13] = np.nan
    values[[0, 63, 64, 2047, 2048, CORNER - 1]] = [np.nan, -np.inf, np.inf, np.nan, np.inf, -np.inf]
    return values, UNEVEN12


@pytest.mark.parametrize("case", ["one bin", "64 distinct", "n_bins = 1", "on the edges", "inf and nan"])
def test_binning_corner_cases(case):
    temps, e, rungs, _ = _flat_problem(8, CORNER, seed=31)
    values, edges = _corner_values(case, np.random.default_rng(41))
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 5)
    got = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, values, edges)
    want = pref.histogram(e, rungs, temps, f, targets, values, edges, dtype=np.longdouble)
    _check(case, got, want)
    filled = int((want[1] > 0).sum())
    if case == "one bin":
        assert filled == 1 and got["counts"].max() == CORNER
    if case == "64 distinct":
        assert filled == 64 and len(set(pref.slots(values[:64], edges))) == 64 and got["counts_outside"].sum() == 0
    if case == "on the edges":
        assert got["counts_outside"].tolist() == [want[1][12], want[1][13], 0] and want[1][12] > 0 and want[1][13] > 0
    if case == "inf and nan":
        assert np.all(got["counts_outside"] > 0) and got["counts_outside"][2] == np.isnan(values).sum()


# ------------------------------------------------------------------------------ 5. temperature chunks and reproducibility


def test_results_do_not_depend_on_the_chunks_and_are_reproducible():
    temps, e, rungs, values = _flat_problem(8, RAGGED, seed=37)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 9)
    whole = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, values, UNEVEN12)
    again = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, values, UNEVEN12)
    keys = ("mass", "below", "above", "not_a_number", "neff_fraction")
    for key in keys:
        assert _bitwise(whole[key], again[key]), key              # two calls
    for t in range(9):
        one = statistics.mbar_free_energy_profile(e, rungs, temps, f, [targets[t]], values, UNEVEN12)
        for key in keys:
            assert _bitwise(one[key][0], whole[key][t]), (key, t)     # alone = among 9
        assert np.array_equal(one["counts"], whole["counts"])


# ------------------------------------------------------------------------------------------ 6. tie to the validated kernels


def test_masses_are_the_reweighted_means_of_the_bins_indicators():
    """mass[t][b] against the reweighted mean of the column 1[A in bin b] of statistics.mbar_reweight_observables.  Two
    assertions, both figures printed.  (a) The difference divided by the mass is held to F_BOUND = 1e-8, the project's cap,
    NOT to the tighter BOUND of the masses: the mean kernel updates mean <- mean + (A - mean) w / W, whose rounding error is
    relative to the size of the column's values (here 1), not to the mean, and its own validated bound
    (test_gpu_mbar_observables.py) is for columns whose mean is of the order of their values.  Here the least mass is
    3.9e-12; the largest difference measured is 5.6e-17, which is 1.5e-10 of its mass (profiles/mbar_profile.txt), while the
    masses themselves are within BOUND of the long-double reference on inputs of this kind (test 7): the relative figure is
    the indicator mean's error.
    (b) The difference itself, |mass - mean|, is held to BOUND: the masses are <= 1, so this is BOUND relative to the size of
    the indicator's values, which is what the mean kernel can keep."""
    temps, e, rungs, values = _flat_problem(8, RAGGED, seed=43)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 5)
    got = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, values, UNEVEN12)
    assert np.all(got["counts"] > 0)
    indicators = np.stack([((values >= UNEVEN12[b]) & (values < UNEVEN12[b + 1])).astype(np.float64) for b in range(12)])
    means = statistics.mbar_reweight_observables(e, rungs, temps, f, targets, indicators)["mean"]
    rel = float(np.max(np.abs(got["mass"] - means) / means))
    diff = float(np.max(np.abs(got["mass"] - means)))
    neff = statistics.mbar_reweight(e, rungs, temps, f, targets)["neff_fraction"]
    rel_neff = float(np.max(np.abs(got["neff_fraction"] - neff) / neff))
    total = got["mass"].sum(axis=1) + got["below"] + got["above"] + got["not_a_number"]
    print("mass against the mean of the bin's indicator: largest difference %.3e (of the mass: %.3e; least mass %.3e); "
          "neff_fraction against mbar_reweight's %.3e; |sum of all slots - 1| %.2e"
          % (diff, rel, got["mass"].min(), rel_neff, np.max(np.abs(total - 1.0))))
    assert rel <= F_BOUND and diff <= BOUND and rel_neff <= BOUND
    assert np.max(np.abs(total - 1.0)) <= 1e-13


# ------------------------------------------------------------------------------------------------- 7. non-finite energies


def test_samples_with_non_finite_energies_are_not_used():
    temps, e, rungs, values = _flat_problem(8, RAGGED, seed=23)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    dirty, dirty_values = e.copy(), values.copy()
    dirty[[3, 64, 2047, 2048, 4100, RAGGED - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    dirty_values[[3, 64, 4100]] = np.nan                      # of unused samples: never seen
    targets = _targets(temps, 4)
    got = statistics.mbar_free_energy_profile(dirty, rungs, temps, f, targets, dirty_values, UNEVEN12)
    want = pref.histogram(dirty, rungs, temps, f, targets, dirty_values, UNEVEN12, dtype=np.longdouble)
    _check("engine-less n=%d K=8, 6 unused samples" % RAGGED, got, want)
    assert got["counts"].sum() + got["counts_outside"].sum() == np.isfinite(dirty).sum() == RAGGED - 6
    assert got["counts_outside"][2] == 0
    dirty[rungs == 5] = np.nan                                # a rung left without a finite sample
    with pytest.raises(_capi.MetropolisLibraryError, match="rung 5 of 8 has no sample with a finite energy"):
        statistics.mbar_free_energy_profile(dirty, rungs, temps, f, targets, dirty_values, UNEVEN12)


# ------------------------------------------------------------------------------------------------------ 8. exact physics


def test_exact_bin_probabilities_of_the_quadratic_energy():
    """Exact samples of E = |x|^2 in 4 real dimensions on LADDER8, 16 independent subsets of 8 x 1024: the masses of x_0 in
    the 12 bins of linspace(-1.5, 1.5, 13), below and above at three temperatures between rungs, 3 x 14 comparisons, each
    within 5 standard errors.  tests/test_mbar_profile_cpu.py shows that the reference meets all of them on these very
    inputs."""
    results = []
    for e, rungs, cols in oref.iso_quadratic_subsets():
        out = statistics.mbar_free_energies(e, rungs, oref.LADDER8)
        assert out["converged"]
        prof = statistics.mbar_free_energy_profile(e, rungs, oref.LADDER8, out["f"], oref.PHYSICS_TARGETS, cols[0],
                                                   pref.PROFILE_EDGES)
        results.append(np.concatenate([prof["mass"], prof["below"][:, None], prof["above"][:, None]], axis=1))
    est, exact = pref.physics_masses(results, oref.PHYSICS_TARGETS)
    ok, m, se = ref.within_5_se(est, exact)
    dev = np.abs(m - exact) / se
    print("deviation / se of the 3 x 14 masses: largest %.2f\n" % dev.max(), dev)
    assert ok.shape == (3, 14) and np.all(ok)
    # the profile as documented: F = -T ln(mass / width), so a difference of F is -T ln of the density ratio
    t = oref.PHYSICS_TARGETS[:, None]
    assert np.all(prof["counts"][3:9] > 100)
    assert np.array_equal(prof["density"], prof["mass"] / prof["widths"][None, :])
    assert np.array_equal(prof["free_energy"], -t * np.log(prof["density"]))
    diff = prof["free_energy"][:, 4] - prof["free_energy"][:, 7]
    want = -oref.PHYSICS_TARGETS * np.log(prof["density"][:, 4] / prof["density"][:, 7])
    assert np.allclose(diff, want, rtol=0, atol=1e-14 * np.max(np.abs(prof["free_energy"][:, 3:9])))


# ------------------------------------------------------------------------------------------------------------- 9. errors


def _ptr(a):
    return _capi.double_ptr(np.ascontiguousarray(a, dtype=np.float64))


def test_error_cases():
    eng, temps, e, rungs, cols = _store_problem(8, 64, 2, 3, 1)
    f = eng.ladder_free_energies()["f"]
    good = np.array([1.0, 2.0, 3.0])
    for edges in ([1.0, 2.0, 2.0], [1.0, 3.0, 2.0], [1.0, np.nan, 3.0], [1.0], np.arange(258.0)):
        with pytest.raises(ValueError):
            eng.free_energy_profile("real_1", edges, [1.0], f)
        with pytest.raises(ValueError):
            statistics.mbar_free_energy_profile(e, rungs, temps, f, [1.0], cols[:, 1].ravel(), edges)
    with pytest.raises(ValueError, match="unknown recorded observable"):
        eng.free_energy_profile("real_3", good, [1.0], f)         # in the catalogue, not recorded
    with pytest.raises(ValueError, match="outside the 3 recorded columns"):
        eng.free_energy_profile(3, good, [1.0], f)
    for bad in ([0.0], [1.0, -1.0], [np.nan], []):
        with pytest.raises(ValueError):
            eng.free_energy_profile("real_1", good, bad, f)
    # the same through the C ABI
    lib, h = eng._lib, eng._handle
    fp, tp = _ptr(f), _ptr([1.0])
    call = lambda column, edges, n_bins, temps_ptr=tp: lib.me_mbar_histogram(h, fp, temps_ptr, 1, column, _ptr(edges), n_bins,     # noqa: E731
                                                                              None, None, None)
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
    r32, values = np.ascontiguousarray(rungs, dtype=np.int32), cols[:, 1].ravel().copy()
    less = lambda edges, n_bins: lib.me_mbar_histogram_samples(0, _ptr(e), _capi.int32_ptr(r32), e.size, _ptr(temps), 8, fp, tp, 1,   # noqa: E731
                                                                _capi.double_ptr(values), _ptr(edges), n_bins, None, None, None)
    assert less(good, 2) == _capi.ME_OK
    assert less([1.0, 1.0, 3.0], 2) == _capi.ME_ERR_INVALID and less(good, 0) == _capi.ME_ERR_INVALID
    assert less(np.arange(258.0), 257) == _capi.ME_ERR_INVALID
    eng.record_observables(None)                                  # no observable store
    assert call(0, good, 2) == _capi.ME_ERR_STATE
    assert call(-1, good, 2) == _capi.ME_OK                       # ... which the energy does not need
    eng.record_energies(0)                                        # no energy store
    assert call(-1, good, 2) == _capi.ME_ERR_STATE
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples"):
        eng.free_energy_profile("energy", good, [1.0], f)
    # a scalar-temp engine without a ladder: as reweight
    scalar = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=128, temp=1.0)
    scalar.record_energies(2)
    scalar.record_observables(["real_0"])
    scalar.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
        scalar.reweight([1.0], f=[0.0])
    for which in ("real_0", "energy"):
        with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
            scalar.free_energy_profile(which, good, [1.0], f=[0.0])


# -------------------------------------------------------------------------------------------------------- 10. end to end


def test_double_well_ladder_end_to_end():
    """A small float64 double-well ladder, 8 rungs x 256 chains, 16 records of the coordinate: the engine form is bit for bit
    the engine-less form on the samples it returns, and the profile has its minima in the wells."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import demo_free_energy_profile as demo
    finally:
        sys.path.pop(0)
    eng = demo.sample(**demo.QUICK)
    assert eng.recorded_observables == ("real_0",) and eng.n_energy_records == 16
    temps = eng.temperatures
    f = eng.ladder_free_energies()["f"]
    got = eng.free_energy_profile("real_0", demo.EDGES, demo.TEMPS, f)
    e, x = eng.energy_samples(), eng.observable_samples()[:, 0]
    rungs = np.tile(np.repeat(np.arange(8), 256), 16).astype(np.int32)
    less = statistics.mbar_free_energy_profile(e, rungs, temps, f, demo.TEMPS, x, demo.EDGES)
    for key in ("mass", "below", "above", "not_a_number", "density", "free_energy", "neff_fraction"):
        assert _bitwise(got[key], less[key]), key
    assert np.array_equal(got["counts"], less["counts"]) and got["counts"].sum() + got["counts_outside"].sum() == e.size
    centers = got["centers"]
    for i in range(len(demo.TEMPS)):                           # the wells at x = +-1 lie below the barrier top at x = 0
        well = got["free_energy"][i][np.abs(np.abs(centers) - 1.0) < 0.06].max()
        top = got["free_energy"][i][np.abs(centers) < 0.06].min()
        print("T = %.2f: F(well) %.3f, F(barrier top) %.3f" % (demo.TEMPS[i], well, top))
        assert well < top


def test_the_demo_runs_to_the_end():
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "demo_free_energy_profile.py"),
                          "--quick"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout[-3000:], run.stderr[-2000:])
    assert run.returncode == 0
    lines = run.stdout.strip().splitlines()
    assert len(lines) >= 42 and "exact" in run.stdout
