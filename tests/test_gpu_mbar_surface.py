"""Joint reweighted histograms and free-energy surfaces on the GPU (csrc/me_mbar_hist2d.hip) against the long-double reference
of tests/mbar_surface_reference.py, the validated 1-D kernel and exact results.  Every figure is printed before it is asserted
(run with -s); profiles/mbar_surface.txt holds the values measured on the MI355X.

Inputs as in test_gpu_mbar_profile.py: the ragged 2048 * 3 + 5 goes through the engine-less form, the engine's stores take
512 x 33 and 2112 x 6 samples; the x values are sqrt(E) plus noise, the y values 0.2 E - 1.5 plus noise from a generator of
their own.  The temperatures per pass R follow from the cells S = (Bx + 3)(By + 3) alone: 4 up to 374, 2 up to 666, then 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref
import mbar_observables_reference as oref
import mbar_surface_reference as sref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_BOUND = 1e-8          # the project's bound for float64 quantities that pass through iterated arithmetic
# Largest relative error of a mass against the long-double reference over tests 1-3 (cells whose reference mass is not zero)
# as measured on the MI355X (profiles/mbar_surface.txt); the tests assert ten times this, capped at 1e-8.
MEASURED_SURFACE_MASS_ERROR = 1.30e-14
BOUND = min(10 * MEASURED_SURFACE_MASS_ERROR, F_BOUND)
RAGGED = 2048 * 3 + 5
LARGE = 2048 * 2048 + 5         # more tiles than blocks: a block walks more than one tile
CORNER = 2048 + 64
UNEVEN12 = 1.0 + np.concatenate([[0.0], np.cumsum([0.3, 0.2, 0.5, 0.1, 0.4, 0.6, 0.25, 0.35, 0.8, 0.15, 0.45, 0.9])])   # 1 ... 6
UNEVEN7 = np.array([-1.0, -0.4, 0.0, 0.3, 1.0, 1.6, 2.8, 4.5])
GRID33 = (np.linspace(0.5, 7.0, 34), np.linspace(-1.5, 5.0, 34))       # the cap: 36 x 36 cells, R = 1
GRID20 = (np.linspace(0.5, 7.0, 21), np.linspace(-1.5, 5.0, 21))       # 23 x 23 = 529 cells, R = 2
FLOAT_KEYS = ("mass", "density", "free_energy", "mass_slots", "outside", "neff_fraction")


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


def _flat_problem(k, n, seed=17):
    """Engine-less inputs from ref.gamma_ladder (the D = 16 quadratic form on 0.5 ... 0.5 * 1.3^7 in ``k`` rungs): ``n``
    samples, rung i % k; x = sqrt(E) plus noise, mostly inside [1, 6]; y = 0.2 E - 1.5 plus noise, mostly inside [-1, 4.5]."""
    per_rung = -(-n // k)
    energies, temps = ref.gamma_ladder(per_rung, n_rungs=k, seed=seed, ratio=(1.3 ** 7) ** (1.0 / (k - 1)))
    e = energies.T.ravel()[:n].copy()
    rungs = (np.arange(n) % k).astype(np.int32)
    x = np.sqrt(e) + 0.25 * np.random.default_rng(seed + 100).standard_normal(n)
    y = 0.2 * e - 1.5 + 0.3 * np.random.default_rng(seed + 200).standard_normal(n)
    return temps, e, rungs, x, y


def _store_problem(k, m, records, q=3, column_x=2, column_y=0, seed=19):
    """The same as an engine's stores: ``(engine, temps, energies (records, k m), rungs, columns (records, q, k m))``; the
    columns ``column_x`` and ``column_y`` hold values of _flat_problem's kind, the others noise."""
    energies, temps = ref.gamma_ladder(m * records, n_rungs=k, seed=seed, ratio=(1.3 ** 7) ** (1.0 / (k - 1)))
    e = energies.reshape(k, records, m).transpose(1, 0, 2).reshape(records, k * m).copy()
    cols = np.random.default_rng(seed + 100).standard_normal((records, q, k * m))
    cols[:, column_x] = np.sqrt(e) + 0.25 * cols[:, column_x]
    cols[:, column_y] = 0.2 * e - 1.5 + 0.3 * cols[:, column_y]
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
    empty cells exactly 0, the others within the bound; the inner views.  Returns the largest relative error of a mass (printed)."""
    bound = BOUND if bound is None else bound
    mass, counts, _ = want
    got, got_counts = out["mass_slots"], out["counts_slots"]
    bx, by = out["edges_x"].size - 1, out["edges_y"].size - 1
    assert got.shape == mass.shape and got.dtype == np.float64 and got_counts.shape == counts.shape, label
    assert got_counts.dtype == np.int64 and np.array_equal(got_counts, counts), label
    assert np.all(got[:, counts == 0] == 0.0), label
    assert np.array_equal(out["mass"], got[:, :bx, :by]) and np.array_equal(out["counts"], got_counts[:bx, :by]), label
    seen = mass != 0
    rel = float(np.max(np.abs(got.astype(np.longdouble)[seen] - mass[seen]) / mass[seen]))
    total = float(max(abs(np.sum(got[t]) - 1.0) for t in range(got.shape[0])))
    print("%s: largest relative error of a mass against long double %.3e (bound %.1e); |sum - 1| %.2e; cells filled %d of %d"
          % (label, rel, bound, total, int((counts > 0).sum()), counts.size))
    assert rel <= bound, (label, rel, bound)
    assert total <= 1e-13, label
    return rel


def _host(temps, e, rungs, f, targets, x, ex, y, ey):
    return statistics.mbar_free_energy_surface(e, rungs, temps, f, targets, x, ex, y, ey)


def _want(temps, e, rungs, f, targets, x, ex, y, ey):
    return sref.histogram2d(e, rungs, temps, f, targets, x, ex, y, ey, dtype=np.longdouble)


# --------------------------------------------------------------------- 1-3. the kernels against the long-double reference


@pytest.mark.parametrize("k, ex, ey, n_targets", [(8, UNEVEN12, UNEVEN7, 9), (33,) + GRID33 + (4,),
                                                  (8, np.linspace(0.5, 7.0, 257), np.array([-3.0, 6.0]), 3)])
def test_ragged_tile_matches_the_long_double_reference(k, ex, ey, n_targets):
    """12 x 7 uneven bins at 9 temperatures: three passes at R = 4; 33 x 33 bins: the cap, R = 1; 256 x 1 bins: the longest
    edge array (1036 cells, R = 1)."""
    temps, e, rungs, x, y = _flat_problem(k, RAGGED)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, n_targets)
    got = _host(temps, e, rungs, f, targets, x, ex, y, ey)
    bx, by = len(ex) - 1, len(ey) - 1
    shapes = {"temps": (n_targets,), "edges_x": (bx + 1,), "edges_y": (by + 1,), "centers_x": (bx,), "centers_y": (by,),
              "widths_x": (bx,), "widths_y": (by,), "mass": (n_targets, bx, by), "density": (n_targets, bx, by),
              "free_energy": (n_targets, bx, by), "mass_slots": (n_targets, bx + 3, by + 3), "outside": (n_targets,),
              "counts": (bx, by), "counts_slots": (bx + 3, by + 3), "neff_fraction": (n_targets,)}
    assert set(got) == set(shapes)              # (no "names": the engine form's)
    for key, shape in shapes.items():
        assert got[key].shape == shape, key
        assert got[key].dtype == (np.int64 if key.startswith("counts") else np.float64), key
    _check("engine-less n=%d K=%d bins=%dx%d T=%d" % (RAGGED, k, bx, by, n_targets), got, _want(temps, e, rungs, f, targets, x, ex, y, ey))
    assert np.array_equal(got["density"], got["mass"] / (np.diff(ex)[:, None] * np.diff(ey)[None, :]))
    with np.errstate(divide="ignore"):
        want_f = -targets[:, None, None] * np.log(got["density"])
    want_f[got["mass"] == 0] = np.inf
    assert np.array_equal(got["free_energy"], want_f) and np.all(np.isposinf(got["free_energy"][got["mass"] == 0]))
    inner = got["mass"].reshape(n_targets, -1).sum(axis=1)
    assert np.max(np.abs(got["outside"] + inner - 1.0)) <= 1e-13


@pytest.mark.parametrize("k, m, records", [(8, 64, 33), (33, 64, 6)])
def test_stores_match_the_reference_and_the_engine_less_form_bit_for_bit(k, m, records):
    eng, temps, e, rungs, cols = _store_problem(k, m, records)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, 5)
    label = "store %dx%d K=%d Q=3" % (records, k * m, k)
    names = eng.observable_names()
    x, y = cols[:, 2].ravel(), cols[:, 0].ravel()
    got = eng.free_energy_surface(names[2], UNEVEN12, names[0], UNEVEN7, targets, f)
    assert got["names"] == (names[2], names[0])
    _check(label, got, _want(temps, e, rungs, f, targets, x, UNEVEN12, y, UNEVEN7))
    by_index = eng.free_energy_surface(2, UNEVEN12, 0, UNEVEN7, targets, f)
    less = _host(temps, e, rungs, f, targets, x, UNEVEN12, y, UNEVEN7)
    for key in FLOAT_KEYS:
        assert _bitwise(got[key], less[key]) and _bitwise(got[key], by_index[key]), key
    assert np.array_equal(got["counts_slots"], less["counts_slots"]) and np.array_equal(got["counts"], less["counts"])
    # the axes exchanged: the counts transpose exactly; the masses agree to rounding (the total runs over the cells in
    # another order)
    swapped = eng.free_energy_surface(names[0], UNEVEN7, names[2], UNEVEN12, targets, f)
    assert swapped["names"] == (names[0], names[2])
    assert np.array_equal(swapped["counts_slots"], got["counts_slots"].T)
    a, b = swapped["mass_slots"].transpose(0, 2, 1), got["mass_slots"]
    assert np.array_equal(a == 0, b == 0)
    rel = float(np.max(np.abs(a - b)[b != 0] / b[b != 0]))
    print("%s: axes exchanged, largest relative difference of a mass %.3e (bound %.1e)" % (label, rel, BOUND))
    assert rel <= BOUND
    # the same column twice: only the diagonal fills
    twice = eng.free_energy_surface(2, UNEVEN12, 2, UNEVEN12, targets, f)
    assert twice["counts_slots"].sum() == np.trace(twice["counts_slots"]) == e.size
    # the energy as the x axis with a recorded column as y ...
    edges_e = np.linspace(0.0, 40.0, 17)
    mixed = eng.free_energy_surface("energy", edges_e, names[0], UNEVEN7, targets, f)
    assert mixed["names"] == ("energy", names[0])
    _check(label + ", energy x column", mixed, _want(temps, e, rungs, f, targets, e, edges_e, y, UNEVEN7))
    less = _host(temps, e, rungs, f, targets, e.ravel(), edges_e, y, UNEVEN7)
    for key in FLOAT_KEYS:
        assert _bitwise(mixed[key], less[key]), key
    # ... and on both axes, with the observable store and without it
    both = eng.free_energy_surface("energy", edges_e, "energy", UNEVEN12 ** 2, targets, f)
    _check(label + ", energy x energy", both, _want(temps, e, rungs, f, targets, e, edges_e, e, UNEVEN12 ** 2))
    eng.record_observables(None)                              # frees the observable store; the energy records stay
    alone = eng.free_energy_surface("energy", edges_e, "energy", UNEVEN12 ** 2, targets, f)
    assert alone["names"] == ("energy", "energy")
    for key in FLOAT_KEYS:
        assert _bitwise(both[key], alone[key]), key
    assert np.array_equal(both["counts_slots"], alone["counts_slots"])
    with pytest.raises(ValueError, match="no observable store"):
        eng.free_energy_surface("energy", edges_e, 0, UNEVEN7, targets, f)


def test_a_block_that_walks_several_tiles_matches_the_long_double_reference():
    """2048 * 2048 + 5 samples: 2049 tiles on 2048 blocks, through the engine-less form; 16 x 16 bins (361 cells, R = 4)."""
    temps, e, rungs, x, y = _flat_problem(8, LARGE)
    f = statistics.mbar_free_energies(e, rungs, temps, tol=1e-8)["f"]
    ex, ey = np.linspace(1.0, 6.0, 17), np.linspace(-1.0, 4.5, 17)
    got = _host(temps, e, rungs, f, [1.1], x, ex, y, ey)
    _check("engine-less n=%d K=8 bins=16x16 T=1" % LARGE, got, _want(temps, e, rungs, f, [1.1], x, ex, y, ey))


# ---------------------------------------------------------------------------------- 4. lane patterns and binning corners


def _pick(edges):
    """Exactly on the first, an inner and the last edge, just below each of them, and a plain inner value."""
    inner = edges[len(edges) // 2]
    return np.array([edges[0], inner, edges[-1], np.nextafter(edges[0], -np.inf), np.nextafter(inner, -np.inf),
                     np.nextafter(edges[-1], -np.inf), 0.5 * (edges[1] + edges[2])])


def _corner_values(case, rng):
    """``(x, edges_x, y, edges_y)`` of a corner case for CORNER samples; sample i sits in lane i % 64 of its wavefront."""
    i = np.arange(CORNER)
    lane = i % 64
    fine = np.linspace(0.0, 10.0, 101)          # 100 bins of 0.1
    one = np.array([0.0, 1.0])
    spread = 0.05 + 0.1 * ((lane * 37) % 64 + 8)          # 64 different bins of `fine` per wavefront
    if case == "one cell":                      # a wavefront's 64 lanes in one cell: one match round
        return 2.0 + 0.4 * rng.random(CORNER), UNEVEN12 + 0.5, 0.35 + 0.5 * rng.random(CORNER), UNEVEN7
    if case == "64 distinct on one x row":      # 4 x 103 = 412 cells (R = 2)
        return np.full(CORNER, 0.5), one, spread, fine
    if case == "64 distinct on one y column":   # 103 x 4 cells
        return spread, fine, np.full(CORNER, 0.5), one
    if case == "64 distinct on two diagonals":
        # 64 cells of ONE diagonal would need 64 slots on both axes, beyond the cap of 1296 cells: 32 x 32 bins (35 x 35
        # cells, R = 1), lanes 0 .. 31 on the diagonal (l, l), lanes 32 .. 63 on the one beside it (l, l + 1 mod 32)
        edges = np.arange(33.0)
        return (lane % 32) + 0.5, edges, ((lane % 32) + lane // 32) % 32 + 0.5, edges
    if case == "groups of 9 and 8":             # the two sides of kDense = 8: lanes 0-8 share a cell, lanes 9-16 another, the
        edges = np.arange(9.0)                  # other 47 lanes hold cells of their own (8 x 8 bins, R = 4)
        cell = np.where(lane < 9, 0, np.where(lane < 17, 1, lane - 15))
        return cell // 8 + 0.25 + 0.5 * rng.random(CORNER), edges, cell % 8 + 0.25 + 0.5 * rng.random(CORNER), edges
    if case == "on the edges":                  # all 49 pairs of the seven picks per axis
        return _pick(UNEVEN12)[i % 7], UNEVEN12, _pick(UNEVEN7)[(i // 7) % 7], UNEVEN7
    assert case == "inf and nan"
    x, y = 1.0 + 5.0 * rng.random(CORNER), -1.0 + 5.5 * rng.random(CORNER)
    x[::7], x[3::11], x[5::13] = np.inf, -np.inf, np.nan
    y[2::9], y[4::10], y[6::17] = np.inf, -np.inf, np.nan
    y[5::26] = np.nan                           # (every second NaN of x: NaN on both)
    x[[0, 63, 64, 2047, 2048, CORNER - 1]] = [np.nan, -np.inf, np.inf, np.nan, np.inf, -np.inf]
    y[[0, 63, 64, 2047, 2048, CORNER - 1]] = [np.nan, np.nan, 1.0, np.inf, -np.inf, np.nan]
    return x, UNEVEN12, y, UNEVEN7


@pytest.mark.parametrize("case", ["one cell", "64 distinct on one x row", "64 distinct on one y column", "64 distinct on two diagonals",
                                  "groups of 9 and 8", "on the edges", "inf and nan"])
def test_lane_patterns_and_binning_corners(case):
    temps, e, rungs, _, _ = _flat_problem(8, CORNER, seed=31)
    x, ex, y, ey = _corner_values(case, np.random.default_rng(41))
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 5)
    got = _host(temps, e, rungs, f, targets, x, ex, y, ey)
    want = _want(temps, e, rungs, f, targets, x, ex, y, ey)
    _check(case, got, want)
    counts = got["counts_slots"]
    bx, by = len(ex) - 1, len(ey) - 1
    filled = int((counts > 0).sum())
    cells = sref.slots(x, ex) * (by + 3) + sref.slots(y, ey)
    if case == "one cell":
        assert filled == 1 and got["counts"].max() == CORNER
    if case.startswith("64 distinct"):
        assert filled == 64 and got["counts"].sum() == CORNER
        for w in range(CORNER // 64):
            assert len(set(cells[64 * w:64 * w + 64])) == 64
        if case.endswith("x row"):
            assert np.count_nonzero(counts.sum(axis=1)) == 1 and np.count_nonzero(counts.sum(axis=0)) == 64
        if case.endswith("y column"):
            assert np.count_nonzero(counts.sum(axis=0)) == 1 and np.count_nonzero(counts.sum(axis=1)) == 64
        if case.endswith("diagonals"):
            assert np.count_nonzero(counts.sum(axis=0)) == 32 and np.count_nonzero(counts.sum(axis=1)) == 32
    if case == "groups of 9 and 8":
        assert filled == 49
        for w in range(CORNER // 64):
            sizes = sorted(np.bincount(cells[64 * w:64 * w + 64])[np.unique(cells[64 * w:64 * w + 64])].tolist())
            assert sizes == [1] * 47 + [8, 9]
    if case == "on the edges":
        # per axis: first edge -> bin 0, inner edge -> its bin, last edge -> above, below the first -> below, ...
        assert filled == 49 and counts[bx + 2].sum() == 0 and counts[:, by + 2].sum() == 0
        assert counts[bx, by] > 0 and counts[bx + 1, by + 1] > 0 and counts[bx, by + 1] > 0 and counts[bx + 1, by] > 0
        assert counts[0, 0] > 0 and counts[bx - 1, by - 1] > 0 and counts[bx, 0] > 0 and counts[0, by + 1] > 0
    if case == "inf and nan":
        assert np.all(counts[bx:].sum(axis=1) > 0) and np.all(counts[:, by:].sum(axis=0) > 0)
        assert np.all(counts[bx:, :by].sum(axis=1) > 0) and np.all(counts[:bx, by:].sum(axis=0) > 0)     # on one axis only
        assert np.all(counts[bx:, by:] > 0)                                                             # on both: all 9 pairs
        assert counts[bx + 2, by + 2] == (np.isnan(x) & np.isnan(y)).sum() > 0
        assert counts[bx + 2].sum() == np.isnan(x).sum() and counts[:, by + 2].sum() == np.isnan(y).sum()
        assert counts.sum() == CORNER


# ------------------------------------------------------------------------------ 5. independence of the request, reproducibility


@pytest.mark.parametrize("ex, ey", [(UNEVEN12, UNEVEN7), GRID20, GRID33], ids=["R=4", "R=2", "R=1"])
def test_results_do_not_depend_on_the_request_and_are_reproducible(ex, ey):
    temps, e, rungs, x, y = _flat_problem(8, RAGGED, seed=37)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 9)
    whole = _host(temps, e, rungs, f, targets, x, ex, y, ey)
    again = _host(temps, e, rungs, f, targets, x, ex, y, ey)
    for key in FLOAT_KEYS:
        assert _bitwise(whole[key], again[key]), key              # two calls
    assert np.array_equal(whole["counts_slots"], again["counts_slots"])
    for t in range(9):
        one = _host(temps, e, rungs, f, [targets[t]], x, ex, y, ey)
        for key in FLOAT_KEYS:
            assert _bitwise(one[key][0], whole[key][t]), (key, t)     # alone = among 9
        assert np.array_equal(one["counts_slots"], whole["counts_slots"])


# ------------------------------------------------------------------------------------------ 6. tie to the validated 1-D kernel


def _one_d(prof):
    return (np.concatenate([prof["mass"], prof["below"][:, None], prof["above"][:, None], prof["not_a_number"][:, None]], axis=1),
            np.concatenate([prof["counts"], prof["counts_outside"]]))


def _relative(label, got, want):
    assert np.array_equal(got == 0, want == 0), label
    rel = float(np.max(np.abs(got - want)[want != 0] / want[want != 0]))
    print("%s: largest relative difference %.3e (bound %.1e)" % (label, rel, BOUND))
    assert rel <= BOUND, label


def test_sums_over_an_axis_are_the_one_dimensional_histograms():
    temps, e, rungs, x, y = _flat_problem(8, RAGGED, seed=43)
    x[[11, 500]], y[[11, 900]] = np.nan, np.nan                # (so that every outer slot of the 1-D calls can be compared)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 5)
    got = _host(temps, e, rungs, f, targets, x, UNEVEN12, y, UNEVEN7)
    along_x = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, x, UNEVEN12)
    along_y = statistics.mbar_free_energy_profile(e, rungs, temps, f, targets, y, UNEVEN7)
    for label, prof, axis in (("sum over y against the profile along x", along_x, 2), ("sum over x against the profile along y", along_y, 1)):
        mass, counts = _one_d(prof)
        assert np.array_equal(got["counts_slots"].sum(axis=axis - 1), counts), label
        assert counts[-1] == 2
        _relative(label, got["mass_slots"].sum(axis=axis), mass)
        assert _bitwise(got["neff_fraction"], prof["neff_fraction"]), label      # reweight_enqueue's in both
    # a y axis whose single bin holds every sample: the 1-D masses
    y_all = np.where(np.isnan(y), 0.0, y)
    flat = _host(temps, e, rungs, f, targets, x, UNEVEN12, y_all, [-1e6, 1e6])
    assert flat["counts_slots"][:, 1:].sum() == 0 and np.all(flat["mass_slots"][:, :, 1:] == 0.0)
    mass, counts = _one_d(along_x)
    assert np.array_equal(flat["counts_slots"][:, 0], counts)
    _relative("one y bin that holds every sample against the profile along x", flat["mass_slots"][:, :, 0], mass)


# ------------------------------------------------------------------------------------------------- 7. non-finite energies


def test_samples_with_non_finite_energies_are_not_used():
    temps, e, rungs, x, y = _flat_problem(8, RAGGED, seed=23)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    dirty, dirty_x, dirty_y = e.copy(), x.copy(), y.copy()
    dirty[[3, 64, 2047, 2048, 4100, RAGGED - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    dirty_x[[3, 64, 4100]] = np.nan                           # of unused samples: never seen
    dirty_y[[64, 2047]] = np.nan
    targets = _targets(temps, 4)
    got = _host(temps, dirty, rungs, f, targets, dirty_x, UNEVEN12, dirty_y, UNEVEN7)
    _check("engine-less n=%d K=8, 6 unused samples" % RAGGED, got,
           _want(temps, dirty, rungs, f, targets, dirty_x, UNEVEN12, dirty_y, UNEVEN7))
    assert got["counts_slots"].sum() == np.isfinite(dirty).sum() == RAGGED - 6
    assert got["counts_slots"][-1].sum() == 0 and got["counts_slots"][:, -1].sum() == 0
    dirty[rungs == 5] = np.nan                                # a rung left without a finite sample
    with pytest.raises(_capi.MetropolisLibraryError, match="rung 5 of 8 has no sample with a finite energy"):
        _host(temps, dirty, rungs, f, targets, dirty_x, UNEVEN12, dirty_y, UNEVEN7)


# ------------------------------------------------------------------------------------------------------ 8. exact physics


def test_exact_cell_probabilities_of_the_quadratic_energy():
    """Exact samples of E = |x|^2 in 4 real dimensions on LADDER8, 16 independent subsets of 8 x 1024: the masses of (x_0,
    x_1) in the 4 x 4 bins of SURFACE_EDGES_X and SURFACE_EDGES_Y, below and above on both axes at three temperatures between
    rungs against the products of the exact 1-D probabilities, 3 x 6 x 6 comparisons, each within 5 standard errors.
    tests/test_mbar_surface_cpu.py shows that the reference meets all of them on these very inputs (the largest deviation is
    2.55 standard errors, the least exact mass 5.4e-6) and that a transposed table does not."""
    results = []
    for e, rungs, cols in sref.xy_quadratic_subsets():
        out = statistics.mbar_free_energies(e, rungs, oref.LADDER8)
        assert out["converged"]
        surf = statistics.mbar_free_energy_surface(e, rungs, oref.LADDER8, out["f"], oref.PHYSICS_TARGETS, cols[0],
                                                   sref.SURFACE_EDGES_X, cols[1], sref.SURFACE_EDGES_Y)
        assert surf["counts_slots"][-1].sum() == 0 and surf["counts_slots"][:, -1].sum() == 0
        results.append(surf["mass_slots"])
    est, exact = sref.physics_masses(results, oref.PHYSICS_TARGETS)
    ok, m, se = ref.within_5_se(est, exact)
    dev = np.abs(m - exact) / se
    print("deviation / se of the 3 x 6 x 6 masses: largest %.2f; least exact mass %.2e\n" % (dev.max(), exact.min()), dev)
    assert ok.shape == (3, 6, 6) and np.all(ok)


# ------------------------------------------------------------------------------------------------------------- 9. errors


def _ptr(a):
    return _capi.double_ptr(np.ascontiguousarray(a, dtype=np.float64))


def test_error_cases():
    eng, temps, e, rungs, cols = _store_problem(8, 64, 2)
    f = eng.ladder_free_energies()["f"]
    good = np.array([1.0, 2.0, 3.0])
    for edges in ([1.0, 2.0, 2.0], [1.0, 3.0, 2.0], [1.0, np.nan, 3.0], [1.0], np.arange(258.0)):
        for ex, ey in ((edges, good), (good, edges)):
            with pytest.raises(ValueError):
                eng.free_energy_surface("real_0", ex, "real_2", ey, [1.0], f)
            with pytest.raises(ValueError):
                _host(temps, e, rungs, f, [1.0], cols[:, 0].ravel(), ex, cols[:, 2].ravel(), ey)
    with pytest.raises(ValueError, match="at most 1296 cells"):
        eng.free_energy_surface("real_0", np.arange(35.0), "real_2", np.arange(34.0), [1.0], f)
    with pytest.raises(ValueError, match="unknown recorded observable"):
        eng.free_energy_surface("real_0", good, "real_3", good, [1.0], f)          # in the catalogue, not recorded
    with pytest.raises(ValueError, match="outside the 3 recorded columns"):
        eng.free_energy_surface(3, good, 0, good, [1.0], f)
    for bad in ([0.0], [1.0, -1.0], [np.nan], []):
        with pytest.raises(ValueError):
            eng.free_energy_surface("real_0", good, "real_2", good, bad, f)
    # the same through the C ABI
    lib, h = eng._lib, eng._handle
    fp, tp = _ptr(f), _ptr([1.0])

    def call(cx, ex, bx, cy, ey, by, temps_ptr=tp):
        return lib.me_mbar_histogram_joint(h, fp, temps_ptr, 1, cx, _ptr(ex), bx, cy, _ptr(ey), by, None, None, None)

    assert call(1, good, 2, 2, good, 2) == _capi.ME_OK            # every output may be null
    assert call(-1, good, 2, 2, good, 2) == _capi.ME_OK and call(1, good, 2, -1, good, 2) == _capi.ME_OK
    assert call(-1, good, 2, -1, good, 2) == _capi.ME_OK and call(1, good, 2, 1, good, 2) == _capi.ME_OK
    for bad, n_bins in (([1.0, 2.0, 2.0], 2), ([1.0, 3.0, 2.0], 2), ([1.0, np.nan, 3.0], 2), ([1.0, np.inf], 1), (good, 0),
                        (np.arange(258.0), 257)):
        assert call(1, bad, n_bins, 2, good, 2) == _capi.ME_ERR_INVALID, (bad, n_bins)
        assert call(1, good, 2, 2, bad, n_bins) == _capi.ME_ERR_INVALID, (bad, n_bins)
    assert call(1, np.arange(257.0), 256, 2, good, 2) == _capi.ME_OK               # 259 x 5 = 1295 cells
    assert call(1, good, 2, 2, np.arange(257.0), 256) == _capi.ME_OK
    assert call(1, np.arange(257.0), 256, 2, np.arange(4.0), 3) == _capi.ME_ERR_INVALID    # 259 x 6 cells
    assert call(1, np.arange(34.0), 33, 2, np.arange(34.0), 33) == _capi.ME_OK             # 36 x 36 = 1296 cells
    assert call(1, np.arange(35.0), 34, 2, np.arange(34.0), 33) == _capi.ME_ERR_INVALID
    assert call(1, np.arange(34.0), 33, 2, np.arange(35.0), 34) == _capi.ME_ERR_INVALID
    assert "1296" in _capi.last_error(h)
    for column in (3, -2):                                        # column index >= recorded columns; neither recorded nor -1
        assert call(column, good, 2, 1, good, 2) == _capi.ME_ERR_INVALID and call(1, good, 2, column, good, 2) == _capi.ME_ERR_INVALID
    assert call(1, good, 2, 2, good, 2, _ptr([0.0])) == _capi.ME_ERR_INVALID       # temperature <= 0
    assert call(1, good, 2, 2, good, 2, _ptr([-1.0])) == _capi.ME_ERR_INVALID
    r32, x, y = np.ascontiguousarray(rungs, dtype=np.int32), cols[:, 0].ravel().copy(), cols[:, 2].ravel().copy()

    def less(ex, bx, ey, by):
        return lib.me_mbar_histogram_joint_samples(0, _ptr(e), _capi.int32_ptr(r32), e.size, _ptr(temps), 8, fp, tp, 1, _capi.double_ptr(x),
                                               _capi.double_ptr(y), _ptr(ex), bx, _ptr(ey), by, None, None, None)

    assert less(good, 2, good, 2) == _capi.ME_OK
    assert less([1.0, 1.0, 3.0], 2, good, 2) == _capi.ME_ERR_INVALID and less(good, 2, good, 0) == _capi.ME_ERR_INVALID
    assert less(good, 2, np.arange(258.0), 257) == _capi.ME_ERR_INVALID
    assert less(np.arange(34.0), 33, np.arange(34.0), 33) == _capi.ME_OK
    assert less(np.arange(34.0), 33, np.arange(35.0), 34) == _capi.ME_ERR_INVALID
    eng.record_observables(None)                                  # no observable store
    assert call(0, good, 2, -1, good, 2) == _capi.ME_ERR_STATE and call(-1, good, 2, 0, good, 2) == _capi.ME_ERR_STATE
    assert call(-1, good, 2, -1, good, 2) == _capi.ME_OK          # ... which the energy does not need
    eng.record_energies(0)                                        # no energy store
    assert call(-1, good, 2, -1, good, 2) == _capi.ME_ERR_STATE
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples"):
        eng.free_energy_surface("energy", good, "energy", good, [1.0], f)
    # a scalar-temp engine without a ladder: as reweight
    scalar = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=128, temp=1.0)
    scalar.record_energies(2)
    scalar.record_observables(["real_0"])
    scalar.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
        scalar.free_energy_surface("real_0", good, "energy", good, [1.0], f=[0.0])


# -------------------------------------------------------------------------------------------------------- 10. end to end


def test_valley_well_ladder_end_to_end():
    """The demo's two-parameter double well, 8 rungs x 256 chains, 16 records of both coordinates: the engine form is bit for bit
    the engine-less form on the samples it returns, and at the coldest target both wells hold mass and the saddle's cell less
    than either."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import demo_free_energy_surface as demo
    finally:
        sys.path.pop(0)
    eng = demo.sample(**demo.QUICK)
    assert eng.recorded_observables == ("real_0", "real_1") and eng.n_energy_records == 16
    temps = eng.temperatures
    f = eng.ladder_free_energies()["f"]
    got = eng.free_energy_surface("real_0", demo.EDGES_X, "real_1", demo.EDGES_Y, demo.TEMPS, f)
    assert got["names"] == ("real_0", "real_1")
    e, cols = eng.energy_samples(), eng.observable_samples()
    rungs = np.tile(np.repeat(np.arange(8), 256), 16).astype(np.int32)
    less = _host(temps, e, rungs, f, demo.TEMPS, cols[:, 0], demo.EDGES_X, cols[:, 1], demo.EDGES_Y)
    for key in FLOAT_KEYS:
        assert _bitwise(got[key], less[key]), key
    assert np.array_equal(got["counts_slots"], less["counts_slots"]) and got["counts_slots"].sum() == e.size
    right, saddle = demo.cell_of(got, demo.WELL), demo.cell_of(got, demo.SADDLE)
    left = demo.cell_of(got, (-demo.WELL[0], demo.WELL[1]))
    cold = got["mass"][int(np.argmin(demo.TEMPS))]
    print("T = %.2f: mass of the left well's cell %.4e, of the right well's %.4e, of the saddle's %.4e"
          % (demo.TEMPS.min(), cold[left], cold[right], cold[saddle]))
    assert cold[left] > 0 and cold[right] > 0 and cold[saddle] < cold[left] and cold[saddle] < cold[right]


def test_the_demo_runs_to_the_end():
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "demo_free_energy_surface.py"),
                          "--quick"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout[-4000:], run.stderr[-2000:])
    assert run.returncode == 0
    lines = run.stdout.strip().splitlines()
    assert len(lines) >= 30 and "exact" in lines[-1]
