"""Error bars of joint reweighted histograms and free-energy surfaces on the GPU (csrc/me_mbar_hist2d_cov.hip: the cell Gram
sums; metropolisengine_amd/statistics.py: the reduced algebra) against the long-double restatement in
tests/mbar_surface_uncertainty_reference.py, against identities that need no reference, against the 1-D unit, and against exact
cell probabilities.  Every figure is printed before it is asserted (run with -s); profiles/mbar_surface_uncertainty.txt holds
the values measured on the MI355X."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_observable_uncertainty_reference as oref
import mbar_profile_uncertainty_reference as ref1d
import mbar_surface_uncertainty_reference as ref
from test_gpu_mbar_surface import CORNER, _corner_values, _flat_problem, _store_problem, _targets
from test_gpu_mbar_uncertainty import TERM_ROUNDING, _gram_samples
from test_gpu_mbar_profile_uncertainty import _hist_gram

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, IP, LP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
N = uref.N_GRAM                 # three tiles and a ragged fourth
LARGE = 2048 * 2048 + 5         # more tiles than blocks: a block walks several tiles
F_BOUND = 1e-8                  # the project's bound for float64 quantities that pass through iterated arithmetic
# (K, grid, targets).  K + 1 = 9, 34, 65 rows are no multiple of any R; one grid per R of csrc/me_mbar_hist2d_cov.hip's rule (42
# cells R = 16, 150 R = 8, 400 R = 4, 784 R = 2, 841 and 1296 R = 1: ref.ROWS); 5 targets: more than one pass per row chunk; "E":
# the x axis is the energy itself
CASES = [(8, "4x3", 1), (33, "12x7", 5), (64, "17x17", 1), (8, "25x25", 5), (33, "26x26", 1), (8, "33x33", 1), (8, "E13x9", 1)]
ENERGY_EDGES = np.linspace(2.0, 28.0, 14)
NEW_KEYS = {"d_mass", "d_mass_slots", "d_outside", "d_free_energy", "lowest", "d_free_energy_from_lowest", "log_mass_cov", "n_samples"}
FLOAT_KEYS = ("mass", "density", "free_energy", "mass_slots", "outside", "neff_fraction", "d_mass", "d_mass_slots", "d_outside",
              "d_free_energy", "d_free_energy_from_lowest", "log_mass_cov")


def gram_bound(n):
    """A term of H is a product of two exponentials: 3 * 2^-53 each (exp_nonpos, tests/test_gpu_mbar_uncertainty.py) and the
    product, which TERM_ROUNDING covers; every term is >= 0, so n 2^-53 covers ANY order of the sum of n of them."""
    return (n + TERM_ROUNDING) * 2.0 ** -53


GRAM_BOUND = gram_bound(N)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return _bitwise(a, b) if a.dtype == np.float64 else np.array_equal(a, b)


def _joint_gram(energies, rungs, temps, f, targets, x, ex, y, ey):
    """me_mbar_histogram_joint_gram_samples: (cell_gram (T, K + 1, S), ladder_gram, column_counts, mass (T, S), counts (S,),
    neff_fraction, n_used)."""
    e = np.ascontiguousarray(energies, dtype=np.float64).ravel()
    r = np.ascontiguousarray(rungs, dtype=np.int32).ravel()
    t = np.ascontiguousarray(temps, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    a, b = np.ascontiguousarray(x, dtype=np.float64).ravel(), np.ascontiguousarray(y, dtype=np.float64).ravel()
    ex, ey = np.ascontiguousarray(ex, dtype=np.float64), np.ascontiguousarray(ey, dtype=np.float64)
    k, s = t.size, (ex.size + 2) * (ey.size + 2)
    h, ladder, cc = np.zeros((tg.size, k + 1, s)), np.zeros((k, k)), np.zeros(k)
    mass, counts, neff = np.zeros((tg.size, s)), np.zeros(s, dtype=np.int64), np.zeros(tg.size)
    n_used = ctypes.c_int64()
    _capi.check(_capi.load().me_mbar_histogram_joint_gram_samples(
        0, e.ctypes.data_as(DP), r.ctypes.data_as(IP), e.size, t.ctypes.data_as(DP), k, f.ctypes.data_as(DP), tg.ctypes.data_as(DP),
        tg.size, a.ctypes.data_as(DP), b.ctypes.data_as(DP), ex.ctypes.data_as(DP), ex.size - 1, ey.ctypes.data_as(DP), ey.size - 1,
        h.ctypes.data_as(DP), ladder.ctypes.data_as(DP), cc.ctypes.data_as(DP), mass.ctypes.data_as(DP), counts.ctypes.data_as(LP),
        neff.ctypes.data_as(DP), ctypes.byref(n_used)))
    return h, ladder, cc, mass, counts, neff, n_used.value


@functools.lru_cache(maxsize=None)
def _inputs(k):
    temps, energies, rungs = uref.synthetic(k)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-13)["f"]
    x = ref.synthetic_values(energies, temps, rungs)
    return temps, energies, rungs, f, x, ref.synthetic_values_y(energies, x)


def _grid(grid, energies, x):
    """``(values_x, edges_x, edges_y)``: "E13x9" has the energy itself on the x axis."""
    if grid.startswith("E"):
        return energies, ENERGY_EDGES, ref.GRIDS[grid[1:]][1]
    return (x,) + ref.GRIDS[grid]


@functools.lru_cache(maxsize=None)
def _case(k, grid, n_targets):
    """Inputs, the device's sums and the long-double reference of one case, computed once and left unchanged."""
    temps, energies, rungs, f, x, y = _inputs(k)
    x, ex, ey = _grid(grid, energies, x)
    targets = uref.targets_for(temps, n_targets)
    dev = _joint_gram(energies, rungs, temps, f, targets, x, ex, y, ey)
    h, mass, counts, w, ladder_counts = ref.cell_gram(energies, rungs, temps, f, targets, x, ex, y, ey)
    return dict(k=k, temps=temps, energies=energies, rungs=rungs, f=f, x=x, y=y, ex=ex, ey=ey, targets=targets, dev=dev, h=h,
                mass=mass, counts=counts, w=w, ladder_counts=ladder_counts)


def _args(case):
    return (case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], case["x"], case["ex"], case["y"], case["ey"])


def _h_error(h_dev, h_ref):
    """Largest |H_dev - H_ref| / H_ref over the entries with H_ref != 0; the others must be exactly 0."""
    seen = h_ref != 0
    assert np.all(h_dev[~seen] == 0.0)
    return float((np.abs(h_dev.astype(ref.LD) - h_ref)[seen] / h_ref[seen]).max())


# ---------------------------------------------------------------------------------------- 1. H against the long-double H
@pytest.mark.parametrize("k,grid,n_targets", CASES)
def test_cell_gram_against_the_long_double_reference(k, grid, n_targets):
    """Entrywise |H_dev - H_ref| <= (N + c) 2^-53 H_ref.  Empty cells exactly 0, counts exact, masses those of
    mbar_free_energy_surface bit for bit, the ladder block that of me_mbar_gram_samples with no targets bit for bit."""
    case = _case(k, grid, n_targets)
    h, ladder, cc, mass, counts, neff, n_used = case["dev"]
    s = (case["ex"].size + 2) * (case["ey"].size + 2)
    if grid in ref.ROWS:
        assert ref.rule_rows(s) == ref.ROWS[grid]
    err = _h_error(h, case["h"])
    print("K = %d, %s, %d targets (%d cells, R = %d): largest relative error of H %.3e (bound %.3e); %d cells filled"
          % (k, grid, n_targets, s, ref.rule_rows(s), err, GRAM_BOUND, int((case["counts"] > 0).sum())))
    assert h.shape == (n_targets, k + 1, s) and n_used == N
    assert np.array_equal(counts, case["counts"]) and counts.dtype == np.int64
    assert np.all(h[:, :, case["counts"] == 0] == 0.0) and np.all(h[:, :, case["counts"] > 0] > 0.0)
    assert np.array_equal(cc, np.asarray(case["ladder_counts"], dtype=np.float64))
    surf = statistics.mbar_free_energy_surface(*_args(case))
    assert _bitwise(mass, surf["mass_slots"].reshape(n_targets, s)) and _bitwise(neff, surf["neff_fraction"])
    assert np.array_equal(counts, surf["counts_slots"].ravel())
    plain = _gram_samples(case["energies"], case["rungs"], case["temps"], case["f"], np.zeros(0))
    assert _bitwise(ladder, plain[0]) and np.array_equal(cc, plain[1])
    assert err <= GRAM_BOUND


# ------------------------------------------------------------------------------ 2. identities that need no reference
def _identities(label, n, k, energies, rungs, temps, f, targets, x, ex, y, ey):
    """tests/test_gpu_mbar_profile_uncertainty.py's _identities with S cells for the B + 3 slots: (a) sum_c H[t][j][c] = G[j, K +
    2 t] and (b) sum_c H[t][K][c] = G[K + 2 t, K + 2 t] of me_mbar_gram_samples; (c) sum_k N_k H[t][k][c] = mass[t][c]."""
    h, _, cc, mass, _, _, _ = _joint_gram(energies, rungs, temps, f, targets, x, ex, y, ey)
    gram = _gram_samples(energies, rungs, temps, f, targets)[0]
    n_cells, u = h.shape[2], 2.0 ** -53
    worst = {}
    for t in range(len(targets)):
        a = k + 2 * t
        lhs = h[t].sum(axis=1)
        bound_ab = ((n + TERM_ROUNDING + n_cells) + (n + TERM_ROUNDING)) * u
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


@pytest.mark.parametrize("k,grid,n_targets", [(8, "4x3", 1), (33, "12x7", 5), (8, "25x25", 5)])
def test_identities_with_the_gram_matrix_and_the_masses(k, grid, n_targets):
    case = _case(k, grid, n_targets)
    _identities("K = %d, %s, %d targets" % (k, grid, n_targets), N, k, *_args(case))


def test_identities_where_a_block_walks_several_tiles():
    """2048 * 2048 + 5 samples: 2049 tiles on 2048 blocks."""
    temps, energies, rungs = uref.synthetic(8, n=LARGE)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-8)["f"]
    x = ref.synthetic_values(energies, temps, rungs)
    y = ref.synthetic_values_y(energies, x)
    _identities("n = %d, K = 8, 4 x 3 bins, 1 target" % LARGE, LARGE, 8, energies, rungs, temps, f, uref.targets_for(temps, 1), x,
                ref.GRIDS["4x3"][0], y, ref.GRIDS["4x3"][1])


# ----------------------------------------------------------------------------------- 3. the derived quantities and the 1-D unit
@pytest.mark.parametrize("k,grid,n_targets", [(8, "4x3", 1), (33, "12x7", 5)])
def test_uncertainties_against_the_reference(k, grid, n_targets):
    """mbar_free_energy_surface_uncertainties (the device's H, the library's reduced algebra) against ref.derived on the SVD route
    of the explicit long-double weight matrix: variances within 4 b max |Theta|, b = ref.route_bound + GRAM_BOUND, capped at
    F_BOUND (the rule of tests/test_gpu_mbar_profile_uncertainty.py)."""
    case = _case(k, grid, n_targets)
    ex, ey, targets = case["ex"], case["ey"], case["targets"]
    bx, by = ex.size - 1, ey.size - 1
    out = statistics.mbar_free_energy_surface_uncertainties(*_args(case))
    lean = statistics.mbar_free_energy_surface_uncertainties(*_args(case), covariance=False)
    surf = statistics.mbar_free_energy_surface(*_args(case))
    assert set(out) == set(surf) | NEW_KEYS and set(lean) == set(out) - {"log_mass_cov"} and out["n_samples"] == N
    for key in surf:
        assert _same(out[key], surf[key]), key
    for key in lean:
        assert _same(out[key], lean[key]), key
    cells = ref.cells_of(case["x"], ex, case["y"], ey)
    worst = 0.0
    for t in range(n_targets):
        explicit, live = ref.explicit_weight_matrix(case["w"], k, t, cells, case["mass"][t])
        cc = ref.column_counts(case["ladder_counts"], live.size)
        theta = ref.theta_svd(explicit, cc)
        want = ref.derived(theta, k, live, case["mass"][t], targets[t], ex, ey)
        bound = min(4.0 * (ref.route_bound(explicit, cc) + GRAM_BOUND), F_BOUND) * np.abs(theta).max()
        p = np.asarray(case["mass"][t], dtype=np.float64).reshape(bx + 3, by + 3)
        full = p > 0
        got = out["d_mass_slots"][t]
        empty = ~full[:bx, :by]
        assert np.all(got[~full] == 0.0) and np.array_equal(np.isnan(out["d_free_energy"][t]), empty)
        assert np.array_equal(np.isnan(out["d_free_energy_from_lowest"][t]), empty)
        assert np.array_equal(np.isnan(out["log_mass_cov"][t]), empty.ravel()[:, None] | empty.ravel()[None, :])
        assert np.array_equal(out["lowest"][t], want["lowest"]) and out["d_free_energy_from_lowest"][t][tuple(want["lowest"])] == 0.0
        tt = targets[t]
        err = max(np.abs((got[full] / p[full]) ** 2 - (want["d_slots"][full] / p[full]) ** 2).max(),
                  np.nanmax(np.abs(out["log_mass_cov"][t] - want["log_mass_cov"])),
                  np.nanmax(np.abs((out["d_free_energy"][t] / tt) ** 2 - (want["d_free_energy"] / tt) ** 2)),
                  np.nanmax(np.abs((out["d_free_energy_from_lowest"][t] / tt) ** 2 - (want["d_free_energy_from_lowest"] / tt) ** 2)),
                  abs(out["d_outside"][t] ** 2 - want["var_outside"]))
        print("K = %d, %s, target %d: largest error of a variance %.3e (bound %.3e); outside %.4f +- %.4f"
              % (k, grid, t, err, bound, out["outside"][t], out["d_outside"][t]))
        worst = max(worst, err / bound)
        assert err <= bound
    print("    worst error / bound %.3e" % worst)


def test_a_single_y_bin_is_the_one_dimensional_unit_bit_for_bit():
    """A y axis of one bin that encloses every y value: H2d[t][j][slot_x, 0] is me_mbar_histogram_gram_samples' H[t][j][slot_x]
    bit for bit (the same cells' samples in the same order through the same instructions), and d_mass[:, :, 0] is the 1-D
    d_mass: Var ln p within 4 b max |Theta| with b = ref.route_bound of the 1-D explicit weight matrix (the two weight matrices
    hold the same non-zero columns)."""
    k = 8
    temps, energies, rungs, f, x, y = _inputs(k)
    targets = uref.targets_for(temps, 5)
    ex, ey = ref.UNEVEN12, np.array([-100.0, 100.0])
    assert np.all((y >= ey[0]) & (y < ey[1]))
    h2, ladder2, _, mass2, counts2, _, _ = _joint_gram(energies, rungs, temps, f, targets, x, ex, y, ey)
    h1, ladder1, _, mass1, counts1, _, _ = _hist_gram(energies, rungs, temps, f, targets, x, ex)
    h2 = h2.reshape(5, k + 1, ex.size + 2, 4)
    assert _bitwise(h2[:, :, :, 0], h1) and np.all(h2[:, :, :, 1:] == 0.0) and _bitwise(ladder2, ladder1)
    assert np.array_equal(counts2.reshape(-1, 4)[:, 0], counts1) and _bitwise(mass2.reshape(5, -1, 4)[:, :, 0], mass1)
    two = statistics.mbar_free_energy_surface_uncertainties(energies, rungs, temps, f, targets, x, ex, y, ey)
    one = statistics.mbar_free_energy_profile_uncertainties(energies, rungs, temps, f, targets, x, ex)
    _, mass_ld, _, w, ladder_counts = ref1d.slot_gram(energies, rungs, temps, f, targets, x, ex)
    for t in range(5):
        explicit, live = ref1d.explicit_weight_matrix(w, k, t, x, ex, mass_ld[t])
        cc = ref1d.column_counts(ladder_counts, live.size)
        bound = 4.0 * ref1d.route_bound(explicit, cc) * np.abs(ref1d.theta_svd(explicit, cc)).max()
        p = one["mass"][t]
        err = np.abs((two["d_mass"][t][:, 0] / p) ** 2 - (one["d_mass"][t] / p) ** 2).max()
        print("target %d: Var ln p of d_mass[:, :, 0] against the 1-D d_mass %.3e (bound %.3e)" % (t, err, bound))
        assert err <= bound


def test_the_x_marginal_of_the_cell_covariance_is_the_one_dimensional_variance():
    """A 12 x 7 grid whose y edges enclose every value: Var p_x = sum_{y, y'} p_c p_c' C_cc' over the cells of one x bin against
    the 1-D d_mass^2, as Var ln p_x, within the bound of the test above."""
    k = 8
    temps, energies, rungs, f, x, y = _inputs(k)
    targets = uref.targets_for(temps, 1)
    ex, ey = ref.UNEVEN12, np.linspace(y.min() - 0.1, y.max() + 0.1, 8)
    two = statistics.mbar_free_energy_surface_uncertainties(energies, rungs, temps, f, targets, x, ex, y, ey)
    one = statistics.mbar_free_energy_profile_uncertainties(energies, rungs, temps, f, targets, x, ex)
    _, mass_ld, _, w, ladder_counts = ref1d.slot_gram(energies, rungs, temps, f, targets, x, ex)
    explicit, live = ref1d.explicit_weight_matrix(w, k, 0, x, ex, mass_ld[0])
    cc = ref1d.column_counts(ladder_counts, live.size)
    bound = 4.0 * ref1d.route_bound(explicit, cc) * np.abs(ref1d.theta_svd(explicit, cc)).max()
    assert two["counts_slots"][:12, 7:].sum() == 0
    p, cov = two["mass"][0], np.nan_to_num(two["log_mass_cov"][0]).reshape(12, 7, 12, 7)
    var = np.array([p[b] @ cov[b, :, b, :] @ p[b] for b in range(12)])
    px = one["mass"][0]
    err = np.abs(var / px ** 2 - (one["d_mass"][0] / px) ** 2).max()
    print("x marginal of the 12 x 7 cell covariance against the 1-D Var ln p: %.3e (bound %.3e)" % (err, bound))
    assert np.allclose(p.sum(axis=1), px, rtol=1e-12, atol=0) and err <= bound


# ------------------------------------------------------------------------------------------- 4. bitwise reproducibility
def test_two_calls_and_one_target_among_five_agree_bit_for_bit():
    for k, grid in ((33, "12x7"), (8, "25x25")):
        case = _case(k, grid, 5)
        args = _args(case)
        again = _joint_gram(*args)
        for a, b in zip(again[:6], case["dev"][:6]):
            assert _same(a, b)
        for t in (0, 3):
            alone = _joint_gram(*args[:4], case["targets"][t:t + 1], *args[5:])
            assert _bitwise(alone[0][0], case["dev"][0][t]) and _bitwise(alone[3][0], case["dev"][3][t]), (grid, t)
            assert _bitwise(alone[1], case["dev"][1])


def test_engine_form_equals_the_engine_less_form_bit_for_bit():
    """An 8 x 64-chain store with 33 records and 3 columns: columns (2, 0), then the energy on x (read as the energy, no value
    column), then the energy on y."""
    eng, temps, e, rungs, cols = _store_problem(8, 64, 33)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, 5)
    ex, ey, ee = np.linspace(1.0, 6.0, 13), np.linspace(-1.0, 4.5, 8), np.linspace(2.0, 30.0, 10)
    names = eng.recorded_observables
    for (wx, vx, gx), (wy, vy, gy) in (((names[2], cols[:, 2].ravel(), ex), (0, cols[:, 0].ravel(), ey)),
                                       (("energy", e.ravel(), ee), (names[0], cols[:, 0].ravel(), ey)),
                                       ((2, cols[:, 2].ravel(), ex), ("energy", e.ravel(), ee))):
        got = eng.free_energy_surface_uncertainties(wx, gx, wy, gy, targets, f)
        less = statistics.mbar_free_energy_surface_uncertainties(e, rungs, temps, f, targets, vx, gx, vy, gy)
        assert set(got) == set(less) | {"names"}
        for key in FLOAT_KEYS:
            assert _bitwise(got[key], less[key]), (wx, wy, key)
        for key in ("counts", "counts_slots", "lowest"):
            assert np.array_equal(got[key], less[key]), (wx, wy, key)
        assert got["n_samples"] == less["n_samples"] == e.size
        plain = eng.free_energy_surface(wx, gx, wy, gy, targets, f)
        for key in plain:
            assert _same(plain[key], got[key]) if key != "names" else plain[key] == got[key], key
    # "recorded": the largest g over the rungs and over the energy and both columns multiplies every variance
    g = eng.recorded_inefficiency()["g"]
    recorded = eng.free_energy_surface_uncertainties(2, ex, 0, ey, targets, f, inefficiency="recorded", covariance=False)
    scalar = eng.free_energy_surface_uncertainties(2, ex, 0, ey, targets, f, inefficiency=float(g[[0, 1, 3]].max()), covariance=False)
    assert "log_mass_cov" not in recorded
    for key in ("d_mass", "d_outside", "d_free_energy_from_lowest"):
        assert _bitwise(recorded[key], scalar[key]), key


def test_exchanging_the_axes_transposes_the_result():
    """counts exactly; d_mass to the algebra bound (the masses' normalising total, and with it H / p, runs over the cells in
    another order: rounding only), as Var ln p within 4 (route_bound + GRAM_BOUND) max |Theta|, the bound of
    test_uncertainties_against_the_reference."""
    case = _case(8, "4x3", 1)
    a = statistics.mbar_free_energy_surface_uncertainties(*_args(case))
    e, r, t, f, tg, x, ex, y, ey = _args(case)
    b = statistics.mbar_free_energy_surface_uncertainties(e, r, t, f, tg, y, ey, x, ex)
    assert np.array_equal(a["counts_slots"], b["counts_slots"].T)
    explicit, live = ref.explicit_weight_matrix(case["w"], 8, 0, ref.cells_of(x, ex, y, ey), case["mass"][0])
    cc = ref.column_counts(case["ladder_counts"], live.size)
    bound = 4.0 * (ref.route_bound(explicit, cc) + GRAM_BOUND) * np.abs(ref.theta_svd(explicit, cc)).max()
    p = a["mass_slots"][0]
    full = p > 0
    err = np.abs((a["d_mass_slots"][0][full] / p[full]) ** 2 - (b["d_mass_slots"][0].T[full] / p[full]) ** 2).max()
    print("axes exchanged: Var ln p %.3e (bound %.3e)" % (err, bound))
    assert np.array_equal(a["lowest"][0], b["lowest"][0][::-1]) and err <= bound


# ------------------------------------------------------------------------------------------------ 5. non-finite values
def test_non_finite_energies_are_left_out_and_nan_values_have_an_error_bar():
    """1 % of the energies +-inf or NaN, scattered: H against the long-double reference on the used samples, and against the
    device's H on the arrays without them within the two bounds added (taking samples out moves the others to other lanes and
    tiles, and the order of a cell's sum goes by the positions).  Where the used samples keep their positions -- the unused ones
    behind them, inside the last tile -- every output equals that of the arrays without them bit for bit."""
    case = _case(8, "4x3", 1)
    rng = np.random.default_rng(3)
    energies, x, y = case["energies"].copy(), case["x"].copy(), case["y"].copy()
    bad = rng.choice(energies.size, energies.size // 100, replace=False)
    energies[bad] = np.resize([np.inf, -np.inf, np.nan], bad.size)
    keep = np.isfinite(energies)
    x[bad[0]] = np.nan                                         # of an unused sample: never seen
    used = np.flatnonzero(keep)
    x[used[17]] = np.nan                                       # of used samples: the NaN slot of each axis
    y[used[29]] = np.nan
    args = (energies, case["rungs"], case["temps"], case["f"], case["targets"], x, case["ex"], y, case["ey"])
    h, ladder, cc, mass, counts, neff, n_used = _joint_gram(*args)
    h_ref, _, counts_ref, _, ladder_counts = ref.cell_gram(*args)
    err = _h_error(h, h_ref)
    bound = gram_bound(int(keep.sum()))
    print("1 %% non-finite energies: largest relative error of H on the used samples %.3e (bound %.3e)" % (err, bound))
    assert n_used == int(keep.sum()) == counts.sum() and np.array_equal(counts, counts_ref)
    assert np.array_equal(cc, np.asarray(ladder_counts, dtype=np.float64)) and err <= bound
    without = _joint_gram(energies[keep], case["rungs"][keep], case["temps"], case["f"], case["targets"], x[keep], case["ex"], y[keep],
                          case["ey"])
    seen = without[0] != 0
    assert np.array_equal(counts, without[4]) and np.array_equal(cc, without[2]) and np.all(h[~seen] == 0.0)
    moved = float((np.abs(h - without[0])[seen] / without[0][seen]).max())
    print("    against the arrays without them (other lanes and tiles): %.3e (bound %.3e)" % (moved, 2 * bound))
    assert moved <= 2 * bound
    # the unused samples behind the used ones, the tile count unchanged: the used samples keep lane, tile and block
    tail = 61
    assert -(-(N + tail) // 2048) == -(-N // 2048)
    e_tail = np.concatenate([case["energies"], np.resize([np.inf, -np.inf, np.nan], tail)])
    r_tail = np.concatenate([case["rungs"], np.resize(np.arange(8, dtype=np.int32), tail)])
    x_tail, y_tail = np.concatenate([case["x"], np.full(tail, np.nan)]), np.concatenate([case["y"], np.linspace(-1.0, 1.0, tail)])
    with_tail = _joint_gram(e_tail, r_tail, case["temps"], case["f"], case["targets"], x_tail, case["ex"], y_tail, case["ey"])
    for a, b in zip(with_tail, case["dev"]):
        assert _same(a, b)
    full = statistics.mbar_free_energy_surface_uncertainties(e_tail, r_tail, case["temps"], case["f"], case["targets"], x_tail,
                                                             case["ex"], y_tail, case["ey"])
    clean = statistics.mbar_free_energy_surface_uncertainties(*_args(case))
    for key in clean:
        assert _same(full[key], clean[key]), key
    out = statistics.mbar_free_energy_surface_uncertainties(*args)
    bx, by = case["ex"].size - 1, case["ey"].size - 1
    assert out["n_samples"] == int(keep.sum()) and out["counts_slots"][bx + 2].sum() == 1 and out["counts_slots"][:, by + 2].sum() == 1
    nan_x, nan_y = out["d_mass_slots"][0][bx + 2], out["d_mass_slots"][0][:, by + 2]
    print("    NaN on x: mass %.3e +- %.3e; NaN on y: mass %.3e +- %.3e"
          % (out["mass_slots"][0][bx + 2].sum(), nan_x.max(), out["mass_slots"][0][:, by + 2].sum(), nan_y.max()))
    assert np.isfinite(nan_x).all() and nan_x.max() > 0 and np.isfinite(nan_y).all() and nan_y.max() > 0
    assert np.all(np.isfinite(out["d_mass"])) and np.isfinite(out["d_outside"][0]) and out["d_outside"][0] > 0


def test_a_cold_target_whose_far_cells_underflow_keeps_every_other_error_bar():
    """The energy on x at T = 0.02 under a ladder that starts at 0.5: the weights of the upper cells are below 1e-154, so their
    squared sums (and further up the masses themselves) are 0 although the cells hold samples.  Such a cell has d_free_energy
    NaN and d_mass NaN (mass > 0) or 0 (mass exactly 0); every other cell has a finite error bar; and the second target's table
    is bit for bit what it is alone."""
    case = _case(8, "4x3", 1)
    e, r, t, f = case["energies"], case["rungs"], case["temps"], case["f"]
    ex, ey = np.linspace(0.0, 80.0, 21), ref.GRIDS["4x3"][1]
    targets = np.array([0.02, case["targets"][0]])
    out = statistics.mbar_free_energy_surface_uncertainties(e, r, t, f, targets, e, ex, case["y"], ey)
    h = _joint_gram(e, r, t, f, targets, e, ex, case["y"], ey)[0].reshape(2, 9, 23, 6)
    resolved = h[:, 8, :20, :3] >= np.finfo(np.float64).tiny
    p, counts = out["mass"], out["counts"]
    lost = ~resolved[0] & (counts > 0)
    print("T = 0.02: %d cells hold samples, %d of them without a resolved sum of squares (%d with mass exactly 0)"
          % (int((counts > 0).sum()), int(lost.sum()), int((lost & (p[0] == 0)).sum())))
    assert lost.sum() >= 4 and np.array_equal(resolved[1], counts > 0)
    assert np.all(np.isfinite(out["d_mass"][resolved])) and np.all(out["d_mass"][resolved] >= 0)
    assert np.all(out["d_mass"][1][resolved[1]] > 0)
    assert np.all(np.isfinite(out["d_free_energy"][resolved])) and np.all(np.isnan(out["d_free_energy"][~resolved]))
    assert np.all(np.isnan(out["d_mass"][~resolved & (p > 0)])) and np.all(out["d_mass"][~resolved & (p == 0)] == 0)
    assert np.array_equal(np.isfinite(out["free_energy"]), p > 0) and np.all(np.isfinite(out["d_outside"]))
    alone = statistics.mbar_free_energy_surface_uncertainties(e, r, t, f, targets[1:], e, ex, case["y"], ey)
    for key in ("mass_slots", "d_mass_slots", "d_free_energy", "log_mass_cov", "d_free_energy_from_lowest", "d_outside"):
        assert _bitwise(out[key][1], alone[key][0]), key


# ------------------------------------------------------------------------------------------------------ 6. lane patterns
def _nine_and_singles(rng):
    """9 lanes of every wavefront in one cell beside 55 lanes with cells of their own (8 x 8 bins, R = 8): one group beyond
    kDense = 8, summed by wave_sum, and one round of the rank loop."""
    lane = np.arange(CORNER) % 64
    edges = np.arange(9.0)
    cell = np.where(lane < 9, 0, lane - 8)
    return cell // 8 + 0.25 + 0.5 * rng.random(CORNER), edges, cell % 8 + 0.25 + 0.5 * rng.random(CORNER), edges


@pytest.mark.parametrize("pattern", ["one cell", "64 distinct on two diagonals", "9 and 55 singles", "groups of 9 and 8"])
def test_lane_patterns_through_the_gram_rows(pattern):
    """Lane patterns through slot_accumulate with GramRows, against the long-double reference as in (1): all 64 lanes of a
    wavefront in one cell; 64 distinct cells; 9 lanes in one cell beside 55 singles, which crosses kDense; and
    tests/test_gpu_mbar_surface.py's 9 lanes in one cell and 8 in another beside 47 singles, the two sides of kDense."""
    temps, e, rungs, _, _ = _flat_problem(8, CORNER, seed=31)
    rng = np.random.default_rng(41)
    x, ex, y, ey = _nine_and_singles(rng) if pattern == "9 and 55 singles" else _corner_values(pattern, rng)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 2)
    h, _, _, mass, counts, _, n_used = _joint_gram(e, rungs, temps, f, targets, x, ex, y, ey)
    h_ref, _, counts_ref, _, _ = ref.cell_gram(e, rungs, temps, f, targets, x, ex, y, ey)
    err, bound = _h_error(h, h_ref), gram_bound(CORNER)
    filled = int((counts > 0).sum())
    print("%s: largest relative error of H %.3e (bound %.3e); %d cells filled of %d" % (pattern, err, bound, filled, counts.size))
    assert n_used == CORNER and np.array_equal(counts, counts_ref)
    assert filled == {"one cell": 1, "64 distinct on two diagonals": 64, "9 and 55 singles": 56, "groups of 9 and 8": 49}[pattern]
    if pattern == "9 and 55 singles":
        cells = ref.cells_of(x, ex, y, ey)
        for w in range(CORNER // 64):
            sizes = sorted(np.bincount(cells[64 * w:64 * w + 64])[np.unique(cells[64 * w:64 * w + 64])].tolist())
            assert sizes == [1] * 55 + [9]
    assert err <= bound


# ------------------------------------------------------------------------------------------------------- 7. calibration
def test_calibration_on_the_device():
    """The subsets, grid and inclusion threshold of tests/test_mbar_surface_uncertainty_cpu.py through the GPU; the same
    condition on the RMS z-scores of every included cell (exact probability >= ref.CAL_MIN_PROBABILITY; no other exclusion)."""
    from test_mbar_surface_uncertainty_cpu import calibration_included
    ex, ey, targets = ref.CAL_EDGES_X, ref.CAL_EDGES_Y, oref.PHYSICS_TARGETS
    included, exact = calibration_included(targets)
    assert np.all(included.reshape(targets.size, -1).sum(axis=1) >= 12)
    z = []
    for e, rungs, cols in ref.calibration_subsets():
        f = statistics.mbar_free_energies(e, rungs, oref.LADDER8, tol=1e-12)["f"]
        out = statistics.mbar_free_energy_surface_uncertainties(e, rungs, oref.LADDER8, f, targets, cols[0], ex, cols[1], ey,
                                                                covariance=False)
        with np.errstate(divide="ignore", invalid="ignore"):
            z.append((out["mass_slots"][:, :6, :6] - exact) / out["d_mass_slots"][:, :6, :6])
    rms = np.sqrt((np.array(z)[:, included] ** 2).mean(axis=0))
    lo, hi = uref.CAL_RMS_Z
    print("rms z of the %d included cell masses on the device (per temperature %s): %.3f ... %.3f"
          % (rms.size, included.reshape(targets.size, -1).sum(axis=1), rms.min(), rms.max()))
    assert np.all(np.isfinite(rms)) and np.all((rms >= lo) & (rms <= hi))


# ------------------------------------------------------------------------------------------------------------ 8. errors
def _ptr(a):
    return _capi.double_ptr(np.ascontiguousarray(a, dtype=np.float64))


def test_error_cases():
    """Those of tests/test_gpu_mbar_surface.py's test_error_cases through the new entry points, the inefficiency and covariance."""
    eng, temps, e, rungs, cols = _store_problem(8, 64, 5)
    f = eng.ladder_free_energies()["f"]
    good = np.array([1.0, 2.0, 3.0])
    x, y = cols[:, 0].ravel().copy(), cols[:, 2].ravel().copy()
    host = lambda ex, ey, **kw: statistics.mbar_free_energy_surface_uncertainties(e, rungs, temps, f, [1.0], x, ex, y, ey, **kw)  # noqa: E731
    for edges in ([1.0, 2.0, 2.0], [1.0, 3.0, 2.0], [1.0, np.nan, 3.0], [1.0], np.arange(258.0)):
        for ex, ey in ((edges, good), (good, edges)):
            with pytest.raises(ValueError):
                eng.free_energy_surface_uncertainties("real_0", ex, "real_2", ey, [1.0], f)
            with pytest.raises(ValueError):
                host(ex, ey)
    with pytest.raises(ValueError, match="at most 1296 cells"):
        eng.free_energy_surface_uncertainties("real_0", np.arange(35.0), "real_2", np.arange(34.0), [1.0], f)
    with pytest.raises(ValueError, match="unknown recorded observable"):
        eng.free_energy_surface_uncertainties("real_0", good, "real_3", good, [1.0], f)
    with pytest.raises(ValueError, match="outside the 3 recorded columns"):
        eng.free_energy_surface_uncertainties(3, good, 0, good, [1.0], f)
    for bad in ([0.0], [1.0, -1.0], [np.nan], []):
        with pytest.raises(ValueError):
            eng.free_energy_surface_uncertainties("real_0", good, "real_2", good, bad, f)
    for bad in (0.99, -2.0, np.nan, np.inf, [1.0, 2.0], np.ones(3), "measured"):
        with pytest.raises(ValueError):
            eng.free_energy_surface_uncertainties("real_0", good, "real_2", good, [1.0], f, inefficiency=bad)
        if not isinstance(bad, str):
            with pytest.raises(ValueError):
                host(good, good, inefficiency=bad)
    for bad in (None, 1, "no"):
        with pytest.raises(ValueError, match="covariance must be True or False"):
            eng.free_energy_surface_uncertainties("real_0", good, "real_2", good, [1.0], f, covariance=bad)
    one = eng.free_energy_surface_uncertainties("real_2", np.linspace(1.0, 6.0, 6), "real_0", np.linspace(-1.0, 4.5, 5), [0.7, 1.9], f)
    four = eng.free_energy_surface_uncertainties("real_2", np.linspace(1.0, 6.0, 6), "real_0", np.linspace(-1.0, 4.5, 5), [0.7, 1.9], f,
                                                 inefficiency=4.0)
    for key in ("d_mass", "d_mass_slots", "d_outside", "d_free_energy", "d_free_energy_from_lowest"):
        assert np.array_equal(four[key], 2.0 * one[key], equal_nan=True), key
    assert np.array_equal(four["log_mass_cov"], 4.0 * one["log_mass_cov"], equal_nan=True) and _bitwise(four["mass"], one["mass"])
    # "recorded" needs a statistical inefficiency of every series it names: a column without variance has none
    flat = cols.copy()
    flat[:, 1] = 0.25
    eng.set_observable_samples(flat)
    assert np.all(np.isnan(eng.recorded_inefficiency()["g"][2]))
    with pytest.raises(ValueError, match="recorded"):
        eng.free_energy_surface_uncertainties("real_1", good, "real_2", good, [1.0], f, inefficiency="recorded")
    with pytest.raises(ValueError, match="recorded"):
        eng.free_energy_surface_uncertainties("energy", good, 1, good, [1.0], f, inefficiency="recorded")
    assert eng.free_energy_surface_uncertainties("real_0", good, "energy", good, [1.0], f, inefficiency="recorded")["n_samples"] == e.size
    eng.set_observable_samples(cols)
    # the same through the C ABI
    lib, h = eng._lib, eng._handle
    fp, tp = _ptr(f), _ptr([1.0])

    def call(cx, ex, bx, cy, ey, by, temps_ptr=tp):
        return lib.me_mbar_histogram_joint_gram(h, fp, temps_ptr, 1, cx, _ptr(ex), bx, cy, _ptr(ey), by, None, None, None, None, None,
                                                None, None)

    assert call(1, good, 2, 2, good, 2) == _capi.ME_OK            # every output may be null
    assert call(-1, good, 2, 2, good, 2) == _capi.ME_OK and call(1, good, 2, -1, good, 2) == _capi.ME_OK
    assert call(-1, good, 2, -1, good, 2) == _capi.ME_OK and call(1, good, 2, 1, good, 2) == _capi.ME_OK
    for bad, n_bins in (([1.0, 2.0, 2.0], 2), ([1.0, 3.0, 2.0], 2), ([1.0, np.nan, 3.0], 2), ([1.0, np.inf], 1), (good, 0),
                        (np.arange(258.0), 257)):
        assert call(1, bad, n_bins, 2, good, 2) == _capi.ME_ERR_INVALID, (bad, n_bins)
        assert call(1, good, 2, 2, bad, n_bins) == _capi.ME_ERR_INVALID, (bad, n_bins)
    assert call(1, np.arange(257.0), 256, 2, good, 2) == _capi.ME_OK               # 259 x 5 = 1295 cells
    assert call(1, np.arange(257.0), 256, 2, np.arange(4.0), 3) == _capi.ME_ERR_INVALID    # 259 x 6 cells
    assert call(1, np.arange(34.0), 33, 2, np.arange(34.0), 33) == _capi.ME_OK             # 36 x 36 = 1296 cells
    assert call(1, np.arange(35.0), 34, 2, np.arange(34.0), 33) == _capi.ME_ERR_INVALID
    assert "1296" in _capi.last_error(h)
    for column in (3, -2):                                        # column index >= recorded columns; neither recorded nor -1
        assert call(column, good, 2, 1, good, 2) == _capi.ME_ERR_INVALID and call(1, good, 2, column, good, 2) == _capi.ME_ERR_INVALID
    assert call(1, good, 2, 2, good, 2, _ptr([0.0])) == _capi.ME_ERR_INVALID       # temperature <= 0
    assert call(1, good, 2, 2, good, 2, _ptr([-1.0])) == _capi.ME_ERR_INVALID
    assert lib.me_mbar_histogram_joint_gram(h, None, tp, 1, 1, _ptr(good), 2, 2, _ptr(good), 2, None, None, None, None, None, None,
                                            None) == _capi.ME_ERR_INVALID          # f missing
    assert lib.me_mbar_histogram_joint_gram(h, fp, tp, 1, 1, None, 2, 2, _ptr(good), 2, None, None, None, None, None, None,
                                            None) == _capi.ME_ERR_INVALID          # edges missing
    r32 = np.ascontiguousarray(rungs, dtype=np.int32)

    def less(ex, bx, ey, by, vx=_capi.double_ptr(x), vy=_capi.double_ptr(y)):
        return lib.me_mbar_histogram_joint_gram_samples(0, _ptr(e), _capi.int32_ptr(r32), e.size, _ptr(temps), 8, fp, tp, 1, vx, vy,
                                                        _ptr(ex), bx, _ptr(ey), by, None, None, None, None, None, None, None)

    assert less(good, 2, good, 2) == _capi.ME_OK
    assert less(good, 2, good, 2, vx=None) == _capi.ME_ERR_INVALID and less(good, 2, good, 2, vy=None) == _capi.ME_ERR_INVALID
    assert less([1.0, 1.0, 3.0], 2, good, 2) == _capi.ME_ERR_INVALID and less(good, 2, good, 0) == _capi.ME_ERR_INVALID
    assert less(good, 2, np.arange(258.0), 257) == _capi.ME_ERR_INVALID
    assert less(np.arange(34.0), 33, np.arange(34.0), 33) == _capi.ME_OK
    assert less(np.arange(34.0), 33, np.arange(35.0), 34) == _capi.ME_ERR_INVALID
    # more than 64 rungs: the Python layer refuses (ValueError), the C ABI as me_mbar_histogram_joint_samples does
    temps65 = np.linspace(0.5, 3.0, 65)
    r65 = (np.arange(e.size) % 65).astype(np.int32)
    with pytest.raises(ValueError):
        statistics.mbar_free_energy_surface_uncertainties(e, r65, temps65, np.zeros(65), [1.0], x, good, y, good)
    f65 = _ptr(np.zeros(65))
    old = lib.me_mbar_histogram_joint_samples(0, _ptr(e), _capi.int32_ptr(r65), e.size, _ptr(temps65), 65, f65, tp, 1, _capi.double_ptr(x),
                                              _capi.double_ptr(y), _ptr(good), 2, _ptr(good), 2, None, None, None)
    new = lib.me_mbar_histogram_joint_gram_samples(0, _ptr(e), _capi.int32_ptr(r65), e.size, _ptr(temps65), 65, f65, tp, 1,
                                                   _capi.double_ptr(x), _capi.double_ptr(y), _ptr(good), 2, _ptr(good), 2, None, None,
                                                   None, None, None, None, None)
    assert old == new != _capi.ME_OK
    eng.record_observables(None)                                  # no observable store
    assert call(0, good, 2, -1, good, 2) == _capi.ME_ERR_STATE and call(-1, good, 2, 0, good, 2) == _capi.ME_ERR_STATE
    assert call(-1, good, 2, -1, good, 2) == _capi.ME_OK          # ... which the energy does not need
    with pytest.raises(ValueError, match="no observable store"):
        eng.free_energy_surface_uncertainties(0, good, "energy", good, [1.0], f)
    eng.record_energies(0)                                        # no energy store
    assert call(-1, good, 2, -1, good, 2) == _capi.ME_ERR_STATE
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples"):
        eng.free_energy_surface_uncertainties("energy", good, "energy", good, [1.0], f)
    # a scalar-temp engine without a ladder: as free_energy_surface
    scalar = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=128, temp=1.0)
    scalar.record_energies(2)
    scalar.record_observables(["real_0"])
    scalar.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
        scalar.free_energy_surface_uncertainties("real_0", good, "energy", good, [1.0], f=[0.0])


# -------------------------------------------------------------------------------------------------------- 9. end to end
def test_valley_well_saddle_height_lies_within_its_error_bar():
    """The demo's two-parameter double well, 8 rungs x 256 chains, 16 records: at the coldest demo temperature the saddle height
    F(saddle) - F(right well) minus the quadrature's lies within 4 of its own "recorded" standard errors, taken from
    log_mass_cov; where the right well is the lowest cell, d_free_energy_from_lowest gives the same error."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import demo_free_energy_surface as demo
    finally:
        sys.path.pop(0)
    eng = demo.sample(**demo.QUICK)
    f = eng.ladder_free_energies()["f"]
    out = eng.free_energy_surface_uncertainties("real_0", demo.EDGES_X, "real_1", demo.EDGES_Y, demo.TEMPS, f, inefficiency="recorded")
    plain = eng.free_energy_surface("real_0", demo.EDGES_X, "real_1", demo.EDGES_Y, demo.TEMPS, f)
    for key in plain:
        assert _same(plain[key], out[key]) if key != "names" else plain[key] == out[key], key
    seen = out["counts"] > 0
    assert np.all(np.isfinite(out["d_free_energy"][1:, seen])) and np.all(np.isnan(out["d_free_energy"][:, ~seen]))
    assert out["n_samples"] == eng.energy_samples().size
    height, error, saddle, well = demo.saddle_height(out, 0)
    exact = demo.quadrature(out["edges_x"], out["edges_y"], float(demo.TEMPS[0]))
    want = exact[saddle] - exact[well]
    print("T = %.2f: F(saddle) - F(right well) = %.4f +- %.4f (recorded inefficiency); quadrature %.4f; %.2f standard errors"
          % (demo.TEMPS[0], height, error, want, (height - want) / error))
    assert np.isfinite(error) and 0.0 < error < height
    if tuple(out["lowest"][0]) == well:
        assert abs(error - out["d_free_energy_from_lowest"][0][saddle]) <= 1e-9 * error
    assert abs(height - want) <= 4.0 * error


def test_the_demo_prints_the_saddle_height_with_its_error():
    run = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "examples", "demo_free_energy_surface.py"),
                          "--quick"], cwd=ROOT, capture_output=True, text=True)
    print(run.stdout[-1500:], run.stderr[-2000:])
    assert run.returncode == 0
    lines = run.stdout.strip().splitlines()
    assert "+-" in lines[-1] and "exact" in lines[-1] and "standard errors" in lines[-1]
