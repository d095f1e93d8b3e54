"""numpy restatement of the cell Gram sums behind the error bars of a joint reweighted histogram (csrc/me_mbar_hist2d_cov.hip
has the definitions), of the explicit weight matrix [K ladder | state | one column per live cell] and of what is derived from
its Theta.  Everything up to the weight matrix is ``np.longdouble``: the ladder and state columns are those of
tests/mbar_uncertainty_reference.py, the slots of an axis those of tests/mbar_profile_reference.py, both imported.  Also the
shared inputs of tests/test_mbar_surface_uncertainty_cpu.py and tests/test_gpu_mbar_surface_uncertainty.py."""
import numpy as np

from mbar_uncertainty_reference import LD, N_GRAM, route_bound, synthetic, targets_for, theta_gram, theta_svd, weight_matrix  # noqa: F401
from mbar_profile_reference import slots
from mbar_profile_uncertainty_reference import column_counts, log_covariance, difference_variances, synthetic_values  # noqa: F401


def cells_of(values_x, edges_x, values_y, edges_y):
    """The cell ``slot_x (By + 3) + slot_y`` of every sample."""
    return slots(np.asarray(values_x, dtype=np.float64).ravel(), edges_x) * (len(edges_y) + 2) + \
        slots(np.asarray(values_y, dtype=np.float64).ravel(), edges_y)


def cell_gram(energies, rungs, temps, f, targets, values_x, edges_x, values_y, edges_y):
    """``(H (T, K + 1, S), mass (T, S), counts (S,), w, ladder_counts)``, ``S = (Bx + 3)(By + 3)``: ``H[t][j][c]`` the sum over
    the used samples of cell c of ``W_nj w_nt`` (``j < K``) and of ``w_nt^2`` (``j = K``), the masses, the used samples per
    cell, and the long-double weight matrix of ``mbar_uncertainty_reference.weight_matrix`` that all of it was taken from
    (ladder column k at k, the state column of target t at ``K + 2 t``) with its ladder counts."""
    targets = np.atleast_1d(np.asarray(targets, dtype=np.float64))
    k, s = np.asarray(temps).size, (len(edges_x) + 2) * (len(edges_y) + 2)
    w, counts, _, _, _ = weight_matrix(energies, rungs, temps, f, targets)
    used = np.isfinite(np.asarray(energies, dtype=np.float64).ravel())
    cell = cells_of(np.asarray(values_x, dtype=np.float64).ravel()[used], edges_x,
                    np.asarray(values_y, dtype=np.float64).ravel()[used], edges_y)
    h = np.zeros((targets.size, k + 1, s), dtype=LD)
    mass = np.zeros((targets.size, s), dtype=LD)
    order = np.argsort(cell, kind="stable")
    seen, starts = np.unique(cell[order], return_index=True)
    ends = np.append(starts[1:], cell.size)
    for t in range(targets.size):
        state = w[:, k + 2 * t]
        for c, lo, hi in zip(seen, starts, ends):
            rows = order[lo:hi]
            h[t, :k, c] = (w[rows, :k] * state[rows, None]).sum(axis=0)
            h[t, k, c] = (state[rows] * state[rows]).sum()
            mass[t, c] = state[rows].sum()
        mass[t] /= state.sum()
    return h, mass, np.bincount(cell, minlength=s).astype(np.int64), w, counts[:k]


def explicit_weight_matrix(w, k, t, cell_used, mass_t):
    """``[w[:, :K] | state of target t | state 1[cell = c] / mass_t[c] for every cell with mass_t[c] > 0]`` and the live cells."""
    state = w[:, k + 2 * t]
    live = np.flatnonzero(np.asarray(mass_t) > 0)
    cols = [w[:, j] for j in range(k)] + [state] + [np.where(cell_used == c, state, LD(0)) / mass_t[c] for c in live]
    return np.stack(cols, axis=1), live


def derived(theta, k, live, mass_t, temp, edges_x, edges_y):
    """The entries of ``mbar_free_energy_surface_uncertainties`` at one temperature from Theta over [K | state | live cells], with
    the library's conventions for an empty cell: ``{"d_slots" (Bx + 3, By + 3), "d_outside", "d_free_energy" (Bx, By),
    "log_mass_cov" (Bx By, Bx By), "d_free_energy_from_lowest" (Bx, By), "lowest" (2,), "var_outside"}``."""
    bx, by = len(edges_x) - 1, len(edges_y) - 1
    s = (bx + 3) * (by + 3)
    p = np.asarray(mass_t, dtype=np.float64)
    cov, _ = log_covariance(theta, k)
    var = np.clip(np.diag(cov), 0.0, None)
    d_slots = np.zeros(s)
    d_slots[live] = p[live] * np.sqrt(var)
    inner = np.zeros((bx + 3, by + 3), dtype=bool)
    inner[:bx, :by] = True
    inner = inner.ravel()
    to_inner = np.full(s, -1)
    to_inner[inner] = np.arange(bx * by)
    bins = inner[live]
    own = to_inner[live[bins]]
    d_free, d_low, log_cov = np.full(bx * by, np.nan), np.full(bx * by, np.nan), np.full((bx * by, bx * by), np.nan)
    d_free[own] = temp * np.sqrt(var[bins])
    log_cov[np.ix_(own, own)] = cov[np.ix_(bins, bins)]
    widths = np.diff(np.asarray(edges_x, dtype=np.float64))[:, None] * np.diff(np.asarray(edges_y, dtype=np.float64))[None, :]
    density = p.reshape(bx + 3, by + 3)[:bx, :by] / widths
    lowest = np.unravel_index(int(np.argmax(density)), (bx, by))
    at = int(np.flatnonzero(live == lowest[0] * (by + 3) + lowest[1])[0])
    d_low[own] = temp * np.sqrt(np.clip(difference_variances(theta, k, at)[bins], 0.0, None))
    d_low[lowest[0] * by + lowest[1]] = 0.0
    po = p[live][~bins]
    var_outside = float(po @ cov[np.ix_(~bins, ~bins)] @ po)
    return {"d_slots": d_slots.reshape(bx + 3, by + 3), "d_outside": np.sqrt(max(var_outside, 0.0)), "var_outside": var_outside,
            "d_free_energy": d_free.reshape(bx, by), "log_mass_cov": log_cov, "d_free_energy_from_lowest": d_low.reshape(bx, by),
            "lowest": np.array(lowest)}


# ---- shared inputs ----------------------------------------------------------------------------------------------------
def synthetic_values_y(energies, values_x, seed=41):
    """A second value column, built as ``synthetic_values`` is and correlated with the first: a fixed-seed standard normal, half
    of the first column and a part that follows the energy, centred."""
    e = np.asarray(energies, dtype=np.float64)
    z = np.random.default_rng(seed).standard_normal(e.size)
    return 0.8 * z + 0.5 * np.asarray(values_x) - 0.05 * (e - e.mean())


UNEVEN12 = np.array([-2.5, -1.9, -1.6, -1.0, -0.7, -0.55, -0.1, 0.0, 0.4, 0.45, 1.1, 1.8, 2.6])
UNEVEN7 = np.array([-2.2, -1.3, -0.6, -0.2, 0.3, 0.35, 1.2, 2.4])
# name -> (edges_x, edges_y); S cells and the R of csrc/me_mbar_hist2d_cov.hip's rule (16 to 106 cells, 8 to 211, 4 to 420, 2 to
# 827, then 1)
GRIDS = {
    "4x3": (np.linspace(-2.0, 2.0, 5), np.linspace(-1.5, 1.5, 4)),              # 42 cells, R = 16
    "12x7": (UNEVEN12, UNEVEN7),                                                # 150 cells, R = 8
    "17x17": (np.linspace(-3.0, 3.0, 18), np.linspace(-3.0, 3.0, 18)),          # 400 cells, R = 4
    "25x25": (np.linspace(-3.5, 3.5, 26), np.linspace(-3.5, 3.5, 26)),          # 784 cells, R = 2
    "26x26": (np.linspace(-3.5, 3.5, 27), np.linspace(-3.5, 3.5, 27)),          # 841 cells, R = 1 (just past the threshold)
    "33x33": (np.linspace(-6.0, 6.0, 34), np.linspace(-6.0, 6.0, 34)),          # 1296 cells, the cap, R = 1; outer bins empty
    "13x9": (np.linspace(-3.0, 3.0, 14), np.linspace(-2.5, 2.5, 10)),
    "7x5": (np.linspace(-1.0, 1.0, 8), np.linspace(-0.8, 0.8, 6)),              # most of the mass in the outer cells
}
ROWS = {"4x3": 16, "12x7": 8, "17x17": 4, "25x25": 2, "26x26": 1, "33x33": 1}


def rule_rows(n_cells):
    """csrc/me_mbar_hist2d_cov.hip's rows per pass, restated: the widest of 16, 8, 4, 2, 1 whose table, at most ``(32 R + 2) S``
    bytes, leaves three workgroups within the 160 KiB of a CU."""
    for rows in (16, 8, 4, 2):
        if n_cells <= (160 * 1024 // 3) // (32 * rows + 2):
            return rows
    return 1


# calibration: the grid and the threshold on the EXACT probability of a cell (chosen on the CPU with the long-double reference,
# tests/test_mbar_surface_uncertainty_cpu.py: the reference alone meets CAL_RMS_Z for every included cell)
CAL_EDGES_X = np.linspace(-1.5, 1.5, 5)
CAL_EDGES_Y = np.array([-1.2, -0.3, 0.2, 0.9, 1.6])
CAL_MIN_PROBABILITY = 0.01


def calibration_subsets():
    """The 64 subsets of 8 x 512 exact samples of E = |x|^2 on LADDER8 with the columns x_0 and x_1."""
    from mbar_surface_reference import xy_quadratic_subsets
    return xy_quadratic_subsets(n_subsets=64, per_rung=512)
