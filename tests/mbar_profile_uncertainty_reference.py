"""numpy restatement of the slot Gram sums behind the error bars of a reweighted histogram (csrc/me_mbar_hist_cov.hip has the
definitions), of the block assembly of the Gram matrix [K ladder | state | one column per live slot] and of what is derived
from its Theta.  Everything up to the Gram matrix is ``np.longdouble``: the ladder and state columns are those of
tests/mbar_uncertainty_reference.py, the slots those of tests/mbar_profile_reference.py, both imported.  Also the shared inputs
of tests/test_mbar_profile_uncertainty_cpu.py and tests/test_gpu_mbar_profile_uncertainty.py."""
import numpy as np

from mbar_uncertainty_reference import LD, N_GRAM, gram, route_bound, synthetic, targets_for, theta_gram, theta_svd, weight_matrix  # noqa: F401
from mbar_profile_reference import slots


def slot_gram(energies, rungs, temps, f, targets, values, edges):
    """``(H (T, K + 1, B + 3), mass (T, B + 3), counts (B + 3,), w, ladder_counts)``: ``H[t][j][s]`` the sum over the used
    samples of slot s of ``W_nj w_nt`` (``j < K``) and of ``w_nt^2`` (``j = K``), the masses ``sum_{slot} w_nt / sum w_nt``,
    the used samples per slot, and the long-double weight matrix ``w`` of ``mbar_uncertainty_reference.weight_matrix`` that all
    of it was taken from (ladder column k at k, the state column of target t at ``K + 2 t``) with its ladder counts."""
    targets = np.atleast_1d(np.asarray(targets, dtype=np.float64))
    k, b = np.asarray(temps).size, len(edges) - 1
    w, counts, _, _, _ = weight_matrix(energies, rungs, temps, f, targets)
    used = np.isfinite(np.asarray(energies, dtype=np.float64).ravel())
    slot = slots(np.asarray(values, dtype=np.float64).ravel()[used], edges)
    h = np.zeros((targets.size, k + 1, b + 3), dtype=LD)
    mass = np.zeros((targets.size, b + 3), dtype=LD)
    for t in range(targets.size):
        state = w[:, k + 2 * t]
        for s in np.unique(slot):
            rows = slot == s
            h[t, :k, s] = (w[rows, :k] * state[rows, None]).sum(axis=0)
            h[t, k, s] = (state[rows] * state[rows]).sum()
            mass[t, s] = state[rows].sum()
        mass[t] /= state.sum()
    return h, mass, np.bincount(slot, minlength=b + 3).astype(np.int64), w, counts[:k]


def explicit_weight_matrix(w, k, t, values_used, edges, mass_t):
    """The weight matrix whose Gram matrix :func:`block_gram` assembles, formed column by column: ``[w[:, :K] | state of target
    t | state 1[slot = s] / mass_t[s] for every slot with mass_t[s] > 0]``, and the live slots."""
    slot = slots(values_used, edges)
    state = w[:, k + 2 * t]
    live = np.flatnonzero(np.asarray(mass_t) > 0)
    cols = [w[:, j] for j in range(k)] + [state] + [np.where(slot == s, state, LD(0)) / mass_t[s] for s in live]
    return np.stack(cols, axis=1), live


def block_gram(h_t, mass_t, ladder_gram):
    """``(G, live)`` over the columns [K ladder | state | one per slot of mass > 0] from the slot Gram sums of one temperature,
    the masses and the ladder block; in the dtype of ``h_t``."""
    k = ladder_gram.shape[0]
    live = np.flatnonzero(np.asarray(mass_t) > 0)
    c = k + 1 + live.size
    g = np.zeros((c, c), dtype=h_t.dtype)
    g[:k, :k] = ladder_gram
    g[:k, k] = g[k, :k] = h_t[:k].sum(axis=1)
    g[k, k] = h_t[k].sum()
    g[:k + 1, k + 1:] = h_t[:, live] / mass_t[live][None, :]
    g[k + 1:, :k + 1] = g[:k + 1, k + 1:].T
    at = k + 1 + np.arange(live.size)
    g[at, at] = h_t[k, live] / mass_t[live] ** 2
    return g, live


def column_counts(ladder_counts, n_live):
    return np.concatenate([np.asarray(ladder_counts, dtype=np.float64), np.zeros(1 + n_live)])


def log_covariance(theta, k):
    """``(Cov(ln p_s, ln p_s') over the live slots, scale)`` without a clamp: ``Theta_ss' + Theta_aa - Theta_sa - Theta_s'a``
    with ``a = K`` the state column.  Every entry is a sum of four entries of Theta with coefficients of magnitude 1, so two
    Thetas that differ by ``b max |Theta|`` entrywise give entries within ``4 b scale`` of each other, ``scale = max |Theta|``
    (the rule of ``mbar_uncertainty_reference.variances``)."""
    theta = np.asarray(theta, dtype=np.float64)
    to_state = theta[k + 1:, k]
    return theta[k + 1:, k + 1:] + theta[k, k] - to_state[:, None] - to_state[None, :], np.abs(theta).max()


def difference_variances(theta, k, at):
    """``Var(ln p_s - ln p_at)`` over the live slots (``at`` an index into them): ``Theta_ss + Theta_at,at - 2 Theta_s,at``, four
    entries of Theta again."""
    block = np.asarray(theta, dtype=np.float64)[k + 1:, k + 1:]
    return np.diag(block) + block[at, at] - 2.0 * block[:, at]


def derived(theta, k, live, mass_t, temp, edges):
    """The entries of ``mbar_free_energy_profile_uncertainties`` at one temperature from Theta over [K | state | live slots],
    with the library's conventions for an empty slot: ``{"d_slots" (B + 3,), "d_free_energy" (B,), "log_mass_cov" (B, B),
    "d_free_energy_from_lowest" (B,), "lowest"}``."""
    b = len(edges) - 1
    p = np.asarray(mass_t, dtype=np.float64)
    cov, _ = log_covariance(theta, k)
    var = np.clip(np.diag(cov), 0.0, None)
    d_slots = np.zeros(b + 3)
    d_slots[live] = p[live] * np.sqrt(var)
    bins = live < b
    own = live[bins]
    d_free, d_low, log_cov = np.full(b, np.nan), np.full(b, np.nan), np.full((b, b), np.nan)
    d_free[own] = temp * np.sqrt(var[bins])
    log_cov[np.ix_(own, own)] = cov[np.ix_(bins, bins)]
    lowest = int(np.argmax(p[:b] / np.diff(np.asarray(edges, dtype=np.float64))))
    at = int(np.searchsorted(own, lowest))
    d_low[own] = temp * np.sqrt(np.clip(difference_variances(theta, k, at)[bins], 0.0, None))
    d_low[lowest] = 0.0
    return {"d_slots": d_slots, "d_free_energy": d_free, "log_mass_cov": log_cov, "d_free_energy_from_lowest": d_low,
            "lowest": lowest}


# ---- shared inputs ----------------------------------------------------------------------------------------------------
def uneven_edges():
    """12 bins of unequal width over the bulk of ``synthetic_values``."""
    return np.array([-2.5, -1.9, -1.6, -1.0, -0.7, -0.55, -0.1, 0.0, 0.4, 0.45, 1.1, 1.8, 2.6])


def fine_edges(n_bins=256):
    """``n_bins`` equal bins over [-6, 6]: with 6149 standard normals the outer ones stay empty."""
    return np.linspace(-6.0, 6.0, n_bins + 1)


def synthetic_values(energies, temps, rungs, seed=37):
    """One value per sample of ``mbar_uncertainty_reference.synthetic``: a fixed-seed standard normal plus a part that follows
    the energy (so that the histogram moves with the temperature), centred."""
    e = np.asarray(energies, dtype=np.float64)
    z = np.random.default_rng(seed).standard_normal(e.size)
    return z + 0.08 * (e - e.mean())


# (K, bins): the four cases of the block assembly against the explicit weight matrix
ASSEMBLY_CASES = [(8, "uneven"), (8, "fine"), (33, "uneven"), (64, "even64")]


def edges_of(name):
    return {"uneven": uneven_edges(), "fine": fine_edges(256), "even64": fine_edges(64), "even100": np.linspace(-3.0, 3.0, 101)}[name]
