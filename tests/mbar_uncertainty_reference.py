"""numpy restatement of the MBAR weight matrix and of its asymptotic covariance (csrc/me_mbar_cov.hip has the definitions;
Shirts & Chodera, J. Chem. Phys. 129:124105, 2008, eqs. 8, 12-15, D8).  W is built in ``np.longdouble`` straight from the
definitions; the Gram matrix is returned in long double, Theta by the Gram route (eigendecomposition of G) and by the SVD
route of eq. D8 applied to W itself, both in float64 (numpy has no long-double decompositions).  Also the shared inputs of
tests/test_mbar_uncertainty_cpu.py and tests/test_gpu_mbar_uncertainty.py."""
import numpy as np

LD = np.longdouble
RCOND = 1e-10
DIM = 16


def weight_matrix(energies, rungs, temps, f, targets=()):
    """``(W, counts, ln_z, mean_e, shift)`` in long double over the samples with a finite energy.  Columns: rung k at k, the
    state and the energy column of target t at K + 2 t and K + 2 t + 1."""
    e64 = np.asarray(energies, dtype=np.float64).ravel()
    used = np.isfinite(e64)
    e = e64[used].astype(LD)
    r = np.asarray(rungs).ravel()[used]
    t = np.asarray(temps, dtype=np.float64).astype(LD)
    f = np.asarray(f, dtype=np.float64).astype(LD)
    k = t.size
    n_k = np.bincount(r, minlength=k).astype(LD)
    a = (np.log(n_k) + f)[None, :] - e[:, None] / t[None, :]
    m = a.max(axis=1)
    d = m + np.log(np.exp(a - m[:, None]).sum(axis=1))
    cols = [np.exp(f[j] - e / t[j] - d) for j in range(k)]
    counts = list(n_k)
    shift = e.min() - LD(1)
    ln_z, mean_e = [], []
    for target in np.asarray(targets, dtype=np.float64).astype(LD):
        l = -e / target - d
        lz = l.max() + np.log(np.exp(l - l.max()).sum())
        w = np.exp(l - lz)
        mean_t = (w * (e - shift)).sum()
        cols += [w, w * (e - shift) / mean_t]
        counts += [LD(0), LD(0)]
        ln_z.append(lz)
        mean_e.append((w * e).sum())
    return np.stack(cols, axis=1), np.array(counts, dtype=LD), np.array(ln_z, dtype=LD), np.array(mean_e, dtype=LD), shift


def gram(w):
    """``W^T W`` in long double."""
    return w.T @ w


def theta_gram(g, counts):
    """Theta from G: G = V diag(lam) V^T, lam clamped at 0, S = sqrt(lam), Theta = V S (I - S V^T N V S)^+ S V^T."""
    lam, v = np.linalg.eigh(np.asarray(g, dtype=np.float64))
    s = np.sqrt(np.clip(lam, 0.0, None))
    n = np.asarray(counts, dtype=np.float64)
    m = np.eye(s.size) - s[:, None] * (v.T @ (n[:, None] * v)) * s[None, :]
    return (v * s[None, :]) @ np.linalg.pinv(m, rcond=RCOND) @ (v * s[None, :]).T


def theta_svd(w, counts):
    """Theta by eq. D8: W = U S V^T, Theta = V S (I - S V^T N V S)^+ S V^T."""
    _, s, vt = np.linalg.svd(np.asarray(w, dtype=np.float64), full_matrices=False)
    n = np.asarray(counts, dtype=np.float64)
    m = np.eye(s.size) - s[:, None] * (vt @ (n[:, None] * vt.T)) * s[None, :]
    return (vt.T * s[None, :]) @ np.linalg.pinv(m, rcond=RCOND) @ (vt.T * s[None, :]).T


def route_bound(w, counts):
    """Largest |Theta_a - Theta_b| / max |Theta| to expect between two float64 routes to Theta = B M^+ B^T, M = I - B^T N B,
    B B^T = G.  Each route takes about 8 float64 steps over C x C matrices (the decomposition, the scaling by S, two
    products for M, the decomposition inside the pseudo-inverse, three products for Theta), each backward stable with an error
    of at most C 2^-53 in norm relative to its operands, and ||B^T N B|| <= 1.  M has one zero eigenvalue (sum_j N_j G_ij =
    1) that rcond removes in both routes; for pseudo-inverses of equal rank a perturbation dM moves M^+ by at most
    3 ||M^+||^2 ||dM|| (Wedin), and ||M^+|| = 1 / mu with mu the smallest eigenvalue of M above the cut, so Theta moves by
    3 * 8 C 2^-53 / mu relative to ||B||^2 / mu, its own size.  Two routes: 2 * 24 = 48, rounded up to 64 C 2^-53 / mu.  The
    small eigenvalues of G do not enter: a direction of eigenvalue lam carries lam, not 1 / lam, into Theta."""
    _, s, vt = np.linalg.svd(np.asarray(w, dtype=np.float64), full_matrices=False)
    n = np.asarray(counts, dtype=np.float64)
    mu = np.linalg.eigvalsh(np.eye(s.size) - s[:, None] * (vt @ (n[:, None] * vt.T)) * s[None, :])
    mu = mu[mu > RCOND * mu.max()].min()
    return 64.0 * s.size * 2.0 ** -53 / mu


def variances(theta, k, n_targets, mean_e, shift):
    """The squares of :func:`sigmas` without the clamp at 0, and for each the largest |Theta| entry times the square of the
    factor in front: ``((var_f_matrix, var_ln_z, var_energy_mean), (scale_f, scale_ln_z, scale_energy_mean))``.  Every
    variance is a sum of four entries of Theta with coefficients of magnitude 1, so two Thetas that differ by ``b max
    |Theta|`` entrywise give variances within ``4 b scale`` of each other."""
    diag = np.diag(theta)
    a = k + 2 * np.arange(n_targets)
    mean_t = np.asarray(mean_e, dtype=np.float64) - float(shift)
    top = np.abs(theta).max()
    return ((diag[:k, None] + diag[None, :k] - 2.0 * theta[:k, :k], theta[a, a] + theta[0, 0] - 2.0 * theta[a, 0],
             mean_t ** 2 * (theta[a + 1, a + 1] + theta[a, a] - 2.0 * theta[a + 1, a])), (top, top, top * mean_t ** 2))


def sigmas(theta, k, n_targets, mean_e, shift):
    """``(d_f, d_f_matrix, d_ln_z, d_energy_mean)`` from Theta over the K + 2 n_targets columns."""
    diag = np.diag(theta)
    var = diag[:k, None] + diag[None, :k] - 2.0 * theta[:k, :k]
    d_f_matrix = np.sqrt(np.clip(var, 0.0, None))
    np.fill_diagonal(d_f_matrix, 0.0)
    a = k + 2 * np.arange(n_targets)
    d_ln_z = np.sqrt(np.clip(theta[a, a] + theta[0, 0] - 2.0 * theta[a, 0], 0.0, None))
    mean_t = np.asarray(mean_e, dtype=np.float64) - float(shift)
    d_mean = mean_t * np.sqrt(np.clip(theta[a + 1, a + 1] + theta[a, a] - 2.0 * theta[a + 1, a], 0.0, None))
    return d_f_matrix[:, 0].copy(), d_f_matrix, d_ln_z, d_mean


def solve(energies, rungs, temps, tol=1e-12, max_iter=20000):
    """The self-consistent iteration of tests/mbar_reference.py in plain float64 numpy (finite energies only)."""
    e = np.asarray(energies, dtype=np.float64)
    t = np.asarray(temps, dtype=np.float64)
    n = np.bincount(rungs, minlength=t.size).astype(np.float64)
    f = np.zeros(t.size)
    for _ in range(max_iter):
        a = (np.log(n) + f)[None, :] - e[:, None] / t[None, :]
        ex = np.exp(a - a.max(axis=1, keepdims=True))
        s_k = (ex / ex.sum(axis=1, keepdims=True)).sum(axis=0)
        f_new = f - np.log(s_k / n)
        f_new -= f_new[0]
        change = np.abs(f_new - f).max()
        f = f_new
        if change <= tol:
            break
    return f


# ---- shared inputs ----------------------------------------------------------------------------------------------------
N_GRAM = 3 * 2048 + 5          # three tiles of the kernel and a ragged fourth


def synthetic(k, n=N_GRAM, seed=23):
    """``(temps, energies, rungs)``: Gamma samples of the D = 16 quadratic form on the ladder 0.5 ... 0.5 1.3^7 of
    tests/test_gpu_mbar.py, ``n`` samples in shuffled order with UNEQUAL rung counts (in the ratio 1 : 2 : 3 : 1 : ...)."""
    temps = 0.5 * (1.3 ** 7) ** (np.arange(k) / (k - 1.0))
    rng = np.random.default_rng(seed)
    share = np.cumsum(1.0 + np.arange(k) % 3)
    edges = np.floor(share / share[-1] * n).astype(np.int64)
    rungs = rng.permutation(np.searchsorted(edges, np.arange(n), side="right")).astype(np.int32)
    energies = rng.gamma(DIM / 2.0, temps[rungs])
    return temps, energies, rungs


def targets_for(temps, n_targets):
    """``n_targets`` temperatures inside the ladder, none of them a rung."""
    if n_targets == 0:
        return np.zeros(0)
    return temps[0] + (temps[-1] - temps[0]) * (np.arange(n_targets) + 0.37) / n_targets


# the calibration problem: a 4-parameter quadratic form (E ~ Gamma(2, T)) whose free energies and mean energies are exact
CAL_TEMPS = np.array([0.5, 0.8, 1.3, 2.0])
CAL_TARGETS = np.array([0.65, 1.7])
CAL_REPLICAS, CAL_PER_RUNG = 64, 512
CAL_RMS_Z = (0.75, 1.3)        # about +-3 standard errors of the RMS of 64 unit normals


def calibration_replicas(seed=5):
    rng = np.random.default_rng(seed)
    rungs = np.repeat(np.arange(CAL_TEMPS.size), CAL_PER_RUNG).astype(np.int32)
    return [(np.concatenate([rng.gamma(2.0, t, CAL_PER_RUNG) for t in CAL_TEMPS]), rungs) for _ in range(CAL_REPLICAS)]


def calibration_exact():
    """``(f, ln_z at the targets, mean energy at the targets)``."""
    return -2.0 * np.log(CAL_TEMPS / CAL_TEMPS[0]), 2.0 * np.log(CAL_TARGETS / CAL_TEMPS[0]), 2.0 * CAL_TARGETS


def rms_z(values, sigmas_, exact, pooled=False):
    """Root-mean-square z-score over the replicas (axis 0), per column; ``pooled``: over the columns (the targets) too."""
    z = (np.asarray(values) - np.asarray(exact)[None, :]) / np.asarray(sigmas_)
    return np.sqrt((z * z).mean(axis=None if pooled else 0))
