"""Long-double reference and backward-error criterion for the per-chain Cholesky refresh (plain numpy, vectorised over
chains; no GPU).  Used by tests/test_cholesky_reference_cpu.py and tests/test_gpu_cholesky_conformance.py.

Layout (include/metropolis_engine.h, ME_FIELD_COV / ME_FIELD_FACTOR): the real lower triangle row by row, entry (i, j) at
``i (i + 1) / 2 + j``; then the Hermitian block, row i at ``pr + i^2``: (Re, Im) pairs of (i, j < i), then the real diagonal.
``pack_*`` are the inverses of ``engine.unpack_real_block``, ``unpack_complex_block`` and ``unpack_real_factor``.

The criterion.  A Cholesky factorisation computed in floating point satisfies, whatever the conditioning of C and in any
order of summation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 10.3 with Lemma 8.4),

    |C - L L^T|_ij  <=  gamma_{n+1} (|L| |L|^T)_ij,        gamma_k = k u / (1 - k u),

because entry (i, j) is ``(C_ij - sum_{k<j} L_ik L_jk) / L_jj``: j products, j subtractions and one division (or square
root), each rounded once.  The device kernels multiply by a reciprocal instead of dividing (one rounding more: k = n + 2)
and some take square root and reciprocal from a hardware estimate refined to about an ulp rather than correctly rounded;
an ulp is up to 2 u relative, so the bound is evaluated with u' = 2 u.  Counting exactly: j u for the sum and at most
2 u' for pivot and reciprocal, (j + 4) u <= (n + 3) u < (n + 2) 2 u.  Fused multiply-adds only remove roundings.

Hermitian block.  L L^H = conj(K) in complex arithmetic: the real part of entry (i, j) is ``Re C_ij - sum_k (ar br + ai bi)``,
a REAL recurrence with 2 j products, and so is the imaginary part -- each complex multiply-add is four real ones, two per
component.  Since ``|ar br| + |ai bi| <= |a| |b|``, each component's residual is bounded by ``(2 j u + 2 u') (|L| |L|^H)_ij``
with |.| the modulus, and the modulus of the residual by sqrt 2 times that: sqrt 2 (2 n + 2) u < (2 n + 4) 2 u.  Hence
k = 2 n + 4 = 2 (n + 2) for the complex block, with u' = 2 u as before.

The ratio of the two sides is invariant under diagonal scaling C -> D C D (L -> D L scales both sides by d_i d_j) and does
not involve the condition number.  ``ratio <= 1`` is the pass condition; it is derived, not measured.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble

UNIT_ROUNDOFF = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NUMPY_DTYPE = {"f32": np.float32, "f64": np.float64}


# ---------------------------------------------------------------------------------------------------- packed layout
def packed_size(nr, nc):
    return nr * (nr + 1) // 2 + nc * nc


def pack_real_block(mats):
    """[n, nr, nr] -> [n, nr (nr + 1) / 2]: the lower triangle row by row (covariance or factor)."""
    mats = np.asarray(mats)
    il = np.tril_indices(mats.shape[1])
    return mats[:, il[0], il[1]]


def pack_complex_block(mats):
    """[n, nc, nc] complex -> [n, nc^2]: the lower triangle as (Re, Im) pairs, the diagonal's real part."""
    mats = np.asarray(mats)
    n, nc = mats.shape[0], mats.shape[1]
    out = np.zeros((n, nc * nc), dtype=mats.real.dtype)
    for i in range(nc):
        for j in range(i):
            out[:, i * i + 2 * j] = mats[:, i, j].real
            out[:, i * i + 2 * j + 1] = mats[:, i, j].imag
        out[:, i * i + 2 * i] = mats[:, i, i].real
    return out


def pack(real_block, complex_block):
    """The engine's packed field from the two blocks (either may be None or empty)."""
    parts = []
    if real_block is not None and np.asarray(real_block).shape[1]:
        parts.append(pack_real_block(real_block))
    if complex_block is not None and np.asarray(complex_block).shape[1]:
        parts.append(pack_complex_block(complex_block))
    return np.concatenate(parts, axis=1)


def packed_identity(n, nr, nc):
    return pack(np.broadcast_to(np.identity(nr), (n, nr, nr)), np.broadcast_to(np.identity(nc).astype(complex), (n, nc, nc)))


# ---------------------------------------------------------------------------------------------------- the reference
def _cholesky(a):
    """Column-by-column Cholesky of [n, m, m] long-double (or complex long-double Hermitian) matrices, lower triangle
    read only.  Returns (L, bad): bad[c] when chain c met a pivot <= 0 (its L is then meaningless)."""
    n, m = a.shape[0], a.shape[1]
    fac = np.zeros_like(a)
    bad = np.zeros(n, dtype=bool)
    for j in range(m):
        row = fac[:, j, :j]
        s = a[:, j, j].real - np.sum(row.real * row.real + row.imag * row.imag, axis=1)
        bad_j = ~(s > 0)
        bad |= bad_j
        d = np.sqrt(np.where(bad_j, LD(1), s))
        fac[:, j, j] = d
        if j + 1 < m:
            t = a[:, j + 1:, j] - (fac[:, j + 1:, :j] @ np.conj(row)[:, :, None])[:, :, 0]
            fac[:, j + 1:, j] = t / d[:, None]
    return fac, bad


def reference_factor(cov_real, cov_complex):
    """(L_real, L_complex, bad): L_real = chol(C) and L_complex = chol(conj K) (the proposals use conj(K): quirk Q3,
    metropolis_engine.py:292-298) per chain in long double; ``bad[c]`` reports a pivot <= 0 in either block of chain c
    instead of raising.  A block may be None."""
    lr = lc = None
    bad = None
    if cov_real is not None and np.asarray(cov_real).shape[1]:
        lr, bad = _cholesky(np.asarray(cov_real).astype(LD))
    if cov_complex is not None and np.asarray(cov_complex).shape[1]:
        lc, bad_c = _cholesky(np.conj(np.asarray(cov_complex).astype(CLD)))
        bad = bad_c if bad is None else bad | bad_c
    return lr, lc, bad


def gamma(n, dtype, complex_block=False):
    """gamma_k of the module docstring in long double: k = n + 2 (real), 2 n + 4 (complex), u' = 2 u of ``dtype``."""
    k = LD(2 * n + 4 if complex_block else n + 2)
    u2 = LD(2) * LD(UNIT_ROUNDOFF[dtype])
    return k * u2 / (LD(1) - k * u2)


def backward_error_ratio(fac, cov, dtype, complex_block=False):
    """Per chain: max over the lower triangle (i >= j) of |C - L L^H|_ij / (gamma_k (|L| |L|^H)_ij), in long double.

    ``fac`` [n, m, m] is the factor as the device stored it (its strict upper triangle is ignored), ``cov`` [n, m, m] the
    matrix it factorised -- for the Hermitian block pass conj(K).  Only the lower triangle of ``cov`` is read, as by the
    kernels.  Pass: ratio <= 1.  A zero bound with a non-zero residual is +inf; non-finite input gives +inf."""
    kind = CLD if complex_block else LD
    fac = np.tril(np.asarray(fac).astype(kind))
    cov = np.asarray(cov).astype(kind)
    m = fac.shape[1]
    resid = np.abs(cov - fac @ np.conj(np.swapaxes(fac, 1, 2)))
    mod = np.abs(fac)
    bound = gamma(m, dtype, complex_block) * (mod @ np.swapaxes(mod, 1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(resid == 0, LD(0), resid / bound)
    ratio = np.where(np.isfinite(ratio), ratio, LD(np.inf))
    il = np.tril_indices(m)
    return ratio[:, il[0], il[1]].max(axis=1)


def trace_condition(cov, fac):
    """cond_tr(C) = tr(C) ||C^-1||_F per chain in long double, from the long-double factor ``fac`` of ``cov``.

    kappa_2(C) <= cond_tr(C) <= n^(3/2) kappa_2(C).  It is the condition number of the FACTOR with respect to a backward error
    of the kind above: to first order dL = L tril'(L^-1 dC L^-H) (tril' halves the diagonal), so
    ||dL||_F <= ||L||_2 ||C^-1||_2 ||dC||_F, and ||dC||_F <= gamma || |L| |L|^H ||_F <= gamma ||L||_F^2 = gamma tr(C); with
    ||L||_2 <= ||L||_F this gives  ||dL||_F / ||L||_F <= gamma tr(C) ||C^-1||_2 <= gamma cond_tr(C)."""
    n, m = fac.shape[0], fac.shape[1]
    inv = np.zeros_like(fac)                       # L^-1 by forward substitution
    eye = np.identity(m, dtype=fac.dtype)
    for i in range(m):
        inv[:, i, :] = (eye[i] - (fac[:, None, i, :i] @ inv[:, :i, :])[:, 0, :]) / fac[:, i, i][:, None]
    cinv = np.conj(np.swapaxes(inv, 1, 2)) @ inv
    trace = np.einsum("cii->c", np.asarray(cov).astype(fac.dtype)).real
    return trace * np.sqrt(np.sum(np.abs(cinv) ** 2, axis=(1, 2)))


def factor_distance(fac, ref):
    """||tril(fac) - ref||_F / ||ref||_F per chain in long double."""
    diff = np.tril(np.asarray(fac).astype(ref.dtype)) - ref
    return np.sqrt(np.sum(np.abs(diff) ** 2, axis=(1, 2)) / np.sum(np.abs(ref) ** 2, axis=(1, 2)))


# ---------------------------------------------------------------------------------------------------- matrix classes
CLASSES = ("spd", "graded_up", "graded_down", "scale_small", "scale_large", "near_singular", "equicorrelated")
WELL_CONDITIONED = ("spd", "scale_small", "scale_large")
GRADING_DECADES = {"f32": 3.0, "f64": 6.0}           # D = 10^-g ... 10^+g
GLOBAL_SCALE = {"f32": 1e12, "f64": 1e20}            # pivots stay normal numbers, far above the kernels' 1e-30 clamp
EQUICORRELATION = 0.999


def _normal(rng, shape, complex_block):
    if complex_block:
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    return rng.standard_normal(shape)


def _one_matrix(name, m, dtype, complex_block, rng):
    a = _normal(rng, (m, m), complex_block)
    spd = a @ np.conj(a.T) / m + np.identity(m)
    if name == "spd":
        return spd
    if name in ("graded_up", "graded_down"):
        g = GRADING_DECADES[dtype]
        d = np.logspace(-g, g, m) if m > 1 else np.ones(1)
        if name == "graded_down":
            d = d[::-1]
        return d[:, None] * spd * d[None, :]
    if name == "scale_small":
        return spd / GLOBAL_SCALE[dtype]
    if name == "scale_large":
        return spd * GLOBAL_SCALE[dtype]
    if name == "near_singular":
        # eigenvalues spaced geometrically from 1 down to 100 n u in a random orthonormal (unitary) basis
        q, _ = np.linalg.qr(a)
        lam = np.logspace(0.0, np.log10(100.0 * m * UNIT_ROUNDOFF[dtype]), m) if m > 1 else np.ones(1)
        return (q * lam[None, :]) @ np.conj(q.T)
    if name == "equicorrelated":
        s = rng.uniform(0.5, 2.0, m)
        if complex_block:
            s = s * np.exp(2j * np.pi * rng.uniform(size=m))
        corr = np.full((m, m), EQUICORRELATION) + (1.0 - EQUICORRELATION) * np.identity(m)
        return s[:, None] * corr * np.conj(s)[None, :]
    raise ValueError(name)


def make_class(name, n_chains, m, dtype, complex_block=False, seed=0):
    """[n_chains, m, m] matrices of class ``name`` (CLASSES), a different one per chain -- the generator is seeded from
    (seed, chain) -- exactly Hermitian, every entry a ``dtype`` number (returned as float64 / complex128)."""
    kind = np.complex128 if complex_block else np.float64
    out = np.zeros((n_chains, m, m), dtype=kind)
    real_type = NUMPY_DTYPE[dtype]
    for c in range(n_chains):
        mat = _one_matrix(name, m, dtype, complex_block, np.random.default_rng([seed, c, m, int(complex_block)]))
        low = np.tril(mat)
        if complex_block:
            low = low.real.astype(real_type).astype(np.float64) + 1j * low.imag.astype(real_type).astype(np.float64)
            low[np.arange(m), np.arange(m)] = low[np.arange(m), np.arange(m)].real
        else:
            low = low.astype(real_type).astype(np.float64)
        out[c] = low + np.conj(np.tril(low, -1).T)
    return out


def make_indefinite(mats, chains):
    """A copy of ``mats`` in which the matrices of ``chains`` have the sign of their middle diagonal entry flipped: not
    positive definite, the Cholesky pivot of that column is negative whatever the rounding."""
    out = mats.copy()
    j = mats.shape[1] // 2
    for c in chains:
        out[c, j, j] = -out[c, j, j]
    return out
