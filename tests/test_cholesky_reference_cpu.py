"""CPU tests of tests/cholesky_reference.py: the long-double reference, the packed layout and -- above all -- that the
backward-error criterion separates a correct Cholesky from a subtly wrong one (no GPU)."""
import numpy as np
import pytest

import cholesky_reference as cr
from metropolisengine_amd.engine import unpack_complex_block, unpack_real_block, unpack_real_factor

SIZES = (4, 17, 33, 64, 96)
N_CHAINS = 3


def plain_cholesky(cov, dtype, drop_term=None, single_reciprocal=False, neighbour_column=None):
    """Textbook column-by-column Cholesky of [n, m, m] matrices in numpy ``dtype`` scalars: every product and every
    subtraction rounded on its own (numpy does not fuse), the k-sum in order, the column scaled by a reciprocal as the
    kernels do.  The keyword arguments plant one defect each:

    drop_term=(j, k)       the k-th term is left out of the off-diagonal sums of column j;
    single_reciprocal      the reciprocal of the pivot's root is rounded to float32 (24 good bits) before use;
    neighbour_column=j     column j takes row j of the NEXT chain's factor in its sums."""
    a = np.asarray(cov).astype(dtype)
    n, m = a.shape[0], a.shape[1]
    fac = np.zeros_like(a)
    for j in range(m):
        s = a[:, j, j].copy()
        t = a[:, j + 1:, j].copy()
        for k in range(j):
            row_jk = fac[:, j, k]
            s = s - row_jk * row_jk
            if drop_term == (j, k):
                continue
            if neighbour_column == j:
                row_jk = np.roll(fac[:, j, k], -1)
            t = t - fac[:, j + 1:, k] * row_jk[:, None]
        assert np.all(s > 0)
        d = np.sqrt(s)
        inv = dtype(1) / d
        if single_reciprocal:
            inv = inv.astype(np.float32).astype(dtype)
        fac[:, j, j] = d
        fac[:, j + 1:, j] = t * inv[:, None]
    return fac


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", cr.CLASSES)
def test_plain_cholesky_stays_within_the_bound(name, dtype):
    """The criterion admits a correct factorisation, fused-free, in the device dtype, on every matrix class the GPU tests
    use, at n = 4, 17, 33, 64, 96 (complex analogue: the real-block recurrence on Re / Im is what the bound counts, so the
    real classes are the check).  Largest ratio seen per class over those sizes, 3 chains each (float32 / float64):

        spd 0.122 / 0.119, graded_up 0.121 / 0.204, graded_down 0.196 / 0.112, scale_small 0.121 / 0.103,
        scale_large 0.102 / 0.132, near_singular 0.086 / 0.143, equicorrelated 0.071 / 0.067

    -- five to ten times inside the worst-case bound, as rounding errors that do not conspire are."""
    worst = 0.0
    for m in SIZES:
        cov = cr.make_class(name, N_CHAINS, m, dtype, seed=11)
        fac = plain_cholesky(cov, cr.NUMPY_DTYPE[dtype])
        ratio = cr.backward_error_ratio(fac, cov, dtype)
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1), (name, dtype, m, ratio)
    print("largest ratio %s %s: %.3f" % (name, dtype, worst))


@pytest.mark.parametrize("m", SIZES)
def test_a_dropped_term_is_rejected(m):
    for dtype in ("f32", "f64"):
        cov = cr.make_class("spd", N_CHAINS, m, dtype, seed=12)
        fac = plain_cholesky(cov, cr.NUMPY_DTYPE[dtype], drop_term=(m - 2, (m - 2) // 2))
        assert np.all(cr.backward_error_ratio(fac, cov, dtype) > 1)


@pytest.mark.parametrize("m", SIZES)
def test_a_reciprocal_of_24_bits_in_float64_is_rejected(m):
    cov = cr.make_class("spd", N_CHAINS, m, "f64", seed=13)
    fac = plain_cholesky(cov, np.float64, single_reciprocal=True)
    assert np.all(cr.backward_error_ratio(fac, cov, "f64") > 1)
    assert np.all(cr.backward_error_ratio(plain_cholesky(cov, np.float64), cov, "f64") <= 1)


@pytest.mark.parametrize("m", SIZES)
def test_a_row_of_the_neighbouring_chain_is_rejected(m):
    for dtype in ("f32", "f64"):
        cov = cr.make_class("spd", N_CHAINS, m, dtype, seed=14)
        fac = plain_cholesky(cov, cr.NUMPY_DTYPE[dtype], neighbour_column=m // 2)
        assert np.all(cr.backward_error_ratio(fac, cov, dtype) > 1)


def test_ratio_is_invariant_under_diagonal_scaling():
    """Powers of two scale exactly: D C D with L -> D L gives the same ratio to the last bit of the long double."""
    cov = cr.make_class("spd", N_CHAINS, 17, "f32", seed=15)
    fac = plain_cholesky(cov, np.float32)
    d = 2.0 ** np.arange(-8, 9)
    scaled = cr.backward_error_ratio(d[None, :, None] * fac.astype(np.float64), d[None, :, None] * cov * d[None, None, :], "f32")
    assert np.array_equal(scaled, cr.backward_error_ratio(fac, cov, "f32"))


@pytest.mark.parametrize("name", cr.CLASSES)
def test_complex_classes_and_reference(name):
    """The Hermitian classes are Hermitian with a real diagonal, their long-double factor of conj(K) reproduces conj(K) far
    inside the float64 bound, and a float64 rounding of that factor passes it with k = 2 n + 4."""
    m = 13
    cov = cr.make_class(name, N_CHAINS, m, "f64", complex_block=True, seed=16)
    assert np.array_equal(cov, np.conj(np.swapaxes(cov, 1, 2))) and np.all(cov[:, np.arange(m), np.arange(m)].imag == 0)
    assert not np.array_equal(cov[0], cov[1])
    _, fac, bad = cr.reference_factor(None, cov)
    assert not bad.any()
    assert np.all(cr.backward_error_ratio(fac, np.conj(cov), "f64", complex_block=True) < 1e-2)
    assert np.all(cr.backward_error_ratio(fac.astype(np.complex128), np.conj(cov), "f64", complex_block=True) <= 1)
    assert np.all(cr.backward_error_ratio(fac, cov, "f64", complex_block=True) > 1)        # K instead of conj(K): caught


def test_reference_matches_numpy_and_reports_bad_pivots_per_chain():
    cov = cr.make_class("spd", 5, 9, "f64", seed=17)
    kmat = cr.make_class("spd", 5, 6, "f64", complex_block=True, seed=17)
    lr, lc, bad = cr.reference_factor(cov, kmat)
    assert not bad.any()
    assert np.allclose(lr.astype(np.float64), np.linalg.cholesky(cov), rtol=1e-13, atol=0)
    assert np.allclose(lc.astype(np.complex128), np.linalg.cholesky(np.conj(kmat)), rtol=1e-13, atol=1e-15)
    _, _, bad = cr.reference_factor(cr.make_indefinite(cov, [1]), cr.make_indefinite(kmat, [3]))
    assert bad.tolist() == [False, True, False, True, False]
    # the factor's own condition number: between kappa_2 and n^(3/2) kappa_2
    kappa = np.linalg.cond(cov)
    cond = cr.trace_condition(cov, lr).astype(np.float64)
    assert np.all(cond >= kappa * (1 - 1e-12)) and np.all(cond <= 9 ** 1.5 * kappa)


@pytest.mark.parametrize("nr,nc", [(5, 0), (3, 4), (0, 5), (1, 1)], ids=["real", "mixed", "complex", "smallest-mixed"])
def test_pack_is_the_inverse_of_the_engine_unpack(nr, nc):
    rng = np.random.default_rng(18)
    n = 4
    packed = rng.standard_normal((n, cr.packed_size(nr, nc)))
    real = unpack_real_block(packed, nr) if nr else None
    cplx = unpack_complex_block(packed, nr, nc) if nc else None
    assert np.array_equal(cr.pack(real, cplx), packed)                                   # covariance: symmetric / Hermitian
    real_f = unpack_real_factor(packed, nr) if nr else None
    cplx_f = unpack_complex_block(packed, nr, nc, hermitian=False) if nc else None
    assert np.array_equal(cr.pack(real_f, cplx_f), packed)                               # factor: lower triangular
    if nr:
        assert np.array_equal(unpack_real_block(cr.pack(real, cplx), nr), real) and np.all(np.triu(real_f, 1) == 0)
    if nc:
        assert np.array_equal(unpack_complex_block(cr.pack(real, cplx), nr, nc), cplx)
        assert np.array_equal(cplx, np.conj(np.swapaxes(cplx, 1, 2)))
    ident = cr.packed_identity(n, nr, nc)
    if nr:
        assert np.array_equal(unpack_real_factor(ident, nr)[0], np.identity(nr))
    if nc:
        assert np.array_equal(unpack_complex_block(ident, nr, nc, hermitian=False)[0], np.identity(nc))
