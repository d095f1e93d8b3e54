"""Long-double reference, per-entry forward-error bound, input classes and a numpy model (with planted defects) of ONE
``measure()``: running mean, running observables and the covariance recursion (plain numpy, vectorised over chains; no
GPU).  Used by tests/test_measure_reference_cpu.py and tests/test_gpu_measure_conformance.py.

What one measure() computes, with i the count of the measure being taken (the loaded ``measure_step_counter`` + 1), every
constant the EXACT rational of i:

    mean         mu (i-1)/i + x/i
    observables  o = [|x_r|, |z_c|, x_r^2]:   obs_mean (i-1)/i + o/i
    covariance   (only when i > 50) packed as in cholesky_reference.pack, delta = x - mu_old:
                 real block       C_ij (i-2)/(i-1) + delta_i delta_j / i
                 Hermitian block  K_ij (i-2)/(i-1) + delta_i conj(delta_j) / i, stored as Re and Im of the columns j < i
                 diagonals        + w^2 / i, w the real group's width (row 1) for the real block and the complex group's
                                  (row 2) for the Hermitian block when a mixed engine's widths are split, row 0 otherwise

Every entry is returned as (S, A): the exact value and the sum of the absolute values of its terms, with delta taken as the
exact difference -- so there is no cancellation inside A, and A does not grow with |mean| / std.

The criterion.  |got - S| <= gamma_k(u) A, gamma_k = k u / (1 - k u), u the unit roundoff of the engine's dtype.  The roundings,
counted as the kernels spell the arithmetic (csrc/me_device.h measure_chain, csrc/me_packed_walk.h covariance_walk,
csrc/me_runtime_dims.hip runtime_means_and_observables -- all three spell it alike):

    mean   fma(x, inv_i, mu * keep):  x/i carries inv_i (host-rounded) and the fma, 2; mu (i-1)/i carries keep (host-rounded),
           the product and the fma, 3.  k = 4 covers both with one to spare.
    obs    o is |x| (exact), x * x (1) or sqrt(fma(re, re, im * im)) (product 1, fma 1 -- halved by the root -- and the root
           itself within 1 ulp = 2 u: at most 3); then as the mean: o/i carries at most 3 + 2 = 5, the kept part 3.  k = 6.
    cov    every delta is one rounding.  Real off-diagonal fma(d_i * d_j, inv_i, m * cov_keep): the new term carries 2 deltas,
           the product, inv_i and the fma, 5; the kept term cov_keep, the product and the fma, 3.  The real diagonal has one
           more fma for the epsilon term (6 and 4; w^2/i itself: w * w, inv_i, the fma: 3).  Hermitian off-diagonal
           fma(fma(a_i, a_j, b_i * b_j), inv_i, m * cov_keep): 2 deltas, the inner product (the b b term only), the inner fma,
           inv_i, the outer fma: 6; the Hermitian diagonal, with the epsilon fma on top, 7 -- the worst entry.  k = 8.

The bounds are first-order sums of roundings made into gamma_k; they are derived from the spelling, not from any run.

Input classes (``make_inputs``), a different value per chain and per coordinate, every value a number of the engine's dtype:

    integers_rank_one  i = 64 (1/64 and 63/64 are exact): mu = 64 a, x = 64 b, a, b in -8 .. 8, complex parameters signed
                       Pythagorean pairs x 64, obs_mean = 64 c, C = 0, widths 8 k with another k per group row.  Every mean,
                       observable and covariance entry is an integer below 2^24: it must equal S BIT FOR BIT in both dtypes.
    integers_keep      i = 65 ((i-2)/(i-1) = 63/64 is exact): x = mu, width 1e-30, C = 64 x a diagonally dominant integer
                       matrix (diagonal 20000 + j, off-diagonals in +-[1, 100] varying with slot and chain, antisymmetric
                       Im): every covariance entry must come back as exactly 63/64 of itself; means and observables are held
                       to the bound.
    scaled             mu, x - mu and the factor of C are normals times 10^linspace(-2, 2, D) per parameter, widths uniform
                       in [0.01, 1]; i in SCALED_COUNTS.
    offset             as scaled with mu = 1000 s_d + noise: |mean| >> std, the case the one-pass form exists for.
"""
import numpy as np

import cholesky_reference as cr

LD = np.longdouble
UNIT_ROUNDOFF = cr.UNIT_ROUNDOFF
NUMPY_DTYPE = cr.NUMPY_DTYPE

K_MEAN, K_OBS, K_COV = 4, 6, 8
K = {"mean": K_MEAN, "obs_mean": K_OBS, "cov": K_COV}

CLASSES = ("integers_rank_one", "integers_keep", "scaled", "offset")
EXACT_COUNT = {"integers_rank_one": 64, "integers_keep": 65}
SCALED_COUNTS = (52, 10 ** 4 + 1, 10 ** 6 + 3)
TINY_WIDTH = 1e-30
PYTHAGOREAN = ((3, 4), (4, 3), (6, 8), (8, 6), (5, 0), (0, 7), (8, 0), (0, 2), (0, 0))


def gamma(k, dtype):
    u = LD(UNIT_ROUNDOFF[dtype])
    return LD(k) * u / (LD(1) - LD(k) * u)


# ------------------------------------------------------------------------------------------------------ packed slots
def slots(nr, nc):
    """Index arrays of the packed layout.  Real block: (ri, rj) of slot k < pr in order.  Hermitian block: for every pair
    j < i (ci, cj) with its Re slot ``cre`` (Im is the next one); ``cdiag`` the diagonal slots."""
    ri, rj = np.tril_indices(nr)
    pr = nr * (nr + 1) // 2
    ci = np.array([i for i in range(nc) for j in range(i)], dtype=int)
    cj = np.array([j for i in range(nc) for j in range(i)], dtype=int)
    cre = pr + ci * ci + 2 * cj
    cdiag = pr + np.arange(nc) ** 2 + 2 * np.arange(nc)
    return ri, rj, ci, cj, cre, cdiag


def n_width_rows(nr, nc):
    return 3 if nr and nc else 1


def width_rows_used(nr, nc, split=None):
    """(row of the real block's width, row of the Hermitian block's)."""
    if split is None:
        split = bool(nr and nc)             # loading ``width`` into a mixed engine marks its rows as split
    return (1, 2) if split and nr and nc else (0, 0)


# ------------------------------------------------------------------------------------------------------ the reference
def reference(inp, split=None):
    """{"mean": (S, A), "obs_mean": (S, A), "cov": (S, A)} in long double, [n, components] each; the covariance as the
    update of every packed slot (whether the engine takes it -- i > 50 -- is the caller's business)."""
    nr, nc, count = inp["nr"], inp["nc"], inp["count"]
    i = LD(count)
    keep, inv_i, cov_keep = (i - 1) / i, 1 / i, (i - 2) / (i - 1)
    x, mu, om, c, w = (np.asarray(inp[k]).astype(LD) for k in ("x", "mean", "obs_mean", "cov", "width"))
    out = {"mean": (mu * keep + x * inv_i, np.abs(mu) * keep + np.abs(x) * inv_i)}
    re, im = x[:, nr:nr + nc], x[:, nr + nc:]
    obs = np.concatenate((np.abs(x[:, :nr]), np.sqrt(re * re + im * im), x[:, :nr] ** 2), axis=1)
    out["obs_mean"] = (om * keep + obs * inv_i, np.abs(om) * keep + obs * inv_i)
    d = x - mu
    ri, rj, ci, cj, cre, cdiag = slots(nr, nc)
    pr = ri.size
    row_r, row_c = width_rows_used(nr, nc, split)
    s, a = c * cov_keep, np.abs(c) * cov_keep
    t = d[:, ri] * d[:, rj] * inv_i
    s[:, :pr] += t
    a[:, :pr] += np.abs(t)
    eps = (w[:, row_r] ** 2 * inv_i)[:, None]
    s[:, :pr][:, ri == rj] += eps
    a[:, :pr][:, ri == rj] += eps
    if nc:
        da, db = d[:, nr:nr + nc], d[:, nr + nc:]
        t1, t2 = da[:, ci] * da[:, cj] * inv_i, db[:, ci] * db[:, cj] * inv_i
        s[:, cre] += t1 + t2
        a[:, cre] += np.abs(t1) + np.abs(t2)
        t1, t2 = db[:, ci] * da[:, cj] * inv_i, da[:, ci] * db[:, cj] * inv_i
        s[:, cre + 1] += t1 - t2
        a[:, cre + 1] += np.abs(t1) + np.abs(t2)
        t = (da * da + db * db) * inv_i + (w[:, row_c] ** 2 * inv_i)[:, None]
        s[:, cdiag] += t
        a[:, cdiag] += t
    out["cov"] = (s, a)
    return out


def ratio(got, s, a, k, dtype):
    """|got - S| / (gamma_k A) per entry in long double; an entry with A = 0 must be 0 (ratio 0, else +inf); a non-finite
    value gives +inf.  Pass: ratio <= 1."""
    err = np.abs(np.asarray(got).astype(LD) - s)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / (gamma(k, dtype) * a))
    return np.where(np.isfinite(r), r, LD(np.inf))


def exact(got, s):
    """Bit for bit: the value read back (a float64 holding the engine's number) IS the long-double S."""
    return np.asarray(got).astype(LD) == s


# ------------------------------------------------------------------------------------------------------ input classes
def _rounded(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(NUMPY_DTYPE[dtype]).astype(np.float64)


def _integer_state(rng, n, nr, nc):
    """64 x small integers: real coordinates in -8 .. 8, complex ones signed Pythagorean pairs."""
    real = rng.integers(-8, 9, (n, nr))
    pairs = np.asarray(PYTHAGOREAN)[rng.integers(0, len(PYTHAGOREAN), (n, nc))] * rng.choice([-1, 1], (n, nc, 2))
    return 64.0 * np.concatenate((real, pairs[:, :, 0], pairs[:, :, 1]), axis=1)


def _integer_matrices(n, nr, nc):
    """Per chain: 64 x a diagonally dominant integer matrix per block (diagonal 20000 + j; off-diagonals +-(1 .. 100) varying
    with slot and chain; the Hermitian block with an antisymmetric imaginary part)."""
    def entries(m, salt):
        c, i, j = np.ogrid[:n, :m, :m]
        mag = (7 * (i * (i + 1) // 2 + j) + 13 * c + salt) % 100 + 1
        sign = 1 - 2 * ((i + 3 * j + c + salt) % 2)
        low = np.tril(mag * sign, -1).astype(np.float64)
        return low
    real = cplx = None
    if nr:
        low = entries(nr, 0)
        real = 64.0 * (low + np.swapaxes(low, 1, 2) + np.diag(20000.0 + np.arange(nr)))
    if nc:
        re, im = entries(nc, 5), entries(nc, 11)
        cplx = 64.0 * ((re + np.swapaxes(re, 1, 2) + np.diag(20000.0 + np.arange(nc))) + 1j * (im - np.swapaxes(im, 1, 2)))
    return real, cplx


def scales(nr, nc):
    d = nr + 2 * nc
    return 10.0 ** np.linspace(-2.0, 2.0, d) if d > 1 else np.ones(1)


def make_inputs(name, n, nr, nc, dtype, count=None, seed=0):
    """One measure()'s inputs of class ``name``: {"x", "mean", "obs_mean" [n, .], "cov" [n, P] packed, "width" [n, 1 or 3],
    "count" (= i; load ``count - 1`` as the measure_step_counter), "nr", "nc"}, every value a ``dtype`` number held in float64."""
    d, nobs, rows = nr + 2 * nc, 2 * nr + nc, n_width_rows(nr, nc)
    rng = np.random.default_rng([seed, nr, nc, CLASSES.index(name)])
    if name in EXACT_COUNT:
        assert count in (None, EXACT_COUNT[name])
        count = EXACT_COUNT[name]
        mean = _integer_state(rng, n, nr, nc)
        obs_mean = 64.0 * rng.integers(0, 9, (n, nobs))
        if name == "integers_rank_one":
            x = _integer_state(rng, n, nr, nc)
            cov = np.zeros((n, cr.packed_size(nr, nc)))
            k = 1 + (np.arange(n)[:, None] + 3 * np.arange(rows)[None, :]) % 7      # another k per chain and per group row
            width = 8.0 * k
        else:
            x = mean.copy()
            cov = cr.pack(*_integer_matrices(n, nr, nc))
            width = np.full((n, rows), TINY_WIDTH)
    else:
        assert name in ("scaled", "offset") and count is not None
        s = scales(nr, nc)
        noise = rng.standard_normal((n, d)) * s
        mean = 1000.0 * s + noise if name == "offset" else noise
        mean = _rounded(mean, dtype)
        x = mean + rng.standard_normal((n, d)) * s
        so = np.concatenate((s[:nr], s[nr:nr + nc], s[:nr] ** 2))
        obs_mean = np.abs(rng.standard_normal((n, nobs))) * so
        real = cplx = None
        if nr:
            real = cr.make_class("spd", n, nr, "f64", seed=seed + 1) * (s[:nr, None] * s[None, :nr])
        if nc:
            sc = s[nr:nr + nc]
            cplx = cr.make_class("spd", n, nc, "f64", complex_block=True, seed=seed + 1) * (sc[:, None] * sc[None, :])
        cov = cr.pack(real, cplx)
        width = rng.uniform(0.01, 1.0, (n, rows))
    inp = {"x": x, "mean": mean, "obs_mean": obs_mean, "cov": cov, "width": width}
    inp = {key: _rounded(val, dtype) for key, val in inp.items()}
    inp.update(count=int(count), nr=nr, nc=nc)
    return inp


def unpack_blocks(packed, nr, nc):
    """(real [n, nr, nr] or None, complex [n, nc, nc] or None) full Hermitian matrices of a packed field."""
    packed = np.asarray(packed, dtype=np.float64)
    n = packed.shape[0]
    ri, rj, ci, cj, cre, cdiag = slots(nr, nc)
    real = cplx = None
    if nr:
        real = np.zeros((n, nr, nr))
        real[:, ri, rj] = packed[:, :ri.size]
        real[:, rj, ri] = packed[:, :ri.size]
    if nc:
        cplx = np.zeros((n, nc, nc), dtype=np.complex128)
        cplx[:, ci, cj] = packed[:, cre] + 1j * packed[:, cre + 1]
        cplx[:, cj, ci] = packed[:, cre] - 1j * packed[:, cre + 1]
        cplx[:, np.arange(nc), np.arange(nc)] = packed[:, cdiag]
    return real, cplx


# ------------------------------------------------------------------------------------------------------ the numpy model
DEFECTS = ("delta_from_new_mean", "two_pass", "im_sign", "re_im_swapped", "real_width_on_hermitian", "no_epsilon",
           "neighbour_chain_delta", "slot_shifted_at_batch", "mean_keep_for_cov_keep")


def _fma(dtype):
    """One fused multiply-add per dtype: float32 as a float64 product-sum (the product is exact) rounded once more, float64
    through long double."""
    if dtype == "f32":
        return lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)
    return lambda a, b, c: (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)


def model(inp, dtype, defect=None, split=None):
    """One measure() as honest device code spells it, in ``dtype`` arithmetic (module docstring), or with one planted
    ``defect`` of DEFECTS.  Returns {"mean", "obs_mean", "cov"} as float64 arrays holding ``dtype`` numbers."""
    assert defect is None or defect in DEFECTS
    t = NUMPY_DTYPE[dtype]
    fma = _fma(dtype)
    nr, nc, count = inp["nr"], inp["nc"], float(inp["count"])
    keep, inv_i, cov_keep = t((count - 1.0) / count), t(1.0 / count), t((count - 2.0) / (count - 1.0))    # rounded on the host
    if defect == "mean_keep_for_cov_keep":
        cov_keep = keep
    x, mu, om, m, w = (np.asarray(inp[k]).astype(t) for k in ("x", "mean", "obs_mean", "cov", "width"))
    mean_new = fma(x, inv_i, mu * keep)
    re, im = x[:, nr:nr + nc], x[:, nr + nc:]
    obs = np.concatenate((np.abs(x[:, :nr]), np.sqrt(fma(re, re, im * im)), x[:, :nr] * x[:, :nr]), axis=1)
    obs_new = fma(obs, inv_i, om * keep)
    d = x - (mean_new if defect == "delta_from_new_mean" else mu)
    if defect == "neighbour_chain_delta":
        d = np.roll(d, 1, axis=0)
    ri, rj, ci, cj, cre, cdiag = slots(nr, nc)
    pr = ri.size
    row_r, row_c = width_rows_used(nr, nc, split)
    if defect == "real_width_on_hermitian":
        row_c = row_r
    w2r, w2c = (w[:, row_r] * w[:, row_r])[:, None], (w[:, row_c] * w[:, row_c])[:, None]
    if defect == "no_epsilon":
        w2r, w2c = w2r * t(0), w2c * t(0)
    out = m * cov_keep
    da, db = d[:, nr:nr + nc], d[:, nr + nc:]
    if defect == "two_pass":
        # the literal form: C keep + mu_old mu_old^H - i/(i-1) mu_new mu_new^H + x x^H / (i-1) + (w^2 / i) I, term by term
        g, h = t(count / (count - 1.0)), t(1.0 / (count - 1.0))

        def literal(a_old, a_new, a_x, ii, jj):
            return (a_old[:, ii] * np.conj(a_old[:, jj]) - g * (a_new[:, ii] * np.conj(a_new[:, jj]))) + (a_x[:, ii] * np.conj(a_x[:, jj])) * h
        out[:, :pr] = out[:, :pr] + literal(mu[:, :nr], mean_new[:, :nr], x[:, :nr], ri, rj)
        out[:, :pr][:, ri == rj] += w2r * inv_i
        if nc:
            z = lambda v: v[:, nr:nr + nc] + 1j * v[:, nr + nc:]           # complex64 / complex128: arithmetic in ``dtype``
            off = literal(z(mu), z(mean_new), z(x), ci, cj)
            out[:, cre] += off.real
            out[:, cre + 1] += off.imag
            idx = np.arange(nc)
            out[:, cdiag] += literal(z(mu), z(mean_new), z(x), idx, idx).real + w2c * inv_i
        return {"mean": mean_new.astype(np.float64), "obs_mean": obs_new.astype(np.float64), "cov": out.astype(np.float64)}
    dj = d[:, rj]
    if defect == "slot_shifted_at_batch":       # the tail after a 16-entry batch starts one column early
        dj = d[:, np.where((rj == 16) & (ri > 16), 15, rj)]
    v = fma(d[:, ri] * dj, inv_i, out[:, :pr])
    diag = ri == rj
    v[:, diag] = fma(w2r, inv_i, v[:, diag])
    out[:, :pr] = v
    if nc:
        ai, bi = da[:, ci], db[:, ci]
        cjj = np.where((cj == 8) & (ci > 8), 7, cj) if defect == "slot_shifted_at_batch" else cj
        aj, bj = da[:, cjj], db[:, cjj]
        vr = fma(fma(ai, aj, bi * bj), inv_i, out[:, cre])
        if defect == "im_sign":
            vi = fma(fma(ai, bj, -(bi * aj)), inv_i, out[:, cre + 1])
        else:
            vi = fma(fma(bi, aj, -(ai * bj)), inv_i, out[:, cre + 1])
        if defect == "re_im_swapped":
            vr, vi = vi, vr
        out[:, cre], out[:, cre + 1] = vr, vi
        out[:, cdiag] = fma(w2c, inv_i, fma(fma(da, da, db * db), inv_i, out[:, cdiag]))
    return {"mean": mean_new.astype(np.float64), "obs_mean": obs_new.astype(np.float64), "cov": out.astype(np.float64)}
