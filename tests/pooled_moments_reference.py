"""Exact reference, forward-error bound and arithmetic models for the pooled-moment reduction (plain numpy; no GPU).
Used by tests/test_pooled_moments_reference_cpu.py and tests/test_gpu_pooled_moments_conformance.py.

The reduction.  ``pooled_moments()`` is the only thing an engine hands to the ensemble layer.  Stage 1 has seven
implementations -- k_pool_gram64 / k_pool_gram64_f64 and k_pool_gram32<NR,NC> / k_pool_gram32_f64<NR,NC> on the matrix
cores (csrc/me_pool_gram.h), k_pool_reduce<R, 64 | 32 | 16> (csrc/me_generic.hip) -- and k_pool_finish adds their partial
rows up.  All of them return the vector ``me_pooled_moments`` documents in include/metropolis_engine.h, D = nr + 2 nc:

    [ n | sum x (D) | sum x_i x_j, packed lower, (i, j) at i (i + 1) / 2 + j (D (D + 1) / 2) |
      sum |x_r| (nr) | sum |z_c| (nc) | sum x_r^2 (nr) | accepted | proposed ]

(``layout``; the state is [real | Re z | Im z], so z_c = x[nr + c] + i x[nr + nc + c]).

The reference.  ``exact_moments`` returns, for every entry, the sum S of its terms t_c over the chains and the sum A of
their absolute values: in int64 -- exactly -- for integer states, in long double (chunks of 4 096 chains, added up in long
double) otherwise.

The bound.  The documented numerics class: a tile of at most 64 chains is multiplied and summed in the engine's dtype R,
tiles are added in float64.  A term that passes through k roundings carries a factor (1 + theta_k), |theta_k| <= gamma_k(u) =
k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., lemma 3.1), in ANY order of summation.

  * Inside a tile (unit roundoff u_R): one rounding for the product x_i x_j; one for a |z_c| row, which is rounded to R
    after a square root taken in double precision (the double-precision steps before it are 2^-29 of that and are
    absorbed by the slack below); and the sum of at most 64 terms.  A plain sum is at most 63 additions.  A matrix-core
    accumulate D = C + a0 b0 + a1 b1 counts as TWO roundings of size u_R per term it touches -- the convention
    ``dense_product_reference.gamma_units`` uses for ``fp32_mfma``, because neither the order nor the internal rounding
    of the instruction's sum is specified and a truncated addition errs by 2 u_R -- and a term sits in at most 64 / 2 = 32
    accumulates of its register plus the addition of the two accumulators, so 2 x 64 covers both forms:

        k = 2 x 64 + 2 = 130                                                           (``K_TILE``)

  * Across tiles (u_64 = 2^-53): a tile's partial sum passes through the float64 additions of its wavefront, its workgroup
    and k_pool_finish: fewer than the number of partial sums, hence fewer than n additions.

  Together  got = sum_c t_c (1 + theta_k)(1 + theta'_n), so

      |got - S|  <=  ( gamma_k(u_R) (1 + gamma_n(u_64)) + gamma_n(u_64) ) A,        k = 130         (float32 engines)

  * float64 engines: everything is float64.  A term is one product (for |z_c|: two squares, a sum and a root, of which the
    root halves the first three: 2 roundings) and sits in fewer than n additions in whatever order:

      |got - S|  <=  gamma_{n + 2}(2^-53) A                                                          (float64 engines)

    which holds for every summation order and therefore does not depend on the launch geometry.

``bound(dtype, n, family)``.  ``family`` is "fp32_mfma" for the float32 Gram kernels and "generic" otherwise; both use
k = 130.  How v_mfma_f32_32x32x2_f32 rounds its internal sum on gfx950 is not documented; ``MFMA_WIDENING`` is the one
place where a measured instruction behaviour would widen the ``fp32_mfma`` family (by a power of two of u), and it is 1:
see DESIGN.md ("Pooled moments: the criterion") for the measured ratios.  The generic family is never widened.

What exactness adds.  The bound is a worst case; a chain dropped at a tile edge moves an entry by 1 / n of A and passes it
at every large n.  The class ``integers`` closes that: every real parameter is a non-zero integer in +-1..8, every complex
parameter a signed Pythagorean pair from {(3,4), (4,3), (6,8), (8,6), (k,0), (0,k)}, so that every product is at most 64
in magnitude, a tile sum at most 4 096 < 2^24, a full sum at most 64 x 263 173 = 1.7 10^7 < 2^53, and |z| the root of a
perfect square (at most 10): in every kernel, either dtype, every summation order and whatever the matrix core's
internal rounding, each entry must EQUAL S.  This class carries the structural checks at every chain count.

What ``wide_integers`` adds.  The bound cannot see WHERE the float32 arithmetic ends: a wavefront (a block of the generic
kernel) owns the tiles first + k step, so float32 accumulators that run on across ITS tiles -- the tempting speed-up --
add one rounding per trip, two trips at the second-trip sizes and 32 at 8 million chains, against the 130 the class allows; the
partial sums of the wavefronts are added in float64 either way.  No practical chain count separates that (the CPU test
records the ratios).  Exactness does, once a tile's sum fills float32's 24 bits: real parameters are integers of
magnitude 363..511, complex ones the Pythagorean pairs times 51 (components at most 408, |z| at most 510), so that every
product is below 2^18 and every partial sum of the at most 64 terms of a tile an integer below 64 x 511^2 < 2^24 -- a tile
is exact in float32 in any order -- while sum x_r^2 of a full tile is at least 64 x 363^2 > 2^23: two tiles of one wavefront
pass 2^24, where float32 holds even integers only, and a full sum (at most 2^18 x 263 173 < 2^53) is exact in float64.
An honest kernel must return S; float32 carried from a wavefront's first tile into its second cannot.  The class runs
where a wavefront or block has a second FULL 64-chain tile: the float32 second-trip cases.

Models of a correct implementation (``model_moments``): tile-wise float32 products and sums in two orders -- sequential,
and pairwise as a matrix-core-like tree -- with float64 across tiles, and all-float64.  Fractions of the bound they reach on
the float classes at the GPU module's sizes (tests/test_pooled_moments_reference_cpu.py prints them):

    float32 tiles, sequential   0.0006 - 0.050        float32 tiles, pairwise   0.0003 - 0.020
    all-float64                 0.0002 - 0.098 from 63 chains on (the bound grows with n, the error with about its root);
                                0.43 at one chain, where a single |z| is held to gamma_3

Planted defects (``DEFECTS``: keyword arguments of ``model_moments``), each caught by one of the two exact classes -- the CPU
test asserts which; the bound on the float classes is what holds the numerics class WITHIN a tile (a tile summed in
bfloat16, say), and none of these needs it:

    drop_last_of_ragged_tile   the last chain of a ragged tile left out of every sum           integers
    stale_prefetch             a wavefront's second-trip tile replaced by its first-trip tile   integers
    tile64_where_32            tiles laid out for 64 chains where 32 are staged                  integers
    transposed_block           pairs of the off-diagonal block written to the transposed slot    integers
    wrong_complex_pairing      Re row c paired with the Im row of c + 1 in |z_c|                integers
    no_abs                     the |x_r| row summed without the absolute value                  integers
    square_of_next_parameter   sum x_r^2 taken from the diagonal of parameter r + 1            integers
    fp32_across_tiles          a wavefront's (block's) tiles first + k step added up in float32,  wide_integers
                               with the launch geometry (``tiles_between_trips``); also with the
                               wavefronts' partial sums added in float32 (``across``)
    f32_sqrt_of_f32_squares    |z_c| = sqrtf(re re + im im) in float32                            NOT caught: see below

The last one errs by at most 3 u per term (two rounded squares, halved by the root, the sum, the root), inside the 130 u the
class allows and exact on Pythagorean pairs; on the large-ratio pairs of ``scaled`` the smaller square vanishes either
way.  A forward-error bound on sums cannot tell it from honest code; the CPU test records its ratio and asserts that it
stays inside the bound, so that nobody takes the conformance module for a test of that property.
"""
import numpy as np

LD = np.longdouble

UNIT_ROUNDOFF = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NUMPY_DTYPE = {"f32": np.float32, "f64": np.float64}

K_TILE = 2 * 64 + 2
MFMA_WIDENING = 1                      # factor on K_TILE for the "fp32_mfma" family only (a power of two; 1 = as derived)


# ---------------------------------------------------------------------------------------------------- layout
def moments_size(nr, nc):
    d = nr + 2 * nc
    return 1 + d + d * (d + 1) // 2 + 2 * nr + nc + 2


def layout(nr, nc):
    """name -> slice of the public moment vector."""
    d = nr + 2 * nc
    p = d * (d + 1) // 2
    at, out = 0, {}
    for name, size in (("n", 1), ("sum", d), ("pairs", p), ("abs_real", nr), ("abs_complex", nc), ("squares", nr),
                       ("accepted", 1), ("proposed", 1)):
        out[name] = slice(at, at + size)
        at += size
    assert at == moments_size(nr, nc)
    return out


def _assemble(nr, nc, count, sums, gram, abs_real, abs_complex, dtype, squares=None):
    """The public vector from its parts; ``gram`` is [D, D]; the two counters are 0 (nothing stepped)."""
    lay = layout(nr, nc)
    d = nr + 2 * nc
    out = np.zeros(moments_size(nr, nc), dtype=dtype)
    out[0] = count
    out[lay["sum"]] = sums
    out[lay["pairs"]] = gram[np.tril_indices(d)]             # row-major lower triangle: (i, j) at i (i + 1) / 2 + j
    out[lay["abs_real"]] = abs_real
    out[lay["abs_complex"]] = abs_complex
    out[lay["squares"]] = np.diagonal(gram)[:nr] if squares is None else squares
    return out


# ---------------------------------------------------------------------------------------------------- the bound
def gamma(m, u):
    return m * u / (1.0 - m * u)


def bound(dtype, n, family="generic"):
    """Largest admissible |got - S| / A of an entry; see the module docstring."""
    u64 = UNIT_ROUNDOFF["f64"]
    if dtype == "f64":
        return gamma(n + 2, u64)
    k = K_TILE * (MFMA_WIDENING if family == "fp32_mfma" else 1)
    g = gamma(n, u64)
    return gamma(k, UNIT_ROUNDOFF["f32"]) * (1.0 + g) + g


# ---------------------------------------------------------------------------------------------------- exact reference
def _chunks(n, size=4096):
    return [(lo, min(n, lo + size)) for lo in range(0, n, size)]


def is_integer_state(x):
    return bool(np.all(x == np.rint(x)) and np.max(np.abs(x), initial=0.0) < 2 ** 20)


def exact_moments(x, nr, nc):
    """(S, A) for the state x [n, D]: per entry of the public vector, the sum of its terms and the sum of their absolute
    values.  int64 and exact for integer states (|z| must then be the root of a perfect square), long double otherwise."""
    x = np.asarray(x)
    n, d = x.shape
    assert d == nr + 2 * nc
    if is_integer_state(x):
        xi = np.rint(x).astype(np.int64)
        re, im = xi[:, nr:nr + nc], xi[:, nr + nc:]
        r2 = re * re + im * im
        root = np.rint(np.sqrt(r2.astype(np.float64))).astype(np.int64)
        assert np.array_equal(root * root, r2), "|z| is not an integer"
        ai = np.abs(xi)
        # the Gram sums in float64: every partial sum is an integer below 2^53, so any order of additions is exact
        xf, af = xi.astype(np.float64), ai.astype(np.float64)
        assert int(np.max(ai, initial=0)) ** 2 * n < 2 ** 53
        s = _assemble(nr, nc, n, xi.sum(axis=0), (xf.T @ xf).astype(np.int64), ai[:, :nr].sum(axis=0), root.sum(axis=0), np.int64)
        a = _assemble(nr, nc, n, ai.sum(axis=0), (af.T @ af).astype(np.int64), ai[:, :nr].sum(axis=0), root.sum(axis=0), np.int64)
        return s, a
    sums, gram, a_sums, a_gram = np.zeros(d, LD), np.zeros((d, d), LD), np.zeros(d, LD), np.zeros((d, d))
    abs_complex = np.zeros(nc, LD)
    for lo, hi in _chunks(n):
        xc = x[lo:hi].astype(LD)
        ac = np.abs(xc)
        sums += xc.sum(axis=0)
        a_sums += ac.sum(axis=0)
        gram += xc.T @ xc
        a64 = np.abs(x[lo:hi])
        a_gram += a64.T @ a64                     # float64: A scales the bound, 4 096 x 2^-53 of it changes no verdict
        re, im = xc[:, nr:nr + nc], xc[:, nr + nc:]
        abs_complex += np.sqrt(re * re + im * im).sum(axis=0)
    s = _assemble(nr, nc, n, sums, gram, a_sums[:nr], abs_complex, LD)
    a = _assemble(nr, nc, n, a_sums, a_gram, a_sums[:nr], abs_complex, LD)
    return s, a


def error_ratio(got, s, a):
    """|got - S| / A per entry as float64, 0 where both vanish and inf where A = 0 but got != S (entries without terms, the
    two counters among them, must come back as exact zeros)."""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(s, dtype=LD))
    a = np.asarray(a, dtype=LD)
    ratio = np.zeros(err.shape, dtype=np.float64)
    live = a > 0
    ratio[live] = (err[live] / a[live]).astype(np.float64)
    ratio[~live & (err > 0)] = np.inf
    return ratio


def is_exact(got, s):
    """Entry by entry equal to an int64 reference (every value below 2^53, so the comparison in float64 is exact)."""
    assert s.dtype == np.int64 and np.max(np.abs(s)) < 2 ** 53
    return np.array_equal(np.asarray(got, dtype=np.float64), s.astype(np.float64))


# ---------------------------------------------------------------------------------------------------- input classes
CLASSES = ("integers", "scaled", "offset")     # every case list draws from these three ...
WIDE = "wide_integers"                          # ... and the float32 second-trip cases add this one
_CLASS_IDS = CLASSES + (WIDE,)
WIDE_REAL = (363, 511)                          # 64 x 363^2 > 2^23, 64 x 511^2 < 2^24
WIDE_COMPLEX = 51                               # (6, 8) x 51 = (306, 408): products below 2^18, |z| = 510
_PYTHAGOREAN = ((3, 4), (4, 3), (6, 8), (8, 6))


def make_state(name, nr, nc, n, seed, dtype):
    """x [n, D] of class ``name`` as a float64 array whose every value is exactly representable in ``dtype``."""
    t = NUMPY_DTYPE[dtype]
    d = nr + 2 * nc
    rng = np.random.default_rng([seed, nr, nc, n, _CLASS_IDS.index(name)])
    if name in ("integers", WIDE):
        wide = name == WIDE
        x = np.empty((n, d))
        x[:, :nr] = rng.integers(WIDE_REAL[0], WIDE_REAL[1] + 1, size=(n, nr)) if wide else rng.integers(1, 9, size=(n, nr))
        kind = rng.integers(0, 6, size=(n, nc))                     # four Pythagorean pairs, (k, 0), (0, k)
        k = rng.integers(1, 9, size=(n, nc))
        re, im = np.where(kind == 4, k, 0), np.where(kind == 5, k, 0)
        for code, (p, q) in enumerate(_PYTHAGOREAN):
            re, im = np.where(kind == code, p, re), np.where(kind == code, q, im)
        x[:, nr:nr + nc], x[:, nr + nc:] = (WIDE_COMPLEX * re, WIDE_COMPLEX * im) if wide else (re, im)
        return x * rng.choice([-1.0, 1.0], size=(n, d))
    scale = 10.0 ** np.linspace(-2.0, 2.0, d)                       # |values| within 1e-7 .. 1e3: normal float32 numbers
    g = rng.standard_normal((n, d))
    if name == "scaled":
        x = g * scale
    elif name == "offset":
        x = (3.0 + 0.1 * g) * scale                                  # every term of every entry has the same sign
    else:
        raise KeyError(name)
    x = x.astype(t).astype(np.float64)
    assert np.all(np.abs(x) > 1e-15) and np.all(np.abs(x) < 1e4)     # squares stay normal float32 numbers
    return x


# ---------------------------------------------------------------------------------------------------- models
def _tile_sum(term, lo, hi, order):
    """sum of term(col), col in [lo, hi), in the terms' own dtype: one after the other, or as a balanced tree."""
    if order == "sequential":
        s = term(lo)
        for col in range(lo + 1, hi):
            s = s + term(col)
        return s
    if hi - lo == 1:
        return term(lo)
    mid = (lo + hi) // 2
    return _tile_sum(term, lo, mid, order) + _tile_sum(term, mid, hi, order)


def model_moments(x, nr, nc, dtype, order=None, tile=64, across=np.float64, trip_step=None, trips=np.float64,
                  drop_last_of_ragged_tile=False,
                  stale_prefetch=None, tile_stride=None, transposed_block=False, wrong_complex_pairing=False, no_abs=False,
                  square_of_next_parameter=False, f32_sqrt_of_f32_squares=False):
    """The reduction as the kernels' documentation states it: augmented rows [x | |x_r| | |z_c|] with |z_c| rounded to the
    device dtype after a double-precision root, products and sums of a ``tile``-chain tile in the device dtype in the given
    ``order`` ("sequential" | "pairwise"; "matmul", the default of the all-float64 model ``dtype="f64"``: whatever order numpy's
    batched product takes), the public layout.  Across tiles: with ``trip_step`` (``tiles_between_trips``) wavefront w adds
    its tiles w + k trip_step up in ``trips`` and the wavefronts' sums are added in ``across``; without it the tiles are added
    one after the other in ``across`` (in float64 the two differ by float64 roundings only).  The other keyword arguments plant one
    defect each (module docstring); ``stale_prefetch`` is (tile that is replaced, tile it is replaced by), ``tile_stride`` the
    chains between the starts of two tiles."""
    t = NUMPY_DTYPE[dtype]
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    xt = x.astype(t)
    re, im = xt[:, nr:nr + nc], xt[:, nr + nc:]
    if wrong_complex_pairing:
        im = np.roll(im, -1, axis=1)
    if f32_sqrt_of_f32_squares:
        z = np.sqrt(re * re + im * im)
    else:
        z = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(t)
    aug = np.concatenate((xt, xt[:, :nr] if no_abs else np.abs(xt[:, :nr]), z), axis=1)
    if drop_last_of_ragged_tile and n % tile:
        aug[n - 1] = 0
    stride = tile if tile_stride is None else tile_stride
    n_tiles = (n + tile - 1) // tile
    tiles = np.zeros((n_tiles, tile, aug.shape[1]), dtype=t)
    for k in range(n_tiles):
        rows = aug[k * stride:min(n, k * stride + tile)]
        tiles[k, :rows.shape[0]] = rows
    if stale_prefetch is not None:
        tiles[stale_prefetch[0]] = tiles[stale_prefetch[1]]
    i, j = np.tril_indices(d)
    if order is None:
        order = "sequential" if dtype == "f32" else "matmul"
    if order == "matmul":
        row_sums, pair_sums = tiles.sum(axis=1), np.matmul(tiles[:, :, :d].transpose(0, 2, 1), tiles[:, :, :d])[:, i, j]
        return _finish_model(nr, nc, n, d, i, j, row_sums, pair_sums, across, trip_step, trips, transposed_block, square_of_next_parameter)
    row_sums = _tile_sum(lambda col: tiles[:, col, :], 0, tile, order)                         # [tiles, n_aug]
    # (the full outer product of a chain's parameters, of which the lower triangle is kept: no gathers inside the loop)
    full = _tile_sum(lambda col: tiles[:, col, :d, None] * tiles[:, col, None, :d], 0, tile, order)
    pair_sums = full[:, i, j]                                                                   # [tiles, pairs]
    return _finish_model(nr, nc, n, d, i, j, row_sums, pair_sums, across, trip_step, trips, transposed_block, square_of_next_parameter)


def _finish_model(nr, nc, n, d, i, j, row_sums, pair_sums, across, trip_step, trips, transposed_block, square_of_next_parameter):
    def total(v):                                                     # one after the other, in ``trips`` then in ``across``
        if trip_step is not None and v.shape[0] > trip_step:
            whole = -(-v.shape[0] // trip_step) * trip_step           # (a wavefront without a tile in the last trip adds 0)
            v = np.concatenate((v, np.zeros((whole - v.shape[0],) + v.shape[1:], v.dtype))).reshape((-1, trip_step) + v.shape[1:])
            v = np.add.accumulate(v.astype(trips), axis=0)[-1]
        return np.add.accumulate(v.astype(across), axis=0)[-1].astype(np.float64)

    row_total, pair_total = total(row_sums), total(pair_sums)
    gram = np.zeros((d, d))
    gram[i, j] = pair_total
    if transposed_block:
        h = d // 2                                                    # block (1, 0) of the two halves: (i, j) <- (h + j, i - h)
        block = gram[h:2 * h, :h].copy()
        gram[h:2 * h, :h] = block.T
    squares = np.diagonal(gram)[:nr].copy()
    if square_of_next_parameter:
        squares = np.array([gram[(r + 1) % d, (r + 1) % d] for r in range(nr)])
    return _assemble(nr, nc, float(n), row_total[:d], gram, row_total[d:d + nr], row_total[d + nr:], np.float64, squares)


MODELS = {"f32_sequential": dict(dtype="f32", order="sequential"), "f32_pairwise": dict(dtype="f32", order="pairwise"),
          "f64": dict(dtype="f64", order="matmul")}

# planted defects: name -> (keyword arguments of model_moments, what catches it: "integers" | "wide_integers" | None)
DEFECTS = {
    "drop_last_of_ragged_tile": (dict(drop_last_of_ragged_tile=True), "integers"),
    "stale_prefetch": (None, "integers"),                              # needs the launch geometry: ``stale_prefetch_tiles``
    "tile64_where_32": (dict(tile=32, tile_stride=64), "integers"),
    "transposed_block": (dict(transposed_block=True), "integers"),
    "wrong_complex_pairing": (dict(wrong_complex_pairing=True), "integers"),
    "no_abs": (dict(no_abs=True), "integers"),
    "square_of_next_parameter": (dict(square_of_next_parameter=True), "integers"),
    "fp32_across_tiles": (dict(trips=np.float32), WIDE),               # needs the launch geometry: ``tiles_between_trips``
    "f32_sqrt_of_f32_squares": (dict(f32_sqrt_of_f32_squares=True), None),
}


# ---------------------------------------------------------------------------------------------------- launch geometry
GRAM32_ROWS = 256                                   # pool_reduce_blocks: partial rows (workgroups) of the small Gram kernels
GRAM32_WAVES = {"f32": 16, "f64": 8}                # wavefronts per workgroup, one tile each per trip
GRAM64_ROWS = 1024                                  # ... and of the 64-parameter ones: one wavefront per row


def chains(tiles):
    """The chain count the GPU module uses for ``tiles`` 64-chain tiles: a ragged last tile of 5 chains."""
    return 64 * tiles - 59


def gram32_second_trip_tiles(dtype):
    """Every wavefront of the 256 workgroups has a tile, the first workgroup's wavefronts a second one, and one more."""
    waves = GRAM32_WAVES[dtype]
    return GRAM32_ROWS * waves + waves + 1


def gram32_second_trip_chains(dtype):
    """263 173 chains in float32 (4 113 tiles), 131 653 in float64 (the 2 057 tiles and five chains of one more)."""
    tiles = gram32_second_trip_tiles(dtype)
    return chains(tiles) if dtype == "f32" else 64 * tiles + 5


def generic_rows(nr, nc):
    """pool_reduce_blocks' cap for the generic kernel: at most 32 MiB of partial sums, within 64 .. 1 024 rows."""
    d = nr + 2 * nc
    entries = 1 + d + nr + nc + d * (d + 1) // 2
    return int(min(1024, max(64, (32 << 20) // (8 * entries))))


def generic_tile(nr, nc, dtype):
    """pool_tile_chains: the widest of 64 / 32 / 16 chains whose augmented rows, pitch tile + 1, fit 160 KiB of LDS."""
    n_aug = 2 * nr + 3 * nc
    for tile in (64, 32, 16):
        if n_aug * (tile + 1) * (4 if dtype == "f32" else 8) <= 160 * 1024:
            return tile
    return 0


def partial_rows(path, nr, nc, n):
    """pool_reduce_blocks: one row of partial sums per 64-chain tile up to the path's cap."""
    cap = GRAM32_ROWS if path == "gram32" else GRAM64_ROWS if path == "gram64" else generic_rows(nr, nc)
    return max(1, min((n + 63) // 64, cap))


def tiles_between_trips(path, nr, nc, dtype, n):
    """The stride of the stage-1 tile loops: the wavefront (gram32: 16 / 8 per partial row; gram64: one per row) or block
    (generic) that starts at tile ``first`` goes on with first + k x this many, tiles of ``path_tile`` chains."""
    return partial_rows(path, nr, nc, n) * (GRAM32_WAVES[dtype] if path == "gram32" else 1)


def stale_prefetch_tiles(path, dtype, n, nr=0, nc=0):
    """(second-trip tile, the first-trip tile of the same wavefront) for the defect, or None without a second trip."""
    step = tiles_between_trips(path, nr, nc, dtype, n)
    return (step, 0) if (n + 63) // 64 > step else None


# ---------------------------------------------------------------------------------------------------- the cases
GRAM32_SETS = ((1, 0), (2, 0), (16, 0), (0, 4), (4, 4), (2, 1), (2, 2), (2, 7))
GRAM32_CHAINS = (1, 63, 65, 197, 64 * 16 + 5)      # the last: a workgroup whose last wavefronts have no tile
GRAM64_CHAINS = (1, 31, 65, 197, chains(GRAM64_ROWS + 3))
N_CLASS = 197


def conformance_cases():
    """Every (path, nr, nc, dtype, n, class) of the GPU module; the CPU module runs the models over the same list.
    ``path`` names the stage-1 kernel: gram32, gram64, generic64 (component-major, runtime dimensions), generic64_tiled
    (the on-demand (96, 0) set), generic32, generic16."""
    out = []
    for dtype in ("f32", "f64"):
        for nr, nc in GRAM32_SETS:
            out += [("gram32", nr, nc, dtype, n, name) for n in GRAM32_CHAINS for name in CLASSES]
        for nr, nc in ((2, 7), (16, 0)):
            out += [("gram32", nr, nc, dtype, gram32_second_trip_chains(dtype), name) for name in ("integers", "offset")]
        out += [("gram64", 64, 0, dtype, n, name) for n in GRAM64_CHAINS for name in (CLASSES if n == N_CLASS else CLASSES[:1])]
        for nr, nc in ((97, 0), (60, 25)):
            out += [("generic64", nr, nc, dtype, N_CLASS, name) for name in CLASSES]
        out += [("generic64_tiled", 96, 0, dtype, N_CLASS, name) for name in ("integers", "scaled")]
    # the block cap of (97, 0) is 847 rows: 850 tiles give the first three blocks a second tile
    out += [("generic64", 97, 0, "f64", chains(850), name) for name in ("integers", "offset")]
    for path, nr, dtype, few in (("generic32", 160, "f64", 33), ("generic32", 316, "f32", 33), ("generic16", 312, "f64", 17)):
        out += [(path, nr, 0, dtype, n, name) for n in (N_CLASS, few) for name in CLASSES]
    # float32 carried across a wavefront's / a block's tiles: wherever a float32 kernel has a second full 64-chain tile
    out += [("gram32", nr, nc, "f32", gram32_second_trip_chains("f32"), WIDE) for nr, nc in ((2, 7), (16, 0))]
    out += [("gram64", 64, 0, "f32", chains(GRAM64_ROWS + 3), WIDE)]
    out += [("generic64", 97, 0, "f32", chains(850), name) for name in ("integers", WIDE)]
    return out


def path_family(path, dtype):
    return "fp32_mfma" if path.startswith("gram") and dtype == "f32" else "generic"


def path_tile(path, nr, nc, dtype):
    """Chains per tile of the path's stage-1 kernel (64 for the Gram kernels)."""
    return 64 if path.startswith("gram") else generic_tile(nr, nc, dtype)
