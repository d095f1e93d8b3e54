"""Long-double reference, per-value forward-error bound, input classes and a numpy model (with planted defects) of the two
links of a step that no other conformance module holds: the per-chain proposal ``x' = x + w L g`` and the built-in energies
``E(x')`` (plain numpy, vectorised over chains; no GPU).  Used by tests/test_proposal_reference_cpu.py and
tests/test_gpu_proposal_conformance.py.

The proposal.  The packed factor row of a chain (csrc/me_device.h: ``tri``, ``cre``, ``cim``, ``cdiag``, restated below) is
the real triangle, row-major, then for every row i of the Hermitian block (Re, Im) of the columns j < i and the real
diagonal.  With zeta_j = (g_re_j + i g_im_j) fl(1/sqrt 2):

    real row i       x'_i = x_i + w_r sum_{j <= i} L_ij g_j
    Hermitian row i  z'_i = z_i + w_c sum_{j <= i} L_ij zeta_j:  are += lre wre - lim wim,  aim += lre wim + lim wre

Every coordinate is returned as (S, A): the exact value and the sum of the absolute values of its terms,
|x_i| + |w| sum |L_ij| |g_j| (four real products per column of the Hermitian block).

The criterion.  |got - S| <= gamma_k(u) A, gamma_k = k u / (1 - k u), u the unit roundoff of the engine's dtype, k the largest
number of roundings a term can pass through on its way into the result -- counted from each spelling (``k_proposal``), one
per product, addition, fused multiply-add and host-rounded constant; a contraction the compiler is free to make can only
lower the count of the spellings that leave it the choice, and the count allows every choice it has:

    registers   propose_registers (CK_PER_CHAIN, CK_PER_CHAIN_NT, CK_SHARED; inside k_step, k_cycle) and the streamed-factor
                body of k_step, which spells the same arithmetic term by term.
                Real row i: ``acc += L_ij g_j`` for j = 0 .. i, then ``x_i + w_r acc``.  The term of column 0 carries its
                product (1), the i additions of the later columns, the product with w_r (1) and the last addition (1):
                k = i + 3.  x_i itself carries 1.
                Hermitian row i: per column ``are += lre wre - lim wim``: a term carries its product (1), the subtraction
                (1) and the addition to the running sum (1), then at most 2 roundings per later column (one when the
                column's expression is formed first and added, two when it is contracted into two dependent fmas), the
                diagonal term's addition (1), the product with w_c (1) and the last addition (1): k = 3 + 2 (i - 1) + 3
                = 2 i + 4 (row 0: 3).  zeta's parts wre = fl(g fl(1/sqrt 2)) count as inputs where they are known bit for
                bit (the identity-shape engine hands them out, see below); where g itself is the input (step_injected)
                the product with fl(1/sqrt 2) is one more rounding: 2 i + 5.
    runtime     k_step_runtime_lds<CK_PER_CHAIN> works by columns with explicit fmas: x' starts as x, and every column j <= i
                adds ``fma(fl(w_r g_j), L_ij, x'_i)``.  x_i passes i + 1 fmas; the term of column 0 one more, its
                fl(w_r g_0): k = i + 2.
                Hermitian row i: every column j < i adds one fma per part of zeta_j to Re z'_i and to Im z'_i, the diagonal
                one: 2 i + 1 fmas on x.  A term carries sc = fl(fl(w_c fl(1/sqrt 2)) g) where the reference has
                w_c fl(g fl(1/sqrt 2)): three roundings apart (two when g itself is the input): k = 2 i + 4 (2 i + 3).
    magphase    k_step_magphase, magnitude stage: mag = sqrt(fma(re, re, im im)) (the radicand's two roundings are halved by
                the root, which is itself within 1 ulp = 2 u: 3), direction (re, im) fl(1 / mag) (mag's 3, the reciprocal
                within 1 ulp, the product: 6), mnew = mag + fl(fl(w w) K_jj) g (mag's 3 and the addition, or the three
                products and the addition: 4 on either term), z' = mnew direction (1).  Each part of z' is held against
                S (re, im) / |z| with S = |z| + w^2 K_jj g, A = |z| + |w^2 K_jj g| scaled by |re| / |z|, |im| / |z|:
                k = 4 + 6 + 1 = 11 (K_MAGPHASE).  |z| = 0 counts as the direction (1, 0).  Where the phase stage cannot be made
                to reject (no real parameter for a wall, no dense energy) the test injects the phase 0 and reads
                |z''| = sqrt(fma(re', re', im' im')) cos 0: the norm of z' within 11, the second root 3 more: 14
                (K_MAGPHASE_AFTER_PHASE).

The counts are derived from the spelling, never from a run.

How g is known.  A fresh identity-shape engine (cov_mode="fixed") of the same parameter space, seed, chain ids and step
counter, stepped once from x = 0 with the power-of-two width W and every proposal accepted, holds W g in the real
coordinates and W fl(g fl(1/sqrt 2)) in the complex ones, bit for bit (``x + w g`` from zero is one exact scaling; every
kernel family draws g with the same Num<R>::normal_pair on the same Philox words).

Energies (``energy_reference``), every term of the exact expression taken with its absolute value for A:

    iso        a (s0 + s1), two interleaved chains of ceil(D/2) squares: product, ceil(D/2) - 1 additions, s0 + s1, the
               product with a: k = ceil(D/2) + 2.
    diag       the same chains of (w_d x_d) x_d: two products, ceil(D/2) - 1 additions, s0 + s1: k = ceil(D/2) + 2.
    runtime    the streamed ``e += weight_of(d) x_d x_d`` of k_step_runtime, k_step_runtime_lds and k_init_energy_runtime
               (iso and diag alike): two products and D - 1 additions: k = D + 1.
    landau     T1 = k (1 - x)^2, T2 = k (1 - y)^2, T3 = x y alpha |c|^2, T4 = x y beta |c|^4, |c|^2 = fma(x2, x2, x3 x3) within
               2 u (both squares positive).  ``fma(x y, fma(beta a2, a2, alpha a2), fma(k ox, ox, k oy oy))``, ox = fl(1 - x)
               one rounding OF THE DIFFERENCE (a term is k (1 - x)^2, not its expansion):
               T1: ox twice (2), k ox, inner fma, outer fma = 5;  T2: oy twice, k oy, (k oy) oy, inner fma, outer fma = 6;
               T3: x y, a2 (2), alpha a2, inner fma, outer fma = 6;  T4: x y, a2 twice (4), beta a2, inner fma, outer fma = 8.
               k = 8.
    landau_terms  row "field" = fl(x y) fma(beta a2, a2, alpha a2): T4 as above without the outer fma but with the last
               product: k = 8; row "area" = fma(k ox, ox, k oy oy): T2 without the outer fma: k = 5.
    cylinder   kappa s / (1 - x0^2) + sum_j (gamma + q_j^2 amp) |z_j|^2 + tot^2 / 2, s = sum x_i^2, amp = 1 + x0^2 / 2,
               q_j = wavenumber (j - (NC - 1)/2), tot = sum |z_j|^2.  The denominator: fl(x0^2) is off by u x0^2, which is
               u x0^2 / (1 - x0^2) of the difference -- 0.81 / 0.19 < 4.27 for |x0| <= 0.9 (CYLINDER_X0_MAX; the inputs stay
               inside) -- plus the subtraction's own rounding: 6 roundings' worth.  Surface term: s (1 + NR - 1), kappa s
               (1), the denominator (6), the division (1), the two final additions (2): NR + 10.  Field term j: q (1) twice
               and q q (1), amp (2) and the product (1), + gamma (1): 7; |z_j|^2 (2) and the product (1), NC - 1 additions
               of the running field, 2 final additions: NC + 11.  Quartic term: tot (2 + NC - 1) twice, the product, the
               last addition: 2 NC + 4.  k = max(NR + 10, NC + 11, 2 NC + 4).

Input classes, every value a number of the device dtype, a different value per chain and per coordinate:

    one_per_row  exact, every path, both dtypes: chain c has in every row i exactly one non-zero entry, at column
                 c mod (i + 1), of value +-2^s with s and the sign a function of the packed slot (``slot_code``); in the
                 Hermitian block the chains alternate between the Re slot and the Im slot of that column (c // (i + 1)
                 even / odd) and take the diagonal where the column is i.  From x = 0 with a power-of-two width every
                 coordinate of x' is one power of two times one identity-engine value, or the (-Im, Re) rotation of one: it
                 must come back EQUAL.  With max(nr, 2 nc - 1) chains every slot is the live one somewhere
                 (``one_per_row_coverage``).
    integers     float64 through step_injected: integer L, g, x below 2^10 with a power-of-two width.  The real rows are
                 exact in any order.  The Hermitian rows cannot be: fl(1/sqrt 2) is no dyadic fraction of a few bits, so
                 no choice of g makes sums of L zeta exact -- they are held to the bound (their exact class is one_per_row).
    scaled       random lower-triangular rows times 10^linspace(-2, 2) by row, x of order one, widths log-uniform over 10^+-3.
    cancelling   random rows and x = -fl(w L g): |S| is a rounding residual, |S| << A in every row, only a bound on A means
                 anything, and an fma-versus-product difference shows.
  energies: integers (small integer states and coefficients, E exact below 2^24; the cylinder with x0 = 0), scaled, and
  cancelling for the Landau forms (alpha < 0, x y < 0).

``model_proposal`` / ``model_energy`` restate honest device code in numpy (float32 with each fma as a float64 product-sum
rounded once, float64 through long double); ``PROPOSAL_DEFECTS`` / ``ENERGY_DEFECTS`` are planted in them.
"""
import numpy as np

LD = np.longdouble
UNIT_ROUNDOFF = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NUMPY_DTYPE = {"f32": np.float32, "f64": np.float64}
INV_SQRT2 = {"f32": float(np.float32(0.70710678118654752440)), "f64": 0.70710678118654752440}   # R(0.707...) of the kernels
STREAM_CHUNK = {"f32": 32, "f64": 16}          # ME_STREAM_CHUNK_BYTES / sizeof(R): entries per chunk of the streamed body
CYLINDER_X0_MAX = 0.9
CYLINDER_DENOMINATOR_FACTOR = 0.81 / 0.19       # x0^2 / (1 - x0^2) at |x0| = 0.9: < 4.27


def gamma(k, dtype):
    u = LD(UNIT_ROUNDOFF[dtype])
    k = np.asarray(k, dtype=LD)
    return k * u / (LD(1) - k * u)


def ratio(got, s, a, k, dtype):
    """|got - S| / (gamma_k A) per value in long double; a value with A = 0 must be 0 (ratio 0, else +inf); a non-finite
    value gives +inf.  Pass: ratio <= 1."""
    err = np.abs(np.asarray(got).astype(LD) - s)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / (gamma(k, dtype) * a))
    return np.where(np.isfinite(r), r, LD(np.inf))


def to_dtype(v, dtype):
    """Rounded to the device dtype, held as float64."""
    return np.asarray(v, dtype=np.float64).astype(NUMPY_DTYPE[dtype]).astype(np.float64)


# ------------------------------------------------------------------------------------------------------ packed layout
def tri(i, j):
    return i * (i + 1) // 2 + j


def cre(pr, i, j):
    return pr + i * i + 2 * j


def cim(pr, i, j):
    return pr + i * i + 2 * j + 1


def cdiag(pr, i):
    return pr + i * i + 2 * i


def packed_size(nr, nc):
    return nr * (nr + 1) // 2 + nc * nc


def n_width_rows(nr, nc):
    return 3 if nr and nc else 1


def unpack(rows, nr, nc):
    """(L_r [n, nr, nr], Re L_c [n, nc, nc], Im L_c [n, nc, nc]) of packed rows [n, P], lower triangles, in the rows' type."""
    rows = np.asarray(rows)
    n, pr = rows.shape[0], nr * (nr + 1) // 2
    assert rows.shape[1] == packed_size(nr, nc)
    lr = np.zeros((n, nr, nr), dtype=rows.dtype)
    lre, lim = np.zeros((n, nc, nc), dtype=rows.dtype), np.zeros((n, nc, nc), dtype=rows.dtype)
    for i in range(nr):
        lr[:, i, :i + 1] = rows[:, tri(i, 0):tri(i, 0) + i + 1]
    for i in range(nc):
        for j in range(i):
            lre[:, i, j] = rows[:, cre(pr, i, j)]
            lim[:, i, j] = rows[:, cim(pr, i, j)]
        lre[:, i, i] = rows[:, cdiag(pr, i)]
    return lr, lre, lim


def packed_identity(n, nr, nc):
    rows = np.zeros((n, packed_size(nr, nc)))
    rows[:, [tri(i, i) for i in range(nr)]] = 1.0
    rows[:, [cdiag(nr * (nr + 1) // 2, i) for i in range(nc)]] = 1.0
    return rows


# ------------------------------------------------------------------------------------------------------ the reference
def widths_used(width, nr, nc):
    """(w_r, w_c) [n] of a width field [n, 1] or [n, 3]: a mixed engine whose widths were loaded uses its group rows."""
    width = np.asarray(width)
    return (width[:, 1], width[:, 2]) if width.shape[1] == 3 else (width[:, 0], width[:, 0])


def proposal_reference(x, w_r, w_c, rows, g, zre, zim, nr, nc, group="all"):
    """(S, A) [n, D] in long double.  g [n, nr]: the real block's normals; zre, zim [n, nc]: the parts of zeta (already
    times fl(1/sqrt 2)).  group: "all", "real" or "complex" -- a resting coordinate is S = x, A = |x|."""
    x = np.asarray(x).astype(LD)
    lr, lre, lim = unpack(np.asarray(rows).astype(LD), nr, nc)
    s, a = x.copy(), np.abs(x)
    if nr and group != "complex":
        w = np.asarray(w_r).astype(LD)[:, None]
        g = np.asarray(g).astype(LD)
        s[:, :nr] += w * np.einsum("nij,nj->ni", lr, g)
        a[:, :nr] += np.abs(w) * np.einsum("nij,nj->ni", np.abs(lr), np.abs(g))
    if nc and group != "real":
        w = np.asarray(w_c).astype(LD)[:, None]
        zre, zim = np.asarray(zre).astype(LD), np.asarray(zim).astype(LD)
        mv = lambda m, v: np.einsum("nij,nj->ni", m, v)
        s[:, nr:nr + nc] += w * (mv(lre, zre) - mv(lim, zim))
        s[:, nr + nc:] += w * (mv(lre, zim) + mv(lim, zre))
        alre, alim, azre, azim = np.abs(lre), np.abs(lim), np.abs(zre), np.abs(zim)
        a[:, nr:nr + nc] += np.abs(w) * (mv(alre, azre) + mv(alim, azim))
        a[:, nr + nc:] += np.abs(w) * (mv(alre, azim) + mv(alim, azre))
    return s, a


def k_proposal(spelling, nr, nc, raw_normals=False):
    """[D] roundings per coordinate; see the module docstring for the derivation.  raw_normals: g itself is the input of
    the Hermitian block (step_injected), not fl(g fl(1/sqrt 2))."""
    i, j = np.arange(nr), np.arange(nc)
    if spelling == "registers":
        kr = i + 3                            # product, i additions, w_r acc, x + .
        kc = 2 * j + 4 + int(raw_normals)     # 3 for the column's own expression, 2 per later column, diagonal, w_c, x + .
    elif spelling == "runtime":
        kr = i + 2                            # fl(w_r g), i + 1 fmas
        kc = 2 * j + 1 + (2 if raw_normals else 3)     # 2 i + 1 fmas, sc against w_c zeta
    else:
        raise KeyError(spelling)
    return np.concatenate((kr, kc, kc))


K_MAGPHASE = 11               # each part of z' after the magnitude stage
K_MAGPHASE_AFTER_PHASE = 14   # |z''| after an accepted phase stage at phase 0


def magphase_reference(x, w, kdiag, g, nr, nc):
    """(S, A, direction) of the magnitude stage: S, A [n, nc] of the new magnitudes |z_j| + (w^2 K_jj) g_j, and the parts
    (re, im) / |z| [n, 2 nc] of the direction that is kept ((1, 0) where |z| = 0).  Part p of z' is S dir_p within
    gamma_11 A |dir_p|."""
    x = np.asarray(x).astype(LD)
    re, im = x[:, nr:nr + nc], x[:, nr + nc:]
    mag = np.hypot(re, im)
    safe = np.where(mag > 0, mag, LD(1))
    direction = np.concatenate((np.where(mag > 0, re / safe, LD(1)), np.where(mag > 0, im / safe, LD(0))), axis=1)
    t = (np.asarray(w).astype(LD) ** 2)[:, None] * np.asarray(kdiag).astype(LD) * np.asarray(g).astype(LD)
    return mag + t, mag + np.abs(t), direction


# ------------------------------------------------------------------------------------------------------ arithmetic model
class Arith:
    """Honest device arithmetic: values of the dtype; a fused multiply-add is the product-sum in a wider type rounded once
    (float64 for float32 -- the product of two floats is exact there; long double for float64)."""

    def __init__(self, dtype):
        self.t = NUMPY_DTYPE[dtype]
        self.wide = np.float64 if dtype == "f32" else LD

    def fl(self, v):
        return np.asarray(v, dtype=self.wide).astype(self.t)

    def w(self, v):
        return np.asarray(v, dtype=self.t).astype(self.wide)

    def mul(self, a, b):
        return self.fl(self.w(a) * self.w(b))

    def add(self, a, b):
        return self.fl(self.w(a) + self.w(b))

    def sub(self, a, b):
        return self.fl(self.w(a) - self.w(b))

    def div(self, a, b):
        return self.fl(self.w(a) / self.w(b))

    def fma(self, a, b, c):
        return self.fl(self.w(a) * self.w(b) + self.w(c))


# defect -> the spelling it is planted in
PROPOSAL_DEFECTS = {
    "transposed_real_slot": "registers",        # L_ij read at tri(j, i)
    "chunk_parity": "registers",                # the streamed body: slot k read as k +- CH (the wrong one of the two buffers)
    "re_im_swapped": "registers",
    "conj_l": "registers",
    "no_sqrt2_on_diagonal": "registers",
    "real_width_on_complex": "registers",
    "neighbour_chain_row": "registers",
    "im_part_sign": "runtime",                  # (lr + i li)(i sc): + li sc instead of - li sc
    "real_tail_drops_last_row": "runtime",      # the row tail of the real columns ends one row early when nr mod 4 = 1
    "complex_batch_starts_late": "runtime",     # the 8-row batch of a complex column starts at row j + 2
}


def model_proposal(spelling, x, w_r, w_c, rows, g, nr, nc, dtype, group="all", defect=None):
    """x' [n, D] (float64 holding values of the dtype) as honest code of the spelling forms it.  g [n, D]: the raw normals of
    every coordinate.  ``defect``: one of PROPOSAL_DEFECTS, planted whatever the spelling it is listed under."""
    ar = Arith(dtype)
    t = ar.t
    x, rows, g = np.asarray(x, dtype=t), np.asarray(rows, dtype=t), np.asarray(g, dtype=t)
    w_r, w_c = np.asarray(w_r, dtype=t), np.asarray(w_c, dtype=t)
    n, pr, p = x.shape[0], nr * (nr + 1) // 2, packed_size(nr, nc)
    c = t(INV_SQRT2[dtype])
    ch = STREAM_CHUNK[dtype]
    if defect == "neighbour_chain_row":
        rows = np.roll(rows, -1, axis=0)
    if defect == "real_width_on_complex":
        w_c = w_r

    def fac(k):
        if defect == "chunk_parity" and k >= ch:
            k = k + ch if k + ch < p else k - ch
        return rows[:, k]

    def pair(i, j):
        lre, lim = fac(cre(pr, i, j)), fac(cim(pr, i, j))
        if defect == "re_im_swapped":
            lre, lim = lim, lre
        if defect == "conj_l":
            lim = -lim
        return lre, lim

    xp = x.copy()
    move_real, move_complex = nr > 0 and group != "complex", nc > 0 and group != "real"
    if spelling == "registers":
        if move_real:
            for i in range(nr):
                acc = np.zeros(n, dtype=t)
                for j in range(i + 1):
                    k = tri(j, i) if defect == "transposed_real_slot" and j < i else tri(i, j)
                    acc = ar.fma(fac(k), g[:, j], acc)
                xp[:, i] = ar.fma(w_r, acc, x[:, i])
        if move_complex:
            wre, wim = ar.mul(g[:, nr:nr + nc], c), ar.mul(g[:, nr + nc:], c)
            for i in range(nc):
                are, aim = np.zeros(n, dtype=t), np.zeros(n, dtype=t)
                for j in range(i):
                    lre, lim = pair(i, j)
                    are = ar.add(are, ar.fma(lre, wre[:, j], -ar.mul(lim, wim[:, j])))
                    aim = ar.add(aim, ar.fma(lre, wim[:, j], ar.mul(lim, wre[:, j])))
                ld = fac(cdiag(pr, i))
                if defect == "no_sqrt2_on_diagonal":
                    are, aim = ar.fma(ld, g[:, nr + i], are), ar.fma(ld, g[:, nr + nc + i], aim)
                else:
                    are, aim = ar.fma(ld, wre[:, i], are), ar.fma(ld, wim[:, i], aim)
                xp[:, nr + i] = ar.fma(w_c, are, x[:, nr + i])
                xp[:, nr + nc + i] = ar.fma(w_c, aim, x[:, nr + nc + i])
    elif spelling == "runtime":
        if move_real:
            for db in range(0, nr, 4):
                sg = [ar.mul(w_r, g[:, db + u]) if db + u < nr else np.zeros(n, dtype=t) for u in range(4)]
                for i in range(db, nr):
                    if defect == "real_tail_drops_last_row" and nr % 4 == 1 and i == nr - 1 and i >= db + 4:
                        continue
                    for u in range(min(4, i - db + 1)):
                        k = tri(db + u, i) if defect == "transposed_real_slot" and db + u < i else tri(i, db + u)
                        xp[:, i] = ar.fma(sg[u], fac(k), xp[:, i])
        if move_complex:
            s_c = ar.mul(w_c, c)
            zre, zim = xp[:, nr:nr + nc], xp[:, nr + nc:]          # (views)
            for im_part in (False, True):
                for j in range(nc):
                    raw = g[:, nr + nc + j] if im_part else g[:, nr + j]
                    sc = ar.mul(s_c, raw)
                    own = zim if im_part else zre
                    sd = ar.mul(w_c, raw) if defect == "no_sqrt2_on_diagonal" else sc
                    own[:, j] = ar.fma(sd, fac(cdiag(pr, j)), own[:, j])
                    first = j + 1
                    if defect == "complex_batch_starts_late" and first + 8 <= nc:
                        first += 1
                    for i in range(first, nc):
                        lr_, li_ = pair(i, j)
                        minus = -sc if defect != "im_part_sign" else sc
                        zre[:, i] = ar.fma(minus if im_part else sc, li_ if im_part else lr_, zre[:, i])
                        zim[:, i] = ar.fma(sc, lr_ if im_part else li_, zim[:, i])
    else:
        raise KeyError(spelling)
    return xp.astype(np.float64)


def model_magphase(x, w, kdiag, g, nr, nc, dtype):
    """|z'| parts [n, 2 nc] of the magnitude stage as honest code forms them (the square root correctly rounded)."""
    ar = Arith(dtype)
    t = ar.t
    x, w, kdiag, g = (np.asarray(v, dtype=t) for v in (x, w, kdiag, g))
    out = np.empty((x.shape[0], 2 * nc))
    for j in range(nc):
        re, im = x[:, nr + j], x[:, nr + nc + j]
        mag = ar.fl(np.sqrt(ar.w(ar.fma(re, re, ar.mul(im, im)))))
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(mag > 0, ar.div(t(1), np.where(mag > 0, mag, t(1))), t(0))
        dre, dim = np.where(mag > 0, ar.mul(re, inv), t(1)), np.where(mag > 0, ar.mul(im, inv), t(0))
        mnew = ar.fma(ar.mul(ar.mul(w, w), kdiag[:, j]), g[:, j], mag)
        out[:, j], out[:, nc + j] = ar.mul(mnew, dre), ar.mul(mnew, dim)
    return out


# ------------------------------------------------------------------------------------------------------ proposal inputs
def split_normals(g, nr, nc, dtype):
    """(g_r, zre, zim) of raw normals [n, D]: zeta's parts as the kernels form them, fl(g fl(1/sqrt 2))."""
    ar = Arith(dtype)
    c = ar.t(INV_SQRT2[dtype])
    g = np.asarray(g, dtype=ar.t)
    return (g[:, :nr].astype(np.float64), ar.mul(g[:, nr:nr + nc], c).astype(np.float64),
            ar.mul(g[:, nr + nc:], c).astype(np.float64))


def slot_code(k):
    """+-2^s, s in -4 .. 4, of packed slot k: consecutive slots differ in s, and so do a slot and the one a row or a
    chunk on in all but a few places."""
    k = np.asarray(k, dtype=np.int64)
    h = (k * 7 + (k // 9) * 4 + (k // 81)) % 18
    return np.where(h >= 9, -1.0, 1.0) * 2.0 ** (h % 9 - 4)


def one_per_row(n, nr, nc):
    """Packed rows [n, P]: in chain c every row has ONE non-zero entry, slot_code of its slot (see the module docstring)."""
    pr = nr * (nr + 1) // 2
    rows = np.zeros((n, packed_size(nr, nc)))
    c = np.arange(n)
    for i in range(nr):
        k = tri(i, c % (i + 1))
        rows[c, k] = slot_code(k)
    for i in range(nc):
        col, odd = c % (i + 1), (c // (i + 1)) % 2
        k = np.where(col == i, cdiag(pr, i), cre(pr, i, col) + odd)
        rows[c, k] = slot_code(k)
    return rows


def one_per_row_coverage(n, nr, nc):
    """[P] bool: the slot is the live one in at least one chain."""
    return (one_per_row(n, nr, nc) != 0).any(axis=0)


def one_per_row_expected(rows, ident, nr, nc, group="all", x=None):
    """x' [n, D] that must come back EQUAL: ``ident`` [n, D] is the identity-shape engine's state (w g, w zeta parts); every
    sum below has one non-zero term, a power of two times a number of the dtype -- exact in float64."""
    lr, lre, lim = unpack(rows, nr, nc)
    out = np.zeros(ident.shape) if x is None else np.array(x, dtype=np.float64)
    mv = lambda m, v: np.einsum("nij,nj->ni", m, v)
    if nr and group != "complex":
        out[:, :nr] = mv(lr, ident[:, :nr])
    if nc and group != "real":
        ire, iim = ident[:, nr:nr + nc], ident[:, nr + nc:]
        out[:, nr:nr + nc] = mv(lre, ire) - mv(lim, iim)
        out[:, nr + nc:] = mv(lre, iim) + mv(lim, ire)
    return out


def random_rows(n, nr, nc, rng, scale_by_row=True):
    """Random lower-triangular rows [n, P], a different one per chain; entries times 10^linspace(-2, 2) by row."""
    pr = nr * (nr + 1) // 2
    rows = rng.standard_normal((n, packed_size(nr, nc)))
    if scale_by_row:
        sr, sc = 10.0 ** np.linspace(-2, 2, nr), 10.0 ** np.linspace(-2, 2, nc)
        for i in range(nr):
            rows[:, tri(i, 0):tri(i, 0) + i + 1] *= sr[i]
        for i in range(nc):
            rows[:, pr + i * i:pr + (i + 1) * (i + 1)] *= sc[i]
    return rows


def scaled_case(n, nr, nc, dtype, seed):
    """(x [n, D], width [n, rows], packed rows [n, P]) of class ``scaled``."""
    rng = np.random.default_rng([seed, nr, nc, n])
    rows = random_rows(n, nr, nc, rng)
    x = rng.standard_normal((n, nr + 2 * nc))
    width = 10.0 ** rng.uniform(-3, 3, (n, n_width_rows(nr, nc)))
    return to_dtype(x, dtype), to_dtype(width, dtype), to_dtype(rows, dtype)


def cancelling_case(n, nr, nc, dtype, seed, g, zre, zim):
    """Class ``cancelling`` for these normals: random rows of order one, widths in [1/4, 4], x = -fl(w L g)."""
    rng = np.random.default_rng([seed, nr, nc, n, 1])
    rows = to_dtype(random_rows(n, nr, nc, rng, scale_by_row=False), dtype)
    width = to_dtype(2.0 ** rng.uniform(-2, 2, (n, n_width_rows(nr, nc))), dtype)
    w_r, w_c = widths_used(width, nr, nc)
    s, _ = proposal_reference(np.zeros((n, nr + 2 * nc)), w_r, w_c, rows, g, zre, zim, nr, nc)
    return to_dtype(-np.asarray(s, dtype=np.float64), dtype), width, rows


def integers_case(n, nr, nc, seed):
    """(x, width, rows, g) of class ``integers``: every value an integer below 2^10, widths powers of two (another per
    group row)."""
    rng = np.random.default_rng([seed, nr, nc, n, 2])
    rows = rng.integers(-9, 10, (n, packed_size(nr, nc))).astype(np.float64)
    x = rng.integers(-500, 501, (n, nr + 2 * nc)).astype(np.float64)
    g = rng.integers(-31, 32, (n, nr + 2 * nc)).astype(np.float64)
    width = np.tile(2.0 ** -np.arange(1, 1 + n_width_rows(nr, nc)), (n, 1)) * 2.0 ** rng.integers(0, 3, (n, 1))
    return x, width, rows, g


# ------------------------------------------------------------------------------------------------------ energies
ENERGY_KINDS = ("iso", "diag", "landau", "landau_terms", "cylinder")


def diag_weights(a, b):
    """The D weights of DiagQuadratic(a, b): real, then the complex weights twice."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return np.concatenate((a, b, b))


def k_energy(kind, nr, nc, runtime=False):
    d = nr + 2 * nc
    if kind in ("iso", "diag"):
        return d + 1 if runtime else (d + 1) // 2 + 2
    if kind == "landau":
        return 8
    if kind == "landau_terms":
        return np.array([8, 5])
    if kind == "cylinder":
        return max(nr + 10, nc + 11, 2 * nc + 4)
    raise KeyError(kind)


def energy_reference(kind, x, nr, nc, coeffs):
    """(S, A) in long double, [n] ([n, 2] for landau_terms: rows "field", "area").  coeffs: iso (a,), diag the D weights,
    landau / landau_terms (k, alpha, beta), cylinder (kappa, gamma, wavenumber)."""
    x = np.asarray(x).astype(LD)
    cf = np.asarray(coeffs).astype(LD)
    if kind == "iso":
        t = cf[0] * x * x
        return t.sum(axis=1), np.abs(t).sum(axis=1)
    if kind == "diag":
        t = cf[None, :] * x * x
        return t.sum(axis=1), np.abs(t).sum(axis=1)
    if kind in ("landau", "landau_terms"):
        assert (nr, nc) == (2, 1)
        k, alpha, beta = cf
        a2 = x[:, 2] ** 2 + x[:, 3] ** 2
        t1, t2 = k * (1 - x[:, 0]) ** 2, k * (1 - x[:, 1]) ** 2
        t3, t4 = x[:, 0] * x[:, 1] * alpha * a2, x[:, 0] * x[:, 1] * beta * a2 * a2
        if kind == "landau":
            return t1 + t2 + t3 + t4, np.abs(t1) + np.abs(t2) + np.abs(t3) + np.abs(t4)
        return np.stack((t3 + t4, t1 + t2), axis=1), np.stack((np.abs(t3) + np.abs(t4), np.abs(t1) + np.abs(t2)), axis=1)
    if kind == "cylinder":
        assert nr >= 1 and nc >= 1 and np.all(np.abs(x[:, 0]) <= CYLINDER_X0_MAX)
        kappa, gam, wavenumber = cf
        x0 = x[:, 0]
        surface = kappa * (x[:, :nr] ** 2).sum(axis=1) / (1 - x0 * x0)
        amp = 1 + x0 * x0 / 2
        q = wavenumber * (np.arange(nc).astype(LD) - LD(nc - 1) / 2)
        mod2 = x[:, nr:nr + nc] ** 2 + x[:, nr + nc:] ** 2
        gterm, qterm = gam * mod2, (q * q)[None, :] * amp[:, None] * mod2
        tot = mod2.sum(axis=1)
        s = surface + gterm.sum(axis=1) + qterm.sum(axis=1) + tot * tot / 2
        a = np.abs(surface) + np.abs(gterm).sum(axis=1) + qterm.sum(axis=1) + tot * tot / 2
        return s, a
    raise KeyError(kind)


ENERGY_DEFECTS = {"dropped_odd_tail": ("iso", "diag"), "weight_shifted_by_one": ("diag",), "beta_a2_for_beta_a2_squared": ("landau", "landau_terms")}


def model_energy(kind, x, nr, nc, coeffs, dtype, runtime=False, defect=None):
    """The functors of csrc/me_device.h (and, ``runtime``, the streamed loop of csrc/me_runtime_dims.hip) as honest code."""
    ar = Arith(dtype)
    t = ar.t
    x, cf = np.asarray(x, dtype=t), np.asarray(coeffs, dtype=t)
    n, d = x.shape[0], nr + 2 * nc
    if kind in ("iso", "diag"):
        wts = np.full(d, cf[0], dtype=t) if kind == "iso" else cf
        if defect == "weight_shifted_by_one":
            wts = np.roll(wts, -1)
        if runtime:
            e = np.zeros(n, dtype=t)
            for k in range(d):
                e = ar.fma(ar.mul(wts[k], x[:, k]), x[:, k], e)
            return e.astype(np.float64)
        s = [np.zeros(n, dtype=t), np.zeros(n, dtype=t)]
        for k in range(d - (1 if defect == "dropped_odd_tail" and d % 2 else 0)):
            s[k % 2] = ar.fma(x[:, k] if kind == "iso" else ar.mul(wts[k], x[:, k]), x[:, k], s[k % 2])
        e = ar.add(s[0], s[1])
        return (ar.mul(cf[0], e) if kind == "iso" else e).astype(np.float64)
    if kind in ("landau", "landau_terms"):
        k, alpha, beta = cf
        a2 = ar.fma(x[:, 2], x[:, 2], ar.mul(x[:, 3], x[:, 3]))
        ox, oy = ar.sub(t(1), x[:, 0]), ar.sub(t(1), x[:, 1])
        quartic = ar.mul(beta, a2)
        field = ar.add(quartic, ar.mul(alpha, a2)) if defect == "beta_a2_for_beta_a2_squared" else ar.fma(quartic, a2, ar.mul(alpha, a2))
        area = ar.fma(ar.mul(k, ox), ox, ar.mul(ar.mul(k, oy), oy))
        xy = ar.mul(x[:, 0], x[:, 1])
        if kind == "landau":
            return ar.fma(xy, field, area).astype(np.float64)
        return np.stack((ar.mul(xy, field), area), axis=1).astype(np.float64)
    if kind == "cylinder":
        kappa, gam, wavenumber = cf
        s = np.zeros(n, dtype=t)
        for i in range(nr):
            s = ar.fma(x[:, i], x[:, i], s)
        x0 = x[:, 0]
        surface = ar.div(ar.mul(kappa, s), ar.fma(-x0, x0, t(1)))
        amp = ar.fma(ar.mul(t(0.5), x0), x0, t(1))
        field, tot = np.zeros(n, dtype=t), np.zeros(n, dtype=t)
        for j in range(nc):
            q = ar.mul(wavenumber, t(j - (nc - 1) * 0.5))
            mod2 = ar.fma(x[:, nr + j], x[:, nr + j], ar.mul(x[:, nr + nc + j], x[:, nr + nc + j]))
            field = ar.fma(ar.fma(ar.mul(q, q), amp, gam), mod2, field)
            tot = ar.add(tot, mod2)
        return ar.fma(ar.mul(t(0.5), tot), tot, ar.add(surface, field)).astype(np.float64)
    raise KeyError(kind)


ENERGY_CLASSES = ("integers", "scaled", "cancelling")


def energy_case(kind, name, n, nr, nc, dtype, seed):
    """(x [n, D], coeffs) of an energy input class; ``cancelling`` exists for the Landau forms only."""
    rng = np.random.default_rng([seed, nr, nc, n, ENERGY_KINDS.index(kind), ENERGY_CLASSES.index(name)])
    d = nr + 2 * nc
    if name == "integers":
        x = rng.integers(1, 5, (n, d)) * rng.choice([-1.0, 1.0], (n, d))     # no zeros: x' = x bit for bit at a tiny width
        if kind == "iso":
            cf = np.array([3.0])
        elif kind == "diag":
            cf = diag_weights(1 + np.arange(nr) % 7, 1 + (3 + np.arange(nc)) % 5)
        elif kind in ("landau", "landau_terms"):
            cf = np.array([2.0, -3.0, 5.0])
        else:
            cf = np.array([3.0, 2.0, 2.0])                     # wavenumber 2: q_j = 2 j - (NC - 1), an integer
            x[:, 0] = 0.0                                      # the denominator is 1, amp is 1
        return x, cf
    if name == "scaled":
        x = rng.standard_normal((n, d)) * 10.0 ** rng.permutation(np.linspace(-2, 2, d))
        if kind == "iso":
            cf = np.array([0.7])
        elif kind == "diag":
            cf = diag_weights(10.0 ** rng.uniform(-2, 2, nr), 10.0 ** rng.uniform(-2, 2, nc))
        elif kind in ("landau", "landau_terms"):
            cf = np.array([1.3, -1.1, 0.45])
        else:
            cf = np.array([1.7, 0.3, 0.9])
            x[:, 0] = rng.uniform(-CYLINDER_X0_MAX, CYLINDER_X0_MAX, n)
            x[:, 0] = np.clip(to_dtype(x[:, 0], dtype), -0.899, 0.899)
        return to_dtype(x, dtype), to_dtype(cf, dtype)
    if name == "cancelling":
        assert kind in ("landau", "landau_terms")
        x = rng.uniform(0.5, 2.0, (n, d)) * rng.choice([-1.0, 1.0], (n, d))
        x[:, 1] = -np.sign(x[:, 0]) * np.abs(x[:, 1])          # x y < 0
        return to_dtype(x, dtype), to_dtype(np.array([1.0, -2.5, 0.8]), dtype)       # alpha < 0
    raise KeyError(name)
