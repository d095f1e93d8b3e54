"""Long-double reference, forward-error bound and arithmetic model for the dense matrix-core products (plain numpy,
vectorised over chains; no GPU).  Used by tests/test_dense_product_reference_cpu.py and
tests/test_gpu_dense_product_conformance.py.

The products.  Five kernels evaluate the dense quadratic form ``E = x^T (A x)`` and, with a shared proposal factor,
``y = L g``: k_step_dense64_bf16x3 (me_dense_bf16x3.h), k_step_dense64_mfma (me_dense_mfma.h), k_step_dense64_f64
(me_dense_f64.h), tri_rows_mfma inside k_step_runtime_lds (me_runtime_dims.hip) and the generic EnergyDense on the folded
triangle in LDS (me_device.h).

The criterion.  With u the unit roundoff of the kernel's type (2^-24, 2^-53), every kernel must satisfy, chain by chain,

    |E_kernel - E|  <=  gamma * sum_ij |x_i| |A_ij| |x_j|          (``abs_form``)
    |y_kernel - y|_i <=  gamma_L * (|L| |g|)_i                      (``abs_matvec``)

in ANY order of summation.  gamma counts, for one term ``x_i A_ij x_j`` of the sum, the relative perturbations it can pick
up on its way into the result (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: a term that
passes through k roundings carries a factor (1 + theta_k), |theta_k| <= gamma_k = k u / (1 - k u)).  Three sources:

  (1) The split (bf16x3 only).  ``bf16_head`` keeps the top 16 bits of a float: sign, exponent and 8 significant bits,
      by truncation.  For v in [2^e, 2^(e+1)): v1 holds bits e .. e-7, the remainder r1 = v - v1 < 2^(e-7) is exact;
      v2 holds the top 8 significant bits of r1, whose leading bit is at most e-8, so r2 = r1 - v2 < 2^(e-15); v3 the top 8
      of r2.  3 x 8 = 24: v = v1 + v2 + v3 EXACTLY for every normal float (leading zeros only move later pieces down), and

          |v1| <= |v|,    |v2| < 2^-7 |v|,    |v3| < 2^-15 |v|.

      The kernel keeps the six products M_a X_b with a + b <= 4 and neglects M2 X3 + M3 X2 + M3 X3, bounded by

          (2^-7 2^-15 + 2^-15 2^-7 + 2^-15 2^-15) |M| |X|  =  (2^-21 + 2^-30) |M| |X|  ~  8 u |M| |X|.

      The supremum is approached by operands of the form 1.0000000 1111111 1... (a zero field under the leading bit, then
      ones); operands with every mantissa bit set sit at 2^-8 and 2^-16 per piece, a neglected 2 u.  (The kernel header used
      to claim 2^-24; it now states this bound.)  Products of two 8-bit pieces are exact in float32.

  (2) The accumulation.  A matrix instruction computes D = C + sum_{k<K} a_k b_k.  What is documented: the products are
      exact for bf16 inputs; the order and the internal rounding of the K-term sum are not specified for any shape (the
      float32-input instruction behaves like a k-ordered fma chain on the classes measured so far; nothing here rests
      on it).  The model behind the bound: the K products are summed in some order, each of the K - 1 additions with a
      relative error of at most u' = 2 u (a correctly rounded or a truncated addition), and the result is added to C
      with one more such error.  A product of the first instruction of an accumulator's chain then carries at most
      (K - 1) + n_acc perturbations of size u', n_acc being the number of instructions that accumulate into that
      register:

          bf16x3, 32x32x16:      K = 16, n_acc = 4 k-steps x 6 products = 24          -> 39 u' = 78 u
          float32 32x32x2:       K = 2,  n_acc = 32                                   -> 33 u' = 66 u
          float64 16x16x4 (64):  K = 4,  n_acc <= 16 (row block mb: 4 (mb + 1))       -> 19 u' = 38 u
          runtime 16x16x4 (D):   K = 4,  n_acc <= 4 ceil(D / 16)                      -> (3 + 4 ceil(D/16)) u'
          generic triangle (D):  no matrix instruction: y_i is a chain of <= D products and additions, each rounded
                                 unless fused                                         -> (D + 1) u

      The folded kernels (float64 dense-64, runtime, generic) first form T_ij = A_ij + A_ji in working precision: one more u.

  (3) The final dot E = sum_i x_i y_i: D multiply-adds.  Whether ``e += x * y`` becomes one fma is the compiler's choice row
      by row (the shipped split-bf16 kernel fuses most rows and leaves the others as a packed multiply and an add), so a
      term counts the rounding of its own product and at most D additions: D + 1 (the kernels' partial sums over lanes are
      shallower).

  gamma = s (1 + g) + g,  g = k u / (1 - k u),  k the count of (2) + (3) in units of u, s the split term of (1) or 0.
  gamma_L is the same without (3) and without the fold.

``gamma_units`` / ``gamma`` give one value per kernel family: derived, not measured.

The calibrated cap.  gamma is a worst case over orders and signs, a factor of ~50 above what honest code does on random
data, and a split kernel that silently dropped one of its six products would still pass it.  ``split_bf16_energy``
restates wave_matmul_64_bf16x3's arithmetic -- truncation pieces, the six retained products per 16-column step in the
kernel's order, float32 accumulators, the float32 dot in the kernel's row order -- with the 16 products of one instruction
exact and summed exactly, one rounding per instruction.  It models only what the source and the instruction set
documentation state; it is never fitted to device output.  Planted defects of the same function (``DEFECTS``;
``FACTOR_DEFECTS`` for L g) give, per input class and on the same inputs, ``r_def`` (largest error / abs_form of the MILDEST defect) beside ``r_ref`` (the honest model); the cap is their
geometric mean sqrt(r_ref r_def): no constant is written down, and the CPU test asserts that the two are far enough apart
for the cap to separate them.
"""
import numpy as np

LD = np.longdouble

UNIT_ROUNDOFF = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NUMPY_DTYPE = {"f32": np.float32, "f64": np.float64}

SPLIT_TERM = 2.0 ** -21 + 2.0 ** -30          # (1): |M2||X3| + |M3||X2| + |M3||X3| <= SPLIT_TERM |M||X|


# ---------------------------------------------------------------------------------------------------- the bound
def gamma_units(family, d):
    """(roundings a term of E can pass through, the same for a component of L g), in units of u; see the docstring."""
    blocks = (d + 15) // 16
    if family == "bf16x3":
        acc, fold, dot = 2 * (15 + 24), 0, d + 1
    elif family == "fp32_mfma":
        acc, fold, dot = 2 * (1 + 32), 0, d + 1
    elif family == "f64_mfma":
        acc, fold, dot = 2 * (3 + 16), 1, d + 1
    elif family == "runtime":
        acc, fold, dot = 2 * (3 + 4 * blocks), 1, d + 1
    elif family == "generic":
        acc, fold, dot = d + 1, 1, d + 1
    else:
        raise KeyError(family)
    return acc + fold + dot, acc


def gamma(family, d, dtype, leg="energy"):
    u = UNIT_ROUNDOFF[dtype]
    k = gamma_units(family, d)[0 if leg == "energy" else 1]
    g = k * u / (1.0 - k * u)
    s = SPLIT_TERM if family == "bf16x3" else 0.0
    return s * (1.0 + g) + g


# ---------------------------------------------------------------------------------------------------- long-double reference
def _chunks(n, size=4096):
    return [(lo, min(n, lo + size)) for lo in range(0, n, size)]


def quadratic_form_ld(a, x):
    """x^T A x per chain in long double: a [D, D], x [n, D] -> [n]."""
    a, x = np.asarray(a, dtype=LD), np.asarray(x, dtype=LD)
    out = np.empty(x.shape[0], dtype=LD)
    for lo, hi in _chunks(x.shape[0]):
        out[lo:hi] = np.einsum("ni,ij,nj->n", x[lo:hi], a, x[lo:hi])
    return out


def abs_form(a, x):
    """sum_ij |x_i| |A_ij| |x_j| per chain in long double."""
    return quadratic_form_ld(np.abs(np.asarray(a, dtype=LD)), np.abs(np.asarray(x, dtype=LD)))


def matvec_ld(l, g):
    """L g per chain in long double: l [D, D], g [n, D] -> [n, D]."""
    return np.asarray(g, dtype=LD) @ np.asarray(l, dtype=LD).T


def abs_matvec(l, g):
    return matvec_ld(np.abs(np.asarray(l, dtype=LD)), np.abs(np.asarray(g, dtype=LD)))


def energy_ratio(e, a, x):
    """max over chains of |e - x^T A x| / abs_form, as a float (multiply by 1 / u for units of u)."""
    err = np.abs(np.asarray(e, dtype=LD) - quadratic_form_ld(a, x))
    return float(np.max(err / abs_form(a, x)))


def matvec_ratio(y, l, g):
    """max over chains and components of |y - L g| / (|L| |g|)."""
    err = np.abs(np.asarray(y, dtype=LD) - matvec_ld(l, g))
    return float(np.max(err / abs_matvec(l, g)))


# ---------------------------------------------------------------------------------------------------- plain chains
def fma_chain_energy(a, x, dtype):
    """x^T (A x) as the textbook loops in the working precision: y_i = fma chain over j ascending, E = fma chain over i
    ascending: the comparison model for the kernels that do not split."""
    t = NUMPY_DTYPE[dtype]
    a, x = np.asarray(a, dtype=t), np.asarray(x, dtype=t)
    n, d = x.shape
    y = np.zeros((n, d), dtype=t)
    for j in range(d):
        y = (y.astype(LD) + x[:, j:j + 1].astype(LD) * a[None, :, j].astype(LD)).astype(t)
    e = np.zeros(n, dtype=t)
    for i in range(d):
        e = (e.astype(LD) + x[:, i].astype(LD) * y[:, i].astype(LD)).astype(t)
    return e


def fma_chain_matvec(l, g, dtype):
    t = NUMPY_DTYPE[dtype]
    l, g = np.asarray(l, dtype=t), np.asarray(g, dtype=t)
    y = np.zeros(g.shape, dtype=t)
    for j in range(g.shape[1]):
        y = (y.astype(LD) + g[:, j:j + 1].astype(LD) * l[None, :, j].astype(LD)).astype(t)
    return y


# ---------------------------------------------------------------------------------------------------- the split-bf16 model
def bf16_pieces(v, count=3):
    """The truncation split of bf16_head (me_dense_bf16x3.h): ``count`` float32 pieces, each the top 16 bits of what the
    pieces before it left over (the subtraction is exact)."""
    rest = np.ascontiguousarray(v, dtype=np.float32)
    out = []
    for _ in range(count):
        head = (rest.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        rest = rest - head
        out.append(head)
    return out


# wave_matmul_64_bf16x3: within a k step, (piece of M, piece of X) in issue order -- qa = 2, 1, 0 and qx = 2 - qa .. 0
RETAINED_PRODUCTS = ((2, 0), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0))
# ... and the order in which the rows of the result reach the final dot: emit(32 mb + acc_row(r)), emit(... + 4)
EMIT_ORDER = tuple(32 * mb + (r & 3) + 8 * (r >> 2) + 4 * half for mb in range(2) for r in range(16) for half in range(2))


def split_bf16_product(m, x, drop=(), pieces=3, transpose=False, misplaced=None):
    """Y = M X as wave_matmul_64_bf16x3 forms it: m [64, 64], x [n, 64] float32 -> [n, 64] float32.
    One v_mfma_f32_32x32x16_bf16 = the exact sum of 16 exact products added to the float32 accumulator, rounded once
    (the block sum is formed in float64: exact while a block's terms span less than 33 binary orders, within 2^-53
    otherwise; the accumulator addition in long double before the rounding to float32).
    Planted defects: ``drop`` -- retained products left out; ``pieces=2`` -- a two-piece split (the four products of pieces 1 and 2: M1 X3 and M3 X1 are missing);
    ``transpose`` -- M's fragments built from M^T; ``misplaced=(qa, qx)`` -- that product reads X's fragment of the
    neighbouring k step."""
    m = np.asarray(m, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    assert m.shape == (64, 64) and x.shape[1] == 64
    if transpose:
        m = m.T
    mp = [p.astype(np.float64) for p in bf16_pieces(m, 3)]
    xp = [p.astype(np.float64) for p in bf16_pieces(x, 3)]
    acc = np.zeros((x.shape[0], 64), dtype=np.float32)
    for s in range(4):
        for qa, qx in RETAINED_PRODUCTS:
            if (qa, qx) in drop or (pieces == 2 and (qa == 2 or qx == 2)):
                continue
            sx = s ^ 1 if misplaced == (qa, qx) else s
            block = xp[qx][:, 16 * sx:16 * sx + 16] @ mp[qa][:, 16 * s:16 * s + 16].T
            acc = (acc.astype(LD) + block.astype(LD)).astype(np.float32)
    return acc


def split_bf16_energy(a, x, drop=(), **defect):
    """E = x^T (A x) as k_step_dense64_bf16x3 forms it: split_bf16_product, then e += x[row] * y[row] as one float32 fma
    per row in the kernel's row order."""
    x = np.asarray(x, dtype=np.float32)
    y = split_bf16_product(a, x, drop=drop, **defect)
    e = np.zeros(x.shape[0], dtype=np.float32)
    for row in EMIT_ORDER:
        e = (e.astype(LD) + x[:, row].astype(LD) * y[:, row].astype(LD)).astype(np.float32)
    return e


# planted defects of the model, name -> keyword arguments of split_bf16_product / split_bf16_energy
DEFECTS = {"drop_M%dX%d" % (qa + 1, qx + 1): dict(drop=((qa, qx),)) for qa, qx in RETAINED_PRODUCTS}
DEFECTS.update({
    "two_piece_split": dict(pieces=2),
    "neighbour_k_step_X1": dict(misplaced=(0, 0)),
})
# A misplaced fragment of the THIRD piece is milder than a dropped product on random data: the wrong fragment has the right
# magnitude, so its error has mean zero and averages out over the 64 terms (ones_mantissa: 20 u against 263 u for a dropped
# order-4 product), too close to honest code for a forward-error cap.  The exact two-hot case catches it bit for bit, and
# it is planted there only.
EXACT_DEFECTS = dict(DEFECTS, neighbour_k_step_X3=dict(misplaced=(0, 2)))
# x^T A x = x^T A^T x: a transposed operand is invisible to the energy (up to the order of rounding) and an O(1) error
# of L g, so it is planted on the factor leg only
FACTOR_DEFECTS = dict(DEFECTS, transposed_M=dict(transpose=True))


def calibrated_cap(a, x, model=split_bf16_energy, ratio=energy_ratio, defects=None):
    """(cap, r_ref, r_def, name of the mildest defect) on these inputs: cap = sqrt(r_ref r_def)."""
    r_ref = ratio(model(a, x), a, x)
    defects = DEFECTS if defects is None else defects
    names = list(defects)
    r = [ratio(model(a, x, **defects[name]), a, x) for name in names]
    k = int(np.argmin(r))
    return float(np.sqrt(r_ref * r[k])), r_ref, r[k], names[k]


# ---------------------------------------------------------------------------------------------------- input classes
CLASSES = ("spd", "asymmetric", "wide", "ones_mantissa")          # random classes: (A, X) = make_case(name, ...)
POW2_SHIFT = {"f32": 40, "f64": 300}


def _spd(d, rng):
    m = rng.standard_normal((d, d))
    return m @ m.T / d + np.identity(d)


def _all_ones(shape, rng, t):
    top = np.nextafter(t(2), t(0))                                  # 1.111...1: every mantissa bit set
    return (top * t(2.0) ** rng.integers(-2, 3, size=shape).astype(t)).astype(t)


def make_case(name, d, seed, dtype, n):
    """(A [d, d], X [n, d]) of class ``name`` as float64 arrays holding values of ``dtype`` exactly.  A depends on
    (name, d, seed, dtype) only: runs at different chain counts share the matrix."""
    t = NUMPY_DTYPE[dtype]
    rng, rng_x = np.random.default_rng([seed, d]), np.random.default_rng([seed, d, n])
    x = rng_x.standard_normal((n, d))
    if name in ("spd", "pow2_scaled"):
        a = _spd(d, rng)
    elif name == "asymmetric":
        a = _spd(d, rng) + 0.05 * np.triu(rng.standard_normal((d, d)), 1)
    elif name == "wide":                                             # entries over six decades, diagonally dominant
        a = _spd(d, rng) * np.exp(rng.uniform(-7.0, 7.0, size=(d, d)))
        a = 0.5 * (a + a.T) + 40.0 * np.diag(np.abs(a).sum(axis=1)) / d
    elif name == "ones_mantissa":
        a, x = _all_ones((d, d), rng, t), _all_ones((n, d), rng_x, t)
    else:
        raise KeyError(name)
    return np.asarray(a, dtype=t).astype(np.float64), np.asarray(x, dtype=t).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- exact two-hot
SPLIT_UNIT = 2 ** 16 + 2 ** 8 + 1              # pieces 2^16, 2^8, 1: all three non-zero in both operands
SPLIT_RETAINED = SPLIT_UNIT ** 2 - 513         # the six retained piece products of SPLIT_UNIT^2 (neglected: 2^8 + 2^8 + 1)


def two_hot_pairs(d):
    """Chain (i, j), i <= j: one per diagonal entry and one per pair -- d (d + 1) / 2 chains."""
    i, j = np.triu_indices(d)
    return i, j


def two_hot_case(d, seed, split):
    """(A, X, c): A asymmetric with a (sign, 2^e) code per position -- off the diagonal sign +-1 and e in 0..3 drawn per
    position, on the diagonal +2^4, so that x^T A x = c^2 (A_ii + A_jj + A_ij + A_ji) > 0 for every chain -- times the
    magnitude c; chain (i, j) has x_i = x_j = c and zeros elsewhere.  c = SPLIT_UNIT for the split kernel, 3 otherwise."""
    rng = np.random.default_rng([seed, d, 2])
    code = rng.choice([-1.0, 1.0], size=(d, d)) * 2.0 ** rng.integers(0, 4, size=(d, d))
    code[np.diag_indices(d)] = 16.0
    c = float(SPLIT_UNIT) if split else 3.0
    i, j = two_hot_pairs(d)
    x = np.zeros((i.size, d))
    x[np.arange(i.size), i] = c
    x[np.arange(i.size), j] = c
    return code * (c if split else 5.0), x, code


def _round_to_bits(v, bits):
    """Round int64 values to ``bits`` significant bits, to nearest even; also returns where the rounding was a tie."""
    v = np.asarray(v, dtype=np.int64)
    mag = np.abs(v)
    length = np.zeros(v.shape, dtype=np.int64)
    nz = mag > 0
    length[nz] = np.floor(np.log2(mag[nz].astype(LD))).astype(np.int64) + 1
    sh = np.maximum(length - bits, 0)
    q, rem = mag >> sh, mag & ((np.int64(1) << sh) - 1)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), np.int64(-1))
    tie = rem == half
    up = (rem > half) & (sh > 0) | tie & ((q & 1) == 1)
    return np.sign(v) * ((q + up) << sh), tie


def two_hot_expected(d, code, split):
    """What integer arithmetic gives for every two-hot chain: (fused, unfused, tie), float64 arrays that hold the values
    exactly and whether the first rounding was a tie for some chain (the CPU test asserts that it is not, so that nothing
    of size 1e-30 can decide it).
    Not split: every product and sum is a small integer, E = 9 * 5 * (code_ii + code_jj + code_ij + code_ji), and the two
    arrays are the same.
    Split: a term A_rk x_k contributes code_rk * SPLIT_RETAINED -- its six retained piece products, each a multiple of 2^16
    below 2^40, as is every partial sum of a row (|code_ri + code_rj| <= 24) -- so y_r is exact in any order.  The final
    dot multiplies by x_r = SPLIT_UNIT: 17 x 22 bits do not fit 24 (no choice of three non-zero pieces does), so E takes
    two float32 roundings, evaluated here on integers: fl(fl(x_a y_a) + x_b y_b) where the second row's multiply-add is
    fused, fl(fl(x_a y_a) + fl(x_b y_b)) where it is not -- the compiler's choice per row, see (3) above; a before b in the
    kernel's row order.  The two differ by an ulp of E at most, 2^-8 of the smallest retained product."""
    i, j = two_hot_pairs(d)
    code = code.astype(np.int64)
    diag = i == j
    if not split:
        e = (45 * np.where(diag, code[i, i], code[i, i] + code[j, j] + code[i, j] + code[j, i])).astype(np.float64)
        return e, e, False
    assert d == 64
    pos = np.argsort(np.asarray(EMIT_ORDER))          # pos[row] = when the row reaches the dot
    first = np.where(pos[i] <= pos[j], i, j)
    second = np.where(pos[i] <= pos[j], j, i)

    def y(r):                                          # row r of A x for chain (i, j), an integer
        return SPLIT_RETAINED * np.where(diag, code[r, i], code[r, i] + code[r, j])

    assert np.all(np.abs(y(first)) < 2 ** 40) and np.all(y(first) % 2 ** 16 == 0)
    e1, tie1 = _round_to_bits(SPLIT_UNIT * y(first), 24)
    p2 = np.where(diag, 0, SPLIT_UNIT * y(second))
    fused = _round_to_bits(e1 + p2, 24)[0]
    unfused = _round_to_bits(e1 + _round_to_bits(p2, 24)[0], 24)[0]
    # only the first rounding can have something tiny beside it (the sum so far, when that multiply-add is fused): float32
    # values absorb it, the later roundings are of exact integers
    return fused.astype(np.float64), unfused.astype(np.float64), bool(np.any(tie1))
