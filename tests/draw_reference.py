"""Per-value references for the draw and accept arithmetic of the step kernels, in plain numpy and ``np.longdouble``
(x87 extended precision, 64-bit significand): what ONE Box-Muller normal, ONE magnitude-phase angle and ONE accept
decision must be, given the Philox words of ``oracle.philox``.

    words            oracle.philox.step_words(seed, chain ids, step, n)         (the stream is the oracle's)
    units            float64: (w + 0.5) 2^-32, exact.  float32: Num<float>::unit restated -- w rounded to float32, then
                     w32 2^-32 + 2^-33 (exact in float64) rounded to float32 -- so that a float32 reference judges the
                     hardware transcendentals on the inputs they really get, not the input rounding
    normals          r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2); for float64 words the nearest quarter revolution
                     is removed in integer arithmetic first (test_math64_cpu._reference_cos_sin), so the reference has
                     no reduction error beside the zeros of cos / sin
    layout           normal i belongs to coordinate i of [real | Re z | Im z]; complex coordinates carry 1/sqrt 2
    accept rule      u <= exp(-d/T) with the kernels' own argument: x = fl(-d fl(1/T)) in float64 (one multiply),
                     fl32(-d32 fl32(log2 e / T)) and 2^x in float32
"""
import numpy as np

from oracle import philox
from test_math64_cpu import _reference_cos_sin, _ulp_err

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
SQRT_HALF = LD("0.70710678118654752440084436210484903")
LN2 = LD("0.69314718055994530941723212145817657")
EPS32 = 2.0 ** -24           # unit roundoff of float32
EPS64 = 2.0 ** -53           # unit roundoff of float64

__all__ = ["LD", "EPS32", "EPS64", "words", "units", "unit_f32", "normal_pairs", "coordinate_normals", "scale_complex",
           "phases", "magphase_words", "accept_reference", "fit_float32_bound", "float32_bound", "ulp_err", "chain_ids"]

ulp_err = _ulp_err


def chain_ids(n_chains, chain_offset=0):
    return np.arange(n_chains, dtype=np.uint64) + np.uint64(chain_offset)


def words(seed, ids, step, n_words):
    """Words 0 .. n_words-1 of one step: [n_chains, n_words], uint64 holding 32-bit values."""
    return philox.step_words(seed, ids, step, n_words)


def unit_f32(w):
    """Num<float>::unit: fmaf((float)w, 2^-32, 2^-33), as a float32 array."""
    w32 = np.asarray(w, dtype=np.uint64).astype(np.float32)                 # v_cvt_f32_u32: round to nearest even
    exact = w32.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33               # <= 34 significant bits: exact
    return exact.astype(np.float32)


def units(w, dtype):
    """The unit-interval values the kernels of ``dtype`` make of the words, as long double (exactly those values)."""
    if dtype == "f32":
        return unit_f32(w).astype(LD)
    return (np.asarray(w, dtype=np.uint64).astype(LD) + LD(0.5)) / LD(2 ** 32)


def normal_pairs(wa, wb, dtype):
    """Box-Muller on word pairs: (g0, g1, r) in long double, r the radius of the pair."""
    r = np.sqrt(LD(-2) * np.log(units(wa, dtype)))
    if dtype == "f32":
        t = (LD(2) * PI) * units(wb, dtype)
        cs, sn = np.cos(t), np.sin(t)
    else:
        cs, sn = _reference_cos_sin(np.asarray(wb, dtype=np.uint64))
    return r * cs, r * sn, r


def coordinate_normals(w, n_normals, dtype):
    """Normals 0 .. n_normals-1 of words ``w[:, :2 ceil(n/2)]`` (normal 2q from words 2q, 2q+1 as r cos, normal 2q+1 as
    r sin) and the radius behind each: two [n_chains, n_normals] long-double arrays."""
    nw = philox.n_normal_words(n_normals)
    g0, g1, r = normal_pairs(w[:, 0:nw:2], w[:, 1:nw:2], dtype)
    g = np.empty((w.shape[0], nw), dtype=LD)
    rad = np.empty((w.shape[0], nw), dtype=LD)
    g[:, 0::2], g[:, 1::2] = g0, g1
    rad[:, 0::2] = rad[:, 1::2] = r
    return g[:, :n_normals], rad[:, :n_normals]


def scale_complex(g, rad, nr):
    """What one accepted identity-shape step from x = 0 with width 1 leaves in the state: g for the real coordinates,
    g / sqrt 2 for the Re and Im parts of the complex ones (the radius is scaled alike)."""
    g, rad = g.copy(), rad.copy()
    g[:, nr:] *= SQRT_HALF
    rad[:, nr:] *= SQRT_HALF
    return g, rad


def magphase_words(nc):
    """Word positions of one magnitude-phase step (me_magphase.h): (W1, accept word of the magnitude stage, first phase
    word, accept word of the phase stage, words in all)."""
    w1 = philox.n_normal_words(nc)
    return w1, w1, w1 + 1, w1 + nc + 1, w1 + nc + 2


def phases(w, dtype):
    """The redrawn phases -pi + 2 pi u of the magnitude-phase sampler, long double, in [-pi, pi]."""
    return -PI + (LD(2) * PI) * units(w, dtype)


def accept_reference(d, u, temp, dtype, band):
    """The accept decision of an UPHILL move of size ``d`` (> 0; d <= 0 accepts) against the uniform ``u`` at temperature
    ``temp`` (scalars or arrays), and a tie flag: |u - p| <= band (an array or scalar the caller derives).

    float64: x = fl(-d64 fl(1/T)), p = e^x.  float32: x = fl32(-d32 fl32(log2 e / T)), p = 2^x.  p in long double.
    Returns (accept, tie, p)."""
    temp = np.asarray(temp, dtype=np.float64)
    d = np.asarray(d)
    if dtype == "f32":
        c = (1.4426950408889634 / temp).astype(np.float32)
        x = (-(d.astype(np.float32)) * c).astype(np.float32)        # float32 * float32 in numpy: one rounding
        p = np.exp(x.astype(LD) * LN2)
    else:
        x = -(d.astype(np.float64)) * (1.0 / temp)
        p = np.exp(x.astype(LD))
    u = np.asarray(u).astype(LD)
    accept = (d <= 0) | (u <= p)
    tie = (d > 0) & (np.abs(u - p) <= band)
    return accept, tie, p


# ---------------------------------------------------------------------------------------------- float32 error model
def fit_float32_bound(got, ref, rad):
    """The smallest (A, B) of the float32 model |g - g_ref| <= A eps32 |g_ref| + B eps32 r_ref that this routine's fixed
    recipe gives for the measured normals ``got``: with e = |g - g_ref| / (eps32 r) and t = |g_ref| / r (|cos| or |sin|),

        B = max e over the samples with t <= 0.1      (beside a zero of cos / sin only the absolute part can pay)
        A = max (e - B) / t over the rest, at least 0  (what the relative part has to add)

    so that A t + B >= e on every sample.  Pairs with r_ref = 0 (u1 = 1) must give g = 0 exactly and are left out."""
    got, ref, rad = (np.asarray(v).astype(LD).ravel() for v in (got, ref, rad))
    live = rad > 0
    assert np.all(got[~live] == 0)
    got, ref, rad = got[live], ref[live], rad[live]
    e = np.abs(got - ref) / (LD(EPS32) * rad)
    t = np.abs(ref) / rad
    small = t <= LD(0.1)
    b = float(e[small].max()) if small.any() else 0.0
    a = float(np.maximum((e[~small] - LD(b)) / t[~small], 0).max()) if (~small).any() else 0.0
    return a, b


# The committed constants: TWICE the worst values tools/measure_draw_conformance.py saw on an MI355X (the hardware is
# deterministic per input, the margin covers the words not drawn); DESIGN.md, "Draw conformance", has the measurements.
FLOAT32_A = 10.93            # measured 5.4617 over 2^22 word pairs (seeds 7001, 7002)
FLOAT32_B = 1.35             # measured 0.6743
FLOAT32_PHASE_REV = 6.83e-8  # float32 magnitude-phase angle, revolutions: measured 3.413e-8 (3 x 2^19 phases)
FLOAT64_PHASE_RAD = 8.97e-16 # float64 magnitude-phase angle, radians: measured 4.484e-16


def float32_bound(ref, rad, a, b):
    """A eps32 |g_ref| + B eps32 r_ref (long double)."""
    return LD(a * EPS32) * np.abs(ref) + LD(b * EPS32) * rad


# ------------------------------------------------------------------------------ the accept rule on the engine's own draws
# What tests/test_gpu_draw_conformance.py runs and tests/test_draw_reference_cpu.py checks the caps of, from the reference
# alone: DiagQuadratic from x0 = 0 with width 1, one step, 2^16 chains.
ACCEPT_SEED = 4242
ACCEPT_CHAINS = 1 << 16
ACCEPT_OFFSET = (1 << 33) + 17
ACCEPT_SHAPES = {(4, 0): ((1.0, 2.0, 0.5, 1.5), ()), (2, 1): ((1.0, 2.0), (1.5,))}
ACCEPT_LADDER = (1.0, 1.001, 1.002, 1.003)
ACCEPT_TEMPS = (0.3, 1.0, 30.0, ACCEPT_LADDER, 1e-3)         # 1e-3: the large dE/T case, nothing may be accepted
ACCEPT_TIE_CAP = {"f32": 1e-3, "f64": 0.0}                   # largest share of chains the tie band may flag
FLOAT64_NORMAL_ULPS = 4.0                                    # me_math64.h: normals <= 4 ulp ...
FLOAT64_COMPLEX_ULPS = 4.5                                   # ... and half an ulp for the 1/sqrt 2 scaling


def chain_temps(temp, n_chains):
    """Per-chain temperatures: a scalar, or a ladder whose rung k owns the k-th run of n_chains / K chains."""
    if np.ndim(temp) == 0:
        return np.full(n_chains, float(temp))
    return np.repeat(np.asarray(temp, dtype=np.float64), n_chains // len(temp))


def accept_case_reference(nr, nc, temp, dtype, f32_ab=None, n_chains=ACCEPT_CHAINS, seed=ACCEPT_SEED, step=0):
    """One step of the accept cases above from the reference alone: the long-double proposal g [n, D] (what an accepted
    chain's state must be), the decision, the tie flags and p.

    The tie band is the first-order image of the normal bounds in p (eps = unit roundoff of the dtype, D = nr + 2 nc,
    d = sum w_i g_i^2, c = 1/T, or log2 e / T in float32, x = -d c, p = e^x or 2^x):
      * the normals: |dg_i| <= k_i 2 eps |g_i| with k = 4 / 4.5 ulp in float64; A eps |g_i| + B eps r_i in float32, so
        |dd| <= sum w_i 2 |g_i| |dg_i|;
      * the energy: D terms of two roundings each (w x, then a fused multiply-add) summed in two interleaved chains, all
        terms >= 0, and the difference to the ledger's exact 0: at most (D + 4) eps d; float32 rounds the reference's d
        once more (eps d);
      * the argument: one multiply, eps |x|, on top of c |dd|;
      * the exponential: exp_nonpos is within 1.5 ulp = 3 eps p (me_math64.h); v_exp_f32 within 1 ulp = 2 eps p (the
        instruction's documented accuracy), and results below the normal range may be flushed: 2^-126 absolute; float64
        subnormal results are within two subnormal steps (tests/test_math64_cpu.py).
    band = p (L (c |dd| + eps |x|) + E eps) + floor, with |dd| the sum of the first two items, L = 1 and E = 3 (float64)
    or L = ln 2 and E = 2 (float32).  ``f32_ab``: the (A, B) of the float32 normal bound."""
    weights_r, weights_c = ACCEPT_SHAPES[(nr, nc)]
    d_ = nr + 2 * nc
    w = words(seed, chain_ids(n_chains, ACCEPT_OFFSET), step, philox.n_normal_words(d_) + 1)
    g, rad = coordinate_normals(w, d_, dtype)
    g, rad = scale_complex(g, rad, nr)
    wd = np.concatenate((weights_r, weights_c, weights_c)).astype(LD)
    d = (wd * g * g).sum(axis=1)
    u = units(w[:, philox.n_normal_words(d_)], dtype)
    temps = chain_temps(temp, n_chains)
    if dtype == "f32":
        a, b = f32_ab
        eps, c = LD(EPS32), (1.4426950408889634 / temps).astype(np.float32).astype(LD)
        dg = float32_bound(g, rad, a, b)
        spread, e_exp, floor, extra = LN2, 2, LD(2.0 ** -126), 1
    else:
        eps, c = LD(EPS64), (1.0 / temps).astype(LD)
        k = np.where(np.arange(d_) < nr, FLOAT64_NORMAL_ULPS, FLOAT64_COMPLEX_ULPS).astype(LD)
        dg = k * 2 * eps * np.abs(g)
        spread, e_exp, floor, extra = LD(1), 3, LD(1e-323), 0
    dd = (wd * 2 * np.abs(g) * dg).sum(axis=1) + (d_ + 4 + extra) * eps * d
    accept, _, p = accept_reference(d, u, temps, dtype, 0)
    band = p * (spread * (c * dd + eps * c * d) + e_exp * eps) + floor
    accept, tie, p = accept_reference(d, u, temps, dtype, band)
    return g, accept, tie, p
