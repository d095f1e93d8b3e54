"""Every step kernel's random draws and accept test, value by value, against tests/draw_reference.py (long double).

The draws are observable bit for bit through the public API: a fresh engine at x0 = 0 with sampling_width = 1 and an energy
that accepts everything leaves x = g after one step (fl(g fl(1/sqrt 2)) in the complex coordinates) -- the identity-shape
update is x + w g, and a per-chain factor that is the identity adds exact zeros.  So every coordinate of every chain is
compared with the reference normal of exactly the word pair the layout assigns to it: 2^16 chains whose global ids start at
2^33 + 17, at step 0 and at step 2^32 + 5 (the high step word of the Philox counter).

Bounds
  float64 normals   4 ulp of the reference (me_math64.h's claim; tests/test_math64_cpu.py holds the host build to it with an
                    emulated v_rsq_f64), 4.5 ulp in the complex coordinates (one more rounding, the 1/sqrt 2).  Worst seen on
                    the device (2^23 normals of two other seeds): 3.63 ulp real, 3.81 ulp complex.
  float32 normals   |g - g_ref| <= A eps32 |g_ref| + B eps32 r_ref against the reference ON THE FLOAT32-ROUNDED UNITS, with
                    eps32 = 2^-24, r_ref the radius of the pair; A + 1 in the complex coordinates.  Measured on an MI355X
                    (tools/measure_draw_conformance.py; 2^22 word pairs of two seeds this file does not use; B = worst
                    error / (eps32 r) where |g_ref| <= 0.1 r, A = worst (error / (eps32 r) - B) / (|g_ref| / r) elsewhere):
                    worst observed A = 5.4617, B = 0.6743; committed draw_reference.FLOAT32_A = 10.93, FLOAT32_B = 1.35,
                    twice that.  (The worst normal, 4.54 eps32 r, sits at u1 = 0.8625, |cos| = 0.9989: it is the radius,
                    i.e. v_log_f32 about 3 ulp off where log2 u1 is near -0.2.  For u1 > 1 - 2^-12 the radius, seen as
                    hypot(g0, g1), is within 3.18 eps32 relative: no loss of relative accuracy beside the zero of the log.)
  phases            the magnitude-phase sampler's angle atan2(Im, Re) against -pi + 2 pi u: float32 in revolutions, float64
                    in radians, measured the same way (3 x 2^19 phases): worst observed 3.413e-8 revolutions / 4.484e-16
                    rad; committed draw_reference.FLOAT32_PHASE_REV = 6.83e-8, FLOAT64_PHASE_RAD = 8.97e-16, twice that.
  layout            no coordinate may pass as the coordinate two places on (the neighbouring word pair's).

The accept rule
  float64, adversarial (step_injected): d = g^2 exact (g has 20 significant bits), u = nextafter^k(fl(p_ref)): accepted for
                    k <= -2, rejected for k >= 2 (exp_nonpos within 1.5 ulp + half an ulp for rounding p_ref).
  both dtypes, on the engine's own draws: the decision ("x changed") equals the reference's on every chain outside the tie band
                    that draw_reference.accept_case_reference derives from the bounds above (its docstring has the
                    derivation); at most 1e-3 of the chains tie in float32, none in float64 (tests/test_draw_reference_cpu.py
                    confirms both from the reference alone, for these very seeds).
"""
import functools

import numpy as np
import pytest

import draw_reference as dr
import metropolisengine_amd as me
from metropolisengine_amd import _capi

pytestmark = pytest.mark.gpu
LD = dr.LD
SEED = 20261020
N = 1 << 16
OFFSET = (1 << 33) + 17
STEPS = (0, (1 << 32) + 5)
MAX_NORMALS = 140
PHASE_WIDTH = 0.25          # magnitude-phase: |z| = 1 + w^2 g stays positive (|g| < 6.7), and w^2 = 1/16 scales exactly


@functools.lru_cache(maxsize=2)
def stream_reference(step, dtype, seed=SEED, n=N):
    """Words and the first MAX_NORMALS reference normals (with their radii) of every chain at one step: computed once and
    shared -- a chain's words do not depend on the parameter space."""
    w = dr.words(seed, dr.chain_ids(n, OFFSET), step, MAX_NORMALS + 4)
    g, rad = dr.coordinate_normals(w, MAX_NORMALS, dtype)
    for a in (w, g, rad):
        a.setflags(write=False)
    return w, g, rad


def set_step(eng, step):
    eng._check(eng._lib.me_set_counters(eng._handle, step, eng._counters()[1]))


def fresh_engine(energy, nr, nc, dtype, step, seed=SEED, n=N, width=1.0, z0=0j, **kw):
    eng = me.MetropolisEngine(energy, None, [0.0] * nr if nr else None, [z0] * nc if nc else None, sampling_width=width,
                              n_chains=n, seed=seed, dtype=dtype, chain_offset=OFFSET, **kw)
    set_step(eng, step)
    return eng


def within_bound(x, g, rad, nr, dtype):
    """[n, D] bool: the state x is the reference normal g within the bound of its dtype."""
    if dtype == "f64":
        k = np.where(np.arange(g.shape[1]) < nr, dr.FLOAT64_NORMAL_ULPS, dr.FLOAT64_COMPLEX_ULPS)
        return dr.ulp_err(x, g) <= k
    a = np.where(np.arange(g.shape[1]) < nr, dr.FLOAT32_A, dr.FLOAT32_A + 1.0).astype(LD)
    return np.abs(x.astype(LD) - g) <= LD(dr.EPS32) * (a * np.abs(g) + LD(dr.FLOAT32_B) * rad)


def check_normals(x, nr, nc, dtype, step, seed=SEED):
    d = nr + 2 * nc
    _, g, rad = stream_reference(step, dtype, seed, x.shape[0])
    g, rad = dr.scale_complex(g[:, :d], rad[:, :d], nr)
    ok = within_bound(x, g, rad, nr, dtype)
    assert ok.all(), "coordinates %s of %d chains miss their reference normal" % (np.flatnonzero(~ok.all(axis=0))[:8], int((~ok.all(axis=1)).sum()))
    # sharp: the neighbouring pair's normal (two coordinates on, same scaling) must NOT pass
    for j in range(d - 2):
        if (j < nr) == (j + 2 < nr):
            wrong = within_bound(x[:, j:j + 1], g[:, j + 2:j + 3], rad[:, j + 2:j + 3], nr if j < nr else 0, dtype)
            assert wrong.mean() < 1e-3, j


def one_accepted_step(kind, nr, nc, dtype, step):
    """The state after one step in which every proposal is accepted, through the kernel that ``kind`` selects."""
    if kind == "identity":
        eng = fresh_engine(me.IsoQuadratic(0.0), nr, nc, dtype, step, temp=1.0, cov_mode="fixed")
    elif kind == "per_chain":
        # the constructor's identity covariances leave every chain's factor the identity; writing one chain's row of the
        # factor field switches the engine to its per-chain kernels (register-resident, streamed, or the runtime-dimension
        # form).  Chain 0 gets L_00 = 2: its x_0 must then be 2 g_0 exactly, so the kernel did read the field.
        eng = fresh_engine(me.DiagQuadratic([0.0] * nr, [0.0] * nc), nr, nc, dtype, step, temp=1.0,
                           covariance_matrix_real=np.identity(nr) if nr else None,
                           covariance_matrix_complex=np.identity(nc) if nc else None)
        assert eng.cov_mode == "reference"
        row = np.zeros((1, nr * (nr + 1) // 2 + nc * nc))
        row[0, [i * (i + 1) // 2 + i for i in range(nr)]] = 1.0
        row[0, [nr * (nr + 1) // 2 + j * j + 2 * j for j in range(nc)]] = 1.0
        row[0, 0] = 2.0
        eng._set(_capi.FIELD_FACTOR, row)
    else:
        assert kind == "dense64" and (nr, nc) == (64, 0)
        eng = fresh_engine(me.DenseQuadratic(np.identity(64)), nr, nc, dtype, step, temp=1e30, cov_mode="fixed")
    eng.step_all(1)
    x = eng._get(_capi.FIELD_PARAMS)
    assert eng.accept_stats() == (x.shape[0], x.shape[0])
    eng.sync()                                  # raises if a status bit is set
    if kind == "per_chain":
        x[0, 0] *= 0.5
    return x


# the smallest shapes that reach each site where Philox words are unpacked into normals
NORMAL_CASES = [
    ("identity", 16, 0, ("f32", "f64")),      # draw_step, k_step
    ("identity", 3, 0, ("f32", "f64")),       # odd D: the accept word is in the second Philox block
    ("identity", 2, 1, ("f32", "f64")),       # the 1/sqrt 2 path
    ("identity", 0, 3, ("f32", "f64")),
    ("per_chain", 4, 4, ("f32", "f64")),      # register-resident per-chain factor
    ("per_chain", 16, 0, ("f64",)),           # 136 entries > kStreamF64Entries: the streamed-factor body of k_step (float64)
    ("per_chain", 24, 0, ("f32",)),           # 300 entries > 160: the streamed-factor body in float32
    ("identity", 130, 0, ("f32", "f64")),     # k_step_runtime
    ("identity", 101, 0, ("f32", "f64")),     # ... odd D
    ("per_chain", 140, 0, ("f32", "f64")),    # k_step_runtime_lds<CK_PER_CHAIN>: the smallest runtime-dimension per-chain shape
    ("dense64", 64, 0, ("f32", "f64")),       # me_dense_f64.h; split-bf16 (me_dense_bf16x3.h on me_dense64.h) in float32
]
NORMAL_PARAMS = [pytest.param(kind, nr, nc, dtype, step, id="%s-%d-%d-%s-step%d" % (kind, nr, nc, dtype, i))
                 for dtype in ("f32", "f64") for i, step in enumerate(STEPS)
                 for kind, nr, nc, dtypes in NORMAL_CASES if dtype in dtypes]


@pytest.mark.parametrize("kind,nr,nc,dtype,step", NORMAL_PARAMS)
def test_every_normal_is_its_word_pairs_reference_normal(kind, nr, nc, dtype, step):
    x = one_accepted_step(kind, nr, nc, dtype, step)
    check_normals(x, nr, nc, dtype, step)


def phase_errors(z, theta_ref):
    """angle(z) - theta_ref in long double, wrapped to (-pi, pi]: the angle of z e^{-i theta_ref}."""
    re, im = z.real.astype(LD), z.imag.astype(LD)
    c, s = np.cos(theta_ref), np.sin(theta_ref)
    return np.arctan2(im * c - re * s, re * c + im * s)


def one_magphase_step(nr, nc, dtype, step, seed=SEED, n=N):
    eng = fresh_engine(me.IsoQuadratic(0.0), nr, nc, dtype, step, seed=seed, n=n, width=PHASE_WIDTH, z0=1.0 + 0j, temp=1.0,
                       complex_sample_method="magnitude-phase")
    eng.step_complex_group()
    x = eng._get(_capi.FIELD_PARAMS)
    assert eng.accept_stats() == (2 * n, 2 * n)             # two decisions per step
    eng.sync()
    return x


@pytest.mark.parametrize("nr,nc,dtype,step", [pytest.param(nr, nc, dtype, step, id="%d-%d-%s-step%d" % (nr, nc, dtype, i))
                                              for dtype in ("f32", "f64") for i, step in enumerate(STEPS)
                                              for nr, nc in ((0, 3), (2, 2))])
def test_magnitude_phase_words(nr, nc, dtype, step):
    """k_step_magphase: pairs 0 .. W1-1 are the magnitude normals (|z| = 1 + w^2 g, w^2 = 1/16), words W1+1 .. W1+nc the
    phases -pi + 2 pi u.  (The accept words W1 and W1+nc+1 decide nothing here; test_magnitude_phase_accept_words has them.)
    Magnitude tolerance: the normal's own bound / 16, plus the roundings of 1 + g/16, of |z| cos, |z| sin and of the
    hypot taken here, <= 6 eps |z| with |z| < 1.5.  Angle bound: measured, see the module docstring."""
    x = one_magphase_step(nr, nc, dtype, step)
    assert not x[:, :nr].any()                              # the real parameters rest
    z = x[:, nr:nr + nc] + 1j * x[:, nr + nc:]
    w, g, rad = stream_reference(step, dtype, SEED, N)
    w1, _, first_phase, _, _ = dr.magphase_words(nc)
    eps = LD(dr.EPS32 if dtype == "f32" else dr.EPS64)
    if dtype == "f32":
        g_tol = dr.float32_bound(g[:, :nc], rad[:, :nc], dr.FLOAT32_A, dr.FLOAT32_B)
    else:
        g_tol = LD(dr.FLOAT64_NORMAL_ULPS) * 2 * eps * np.abs(g[:, :nc])
    mag = np.hypot(z.real.astype(LD), z.imag.astype(LD))
    assert np.all(np.abs(mag - (1 + g[:, :nc] / 16)) <= g_tol / 16 + 9 * eps)
    theta = dr.phases(w[:, first_phase:first_phase + nc], dtype)
    err = np.abs(phase_errors(z, theta))
    bound = LD(dr.FLOAT32_PHASE_REV) * 2 * dr.PI if dtype == "f32" else LD(dr.FLOAT64_PHASE_RAD)
    assert np.all(err <= bound), float(err.max())
    # sharp: the neighbouring word's phase does not pass
    for j in range(nc):
        other = dr.phases(w[:, first_phase + j + 1], dtype)
        assert (np.abs(phase_errors(z[:, j], other)) <= bound).mean() < 1e-3


# ------------------------------------------------------------------------------------------------------ the accept rule
KS = (-64, -8, -2, 2, 8, 64)
SPECIAL_RATIOS = (0.5 * np.log(2.0), np.log(2.0), 708.4, 745.0, 746.0, 1000.0)


def round_to_bits(v, bits):
    m, e = np.frexp(v)
    return np.ldexp(np.round(np.ldexp(m, bits)), e - bits)


def step_ulps(v, k):
    """nextafter^k(v) for float64 arrays v >= 0 (k < 0: towards 0, never below it)."""
    out = v.copy()
    for _ in range(abs(k)):
        out = np.nextafter(out, np.inf if k > 0 else 0.0)
    return out


def adversarial_draws(temps, lo, hi, uphill_of=lambda g: g * g, g_of=np.sqrt):
    """Per chain (its temperature in ``temps``): an injected normal g of 20 significant bits whose uphill move d is exact,
    an injected uniform u = nextafter^k(fl(p_ref)), and the decision that u must get.  d/T runs log-spaced from lo to hi plus
    the special ratios (to the 2^-20 that g's rounding allows); every ratio meets every k, shuffled over the chains so
    that every rung of a ladder sees the whole range."""
    n = temps.size
    m = n // len(KS)
    ratios = np.concatenate((np.geomspace(lo, hi, m - len(SPECIAL_RATIOS)), SPECIAL_RATIOS))
    combos = np.random.default_rng(5).permutation(m * len(KS))
    combos = np.concatenate((combos, combos[:n - combos.size]))
    ratio, k = ratios[combos // len(KS)], np.asarray(KS)[combos % len(KS)]
    g = round_to_bits(g_of(ratio * temps), 20)
    d = uphill_of(g)
    assert np.array_equal(d.astype(LD), uphill_of(g.astype(LD))) and np.all(d > 0)       # d is exact in float64
    _, _, p = dr.accept_reference(d, 0.0, temps, "f64", 0)
    p64 = p.astype(np.float64)
    u = np.empty(n)
    for kk in KS:
        sel = k == kk
        u[sel] = step_ulps(p64[sel], kk)
    under = p64 == 0.0                                   # p_ref underflows: every u > 0 must be rejected
    u[under] = step_ulps(p64[under], 1) * np.abs(k[under])
    expect = (k < 0) & ~under
    assert expect.sum() > n // 3 and under.sum() >= len(KS) and np.all(u[under] > 0)
    return g, u, expect


LADDER = (1.0, 1.001, 1.002, 1.003)


@pytest.mark.parametrize("temp", [0.1, 1.0, 3e4, LADDER], ids=["T0.1", "T1", "T3e4", "ladder"])
def test_float64_accept_threshold_to_two_ulp(temp):
    """One real parameter, IsoQuadratic(1), x0 = 0, width 1, 4096 chains, one injected launch: d = g^2 exactly, and the
    uniform sits k float64 steps from the rounded long-double exp(fl(-d fl(1/T))).  |k| >= 2 must decide as the reference."""
    n = 4096
    kw = dict(temperatures=list(temp)) if np.ndim(temp) else dict(temp=temp)
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0], None, sampling_width=1.0, n_chains=n, seed=1, dtype="f64",
                              cov_mode="fixed", **kw)
    temps = dr.chain_temps(temp, n)
    if np.ndim(temp):
        assert np.array_equal(eng.chain_temperatures(), temps)
    g, u, expect = adversarial_draws(temps, 1e-17, 700.0)
    eng.step_injected(g[None, :, None], u[None, :])
    x = eng._get(_capi.FIELD_PARAMS)[:, 0]
    accepted = x != 0
    assert np.array_equal(accepted, expect), "%d decisions differ" % int((accepted != expect).sum())
    assert np.array_equal(x[accepted], g[accepted])
    assert eng.accept_stats() == (int(expect.sum()), n)
    eng.sync()


def test_magnitude_phase_accept_words():
    """The injected magnitude-phase kind: its uniforms are [u_mag, phases 1 .. nc, u_phase], the accept draws at positions 0
    and nc + 1.  One complex parameter at z = 1, width 1, K = 1, IsoQuadratic(1):

    magnitude stage  |z| -> m = 1 + g with 20 significant bits, d = m^2 - 1 exact, u_mag at the threshold as in
                     test_float64_accept_threshold_to_two_ulp (d/T from 1e-5: 1 + g has to stay representable);
                     the phase stage then proposes the phase 0 it already has (u = 0.5: theta = fma(2 pi, 0.5, -pi) = 0, d = 0) and
                     accepts, so |z| tells the magnitude decision -- whatever sits at position nc + 1 (here: 2, which
                     would reject any uphill move).
    phase stage      on a mixed (2, 2) engine with E = x^T diag(1, 1, 1, 1, 3, 3) x, Im twice as steep as Re: g = 0 keeps
                     |z| = 1, the phases move z from 1 to e^{i theta}, d = 2 (sin^2 theta_1 + sin^2 theta_2) to a few
                     ulp, and u_phase = p_ref (1 -+ 1e-9) must accept / reject while position 0 holds the uniform that
                     would decide the other way (0 accepts everything, 2 rejects every uphill move)."""
    n = 4096
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, None, [1.0 + 0j], sampling_width=1.0, n_chains=n, seed=1, dtype="f64",
                              temp=1.0, complex_sample_method="magnitude-phase")
    g1, u, expect = adversarial_draws(np.ones(n), 1e-5, 700.0, uphill_of=lambda m: m * m - 1, g_of=lambda d: np.sqrt(1 + d))
    uniforms = np.stack((u, np.full(n, 0.5), np.full(n, 2.0)), axis=1)
    eng.step_injected((g1 - 1.0)[None, :, None], uniforms[None], kind=_capi.STEP_COMPLEX_MAGNITUDE_PHASE)
    x = eng._get(_capi.FIELD_PARAMS)
    assert np.array_equal(x[:, 0], np.where(expect, g1, 1.0)) and not x[:, 1].any()
    assert eng.accept_stats() == (int(expect.sum()) + n, 2 * n)

    eng = me.MetropolisEngine(me.DenseQuadratic(np.diag([1.0, 1.0, 1.0, 1.0, 3.0, 3.0])), None, [0.0, 0.0], [1.0 + 0j] * 2,
                              sampling_width=1.0, n_chains=n, seed=1, dtype="f64", temp=1.0,
                              complex_sample_method="magnitude-phase")
    rng = np.random.default_rng(6)
    u_phase = rng.uniform(0.05, 0.95, (n, 2))
    theta = -dr.PI + 2 * dr.PI * u_phase.astype(LD)
    d = 2 * (np.sin(theta) ** 2).sum(axis=1)
    p = np.exp(-d)
    want = rng.integers(0, 2, n).astype(bool)
    u_ph = (p * np.where(want, 1 - LD(1e-9), 1 + LD(1e-9))).astype(np.float64)
    uniforms = np.column_stack((np.where(want, 2.0, 0.0), u_phase, u_ph))
    eng.step_injected(np.zeros((1, n, 2)), uniforms[None], kind=_capi.STEP_COMPLEX_MAGNITUDE_PHASE)
    x = eng._get(_capi.FIELD_PARAMS)
    moved = x[:, 4] != 0                                    # Im z_0 left 0
    assert np.array_equal(moved, want)
    z = x[:, 2:4] + 1j * x[:, 4:6]
    assert np.abs(phase_errors(z[want], theta[want])).max() < 1e-14
    assert eng.accept_stats() == (n + int(want.sum()), 2 * n)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_magnitude_phase_accept_words_on_the_engines_own_draws(dtype):
    """Words W1 and W1+nc+1 of the Philox stream are the accept draws of the two stages: (2, 2) with
    E = x^T diag(1, 1, 8, 8, 9, 9) x at T = 1 from z = 1, width 1/4.  Magnitude stage: d = 8 sum (m_j^2 - 1), m = 1 + g/16;
    phase stage: d = sum c_j^2 sin^2 theta_j at the magnitudes c the first stage left.  Both decisions show in z (its
    magnitudes, its phases) and must be the reference's outside a coarse tie band -- this is a layout check, the thresholds
    are the other tests': 1e-12 in float64; 5e-5 in float32, ten times what the float32 bounds allow in p <= 1 (normals
    5e-7 in d, roundings of an energy near 20 a few eps32 E = 4e-6, phases 4e-7 rad).  A stage that read the other
    stage's word would differ on a tenth of the chains and more (asserted from the reference)."""
    nr, nc = 2, 2
    eng = fresh_engine(me.DenseQuadratic(np.diag([1.0, 1.0, 8.0, 8.0, 9.0, 9.0])), nr, nc, dtype, 0, width=PHASE_WIDTH,
                       z0=1.0 + 0j, temp=1.0, complex_sample_method="magnitude-phase")
    eng.step_complex_group()
    x = eng._get(_capi.FIELD_PARAMS)
    stats = eng.accept_stats()
    eng.sync()
    z = x[:, nr:nr + nc] + 1j * x[:, nr + nc:]
    w, g, _ = stream_reference(0, dtype, SEED, N)
    _, mag_word, first_phase, phase_word, _ = dr.magphase_words(nc)
    band = 1e-12 if dtype == "f64" else 5e-5
    m = 1 + g[:, :nc] / 16
    u_mag, u_phase = dr.units(w[:, mag_word], dtype), dr.units(w[:, phase_word], dtype)
    d1 = 8 * (m * m - 1).sum(axis=1)
    acc1, tie1, _ = dr.accept_reference(d1, u_mag, 1.0, dtype, band)
    cur = np.where(acc1[:, None], m, LD(1))
    theta = dr.phases(w[:, first_phase:first_phase + nc], dtype)
    d2 = (cur * cur * np.sin(theta) ** 2).sum(axis=1)
    acc2, tie2, _ = dr.accept_reference(d2, u_phase, 1.0, dtype, band)
    # what the device decided, read off the state
    mag = np.abs(z).astype(LD)
    got1 = np.abs(mag - m).max(axis=1) < np.abs(mag - 1).max(axis=1)
    far = np.abs(theta).argmax(axis=1)[:, None]             # the parameter whose new phase is farthest from the old one, 0
    z_far, theta_far = np.take_along_axis(z, far, 1)[:, 0], np.take_along_axis(theta, far, 1)[:, 0]
    got2 = np.abs(phase_errors(z_far, theta_far)) < np.abs(phase_errors(z_far, LD(0) * theta_far))
    clear1 = ~tie1 & (np.abs(m - 1).max(axis=1) > 1e-3)
    clear2 = clear1 & ~tie2 & (np.abs(theta_far) > 1e-3)
    assert clear2.mean() > 0.98
    assert np.array_equal(got1[clear1], acc1[clear1])
    assert np.array_equal(got2[clear2], acc2[clear2])
    assert 0.1 < acc1.mean() < 0.9 and 0.1 < acc2.mean() < 0.9
    assert stats == (int(got1.sum()) + int(got2.sum()), 2 * N)
    swapped1, _, _ = dr.accept_reference(d1, u_phase, 1.0, dtype, band)
    swapped2, _, _ = dr.accept_reference(d2, u_mag, 1.0, dtype, band)
    assert (swapped1 != acc1).mean() > 0.1 and (swapped2 != acc2).mean() > 0.1


ACCEPT_PARAMS = [pytest.param(shape, temp, dtype, id="%d-%d-%s-%s" % (shape + (dtype, "ladder" if np.ndim(temp) else "T%g" % temp)))
                 for dtype in ("f32", "f64") for shape in sorted(dr.ACCEPT_SHAPES) for temp in dr.ACCEPT_TEMPS]


@pytest.mark.parametrize("shape,temp,dtype", ACCEPT_PARAMS)
def test_accept_decisions_on_the_engines_own_draws(shape, temp, dtype):
    """DiagQuadratic from x0 = 0, width 1, 2^16 chains, one step: a chain moved iff the reference accepts, on every chain
    outside the tie band; accepted chains hold their reference proposal; accept_stats() counts the chains that moved.  At
    T = 1e-3 (dE/T in the thousands) nothing is accepted and no status bit is raised."""
    nr, nc = shape
    a, b = dr.ACCEPT_SHAPES[shape]
    kw = dict(temperatures=list(temp)) if np.ndim(temp) else dict(temp=temp)
    eng = me.MetropolisEngine(me.DiagQuadratic(a, b), None, [0.0] * nr, [0j] * nc if nc else None, sampling_width=1.0,
                              n_chains=dr.ACCEPT_CHAINS, seed=dr.ACCEPT_SEED, dtype=dtype, chain_offset=dr.ACCEPT_OFFSET,
                              cov_mode="fixed", **kw)
    g, accept, tie, _ = dr.accept_case_reference(nr, nc, temp, dtype, (dr.FLOAT32_A, dr.FLOAT32_B))
    assert tie.mean() <= dr.ACCEPT_TIE_CAP[dtype]
    eng.step_all(1)
    x = eng._get(_capi.FIELD_PARAMS)
    moved = x.any(axis=1)
    wrong = (moved != accept) & ~tie
    assert not wrong.any(), "%d decisions differ from the reference" % int(wrong.sum())
    assert eng.accept_stats() == (int(moved.sum()), dr.ACCEPT_CHAINS)
    eng.sync()                                              # no status bit
    if np.ndim(temp) == 0 and temp == 1e-3:
        assert not moved.any()
    else:
        tol = 1e-14 if dtype == "f64" else 1e-5
        assert np.abs(x[moved].astype(LD) - g[moved]).max() < tol      # (the per-value bounds are the normals tests')
