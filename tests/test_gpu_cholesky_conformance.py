"""GPU conformance of EVERY Cholesky refresh kernel against the backward-error criterion of tests/cholesky_reference.py:
|C - L L^H|_ij <= gamma_k (|L| |L|^H)_ij -- derived, conditioning-independent -- on chosen matrices instead of the tame
covariances a quadratic energy produces.

How a kernel is handed a chosen matrix (checkpoint surface only): a ``cov_mode="reference"`` engine's ``state_dict`` is
rewritten -- ``cov`` = the crafted packed matrices, ``mean`` = the current parameters (the rank-one term of the recursion
vanishes), ``measure_step_counter`` = 10^4 (> 50; the recursion keeps (i-2)/(i-1) of the old matrix), a sampling width of
1e-30 (the epsilon term w^2 / i is nothing) -- loaded, and ``measure()`` called once.  The kernels factorise the value they
store, so (covariance read back, factor read back) is exactly (input, output) of the factorisation, in the engine's dtype.

Case -> kernel (dispatch: csrc/me_kernels.hip ``measure`` / ``cycle``, csrc/me_runtime_dims.hip ``measure``):

    (1,0) (16,0) (17,0) (4,4) (2,7) (0,12)   cholesky_packed in registers, fused into k_measure (<= 160 packed entries; (17,0)
                                             with 153 and (0,12) with 144 are the largest real / complex ones)
    (4,4) (16,0) through cycle(1)            cholesky_packed fused into k_cycle
    18 31 32                                 k_factor_tile, 32 lanes per chain, two chains per wavefront (18: 171 entries, the
                                             smallest streamed size; 31, 32: the full lane group)
    33 63 64                                 k_factor_tile; float64: 64 lanes per chain, every third broadcast pair through
                                             v_readlane; float32: two rows per lane (33, 63: the last lane owns a phantom row)
    65 96                                    k_factor_stream
    (1,13) (0,13) (20,6)                     k_factor_mixed (real rows, then chol(conj K))
    129 136                                  k_factor_runtime (runtime-dimension set, beyond 128 degrees of freedom)
    (125,4)                                  k_factor_runtime for the real block + k_factor_runtime_complex
    (4,4) warm start                         the host Cholesky of the constructor's matrices (csrc/me_api.hip, double)

Every case runs in float32 and float64, over every class of cholesky_reference.CLASSES, with a ragged chain count
(2 x 64 + 7; 64 + 7 beyond 64 parameters), a different matrix per chain.

Bad pivots: ST_BAD_PIVOT surfaces as FloatingPointError at the next synchronising call and is cleared by it; the engine
stays readable (csrc/me_api.hip report_status), so the good chains are checked in the SAME engine -- and, on top, must be
bitwise what a run without the bad chains gives.
"""
import numpy as np
import pytest

import cholesky_reference as cr
import metropolisengine_amd as me

pytestmark = pytest.mark.gpu

MEASURES = 10 ** 4
TINY_WIDTH = 1e-30

REGISTER = [(1, 0), (16, 0), (17, 0), (4, 4), (2, 7), (0, 12)]
TILE = [(18, 0), (31, 0), (32, 0), (33, 0), (63, 0), (64, 0)]
STREAM = [(65, 0), (96, 0)]
MIXED = [(1, 13), (0, 13), (20, 6)]
RUNTIME = [(129, 0), (136, 0)]
RUNTIME_COMPLEX = [(125, 4)]
CASES = ([pytest.param(nr, nc, id="packed-%d-%d" % (nr, nc)) for nr, nc in REGISTER] +
         [pytest.param(nr, nc, id="tile-%d" % nr) for nr, nc in TILE] +
         [pytest.param(nr, nc, id="stream-%d" % nr) for nr, nc in STREAM] +
         [pytest.param(nr, nc, id="mixed-%d-%d" % (nr, nc)) for nr, nc in MIXED] +
         [pytest.param(nr, nc, id="runtime-%d" % nr) for nr, nc in RUNTIME] +
         [pytest.param(nr, nc, id="runtime-complex-%d-%d" % (nr, nc)) for nr, nc in RUNTIME_COMPLEX])


def n_chains_for(nr, nc):
    return 2 * 64 + 7 if nr + 2 * nc <= 64 else 64 + 7


def craft(name, n, nr, nc, dtype, seed):
    real = cr.make_class(name, n, nr, dtype, seed=seed) if nr else None
    cplx = cr.make_class(name, n, nc, dtype, complex_block=True, seed=seed) if nc else None
    return real, cplx


def refresh(nr, nc, dtype, real, cplx, n, cycle=False, width=TINY_WIDTH):
    """One refresh of the per-chain factors from the crafted matrices (module docstring).  Returns the engine with the
    launch enqueued; the first synchronising call reports a bad pivot."""
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * nr if nr else None, [0.1 + 0.1j] * nc if nc else None,
                              temp=1.0, n_chains=n, seed=7, dtype=dtype, sampling_width=width)
    assert eng.cov_mode == "reference"
    state = eng.state_dict()
    packed = cr.pack(real, cplx)
    assert packed.shape == state["cov"].shape
    state["cov"] = packed
    state["mean"] = state["params"].copy()
    state["factor"] = cr.packed_identity(n, nr, nc)
    state["measure_step_counter"] = MEASURES
    state["uses_per_chain_factors"] = True
    eng.load_state_dict(state)
    if cycle:
        eng.cycle(1)
        assert eng.fused_cycles() == 1                     # the one-launch k_cycle, not a step and a measure launch
    else:
        eng.measure()
    return eng


def check_input_survived(read, crafted, dtype, width=TINY_WIDTH):
    """The matrix the kernel factorised is the crafted one times (i-2)/(i-1), entry by entry to two roundings (plus the
    epsilon term on the diagonal): its class -- scale, grading, near-singularity -- is the intended one."""
    keep = (MEASURES - 1.0) / MEASURES
    u = cr.UNIT_ROUNDOFF[dtype]
    tol = 4 * u * np.abs(crafted)
    tol[:, np.arange(crafted.shape[1]), np.arange(crafted.shape[1])] += 2 * width * width / MEASURES
    assert np.all(np.abs(read - keep * crafted) <= tol)


def check_block(fac, cov_read, dtype, good, complex_block, well_conditioned, what):
    """The assertions on one block of the good chains; returns the largest ratio."""
    m = fac.shape[1]
    target = np.conj(cov_read) if complex_block else cov_read          # the proposals factorise conj(K) (quirk Q3)
    assert np.all(np.triu(fac, 1) == 0), what                          # (every chain: nothing is ever written there)
    assert np.all(np.isfinite(fac[good])), what
    diag = fac[good][:, np.arange(m), np.arange(m)]
    assert np.all(diag.imag == 0) and np.all(diag.real > 0), what
    ratio = cr.backward_error_ratio(fac[good], target[good], dtype, complex_block)
    print("%s %s: largest backward-error ratio %.4f" % (what, dtype, float(ratio.max())))
    assert np.all(ratio <= 1), (what, np.flatnonzero(good)[np.flatnonzero(ratio > 1)], ratio.max())
    if well_conditioned:
        if complex_block:
            _, ref, bad = cr.reference_factor(None, cov_read[good])
        else:
            ref, _, bad = cr.reference_factor(cov_read[good], None)
        assert not bad.any(), what
        bound = cr.trace_condition(target[good], ref) * cr.gamma(m, dtype, complex_block)
        assert np.all(cr.factor_distance(fac[good], ref) <= bound), what
    return float(ratio.max())


def check_engine(eng, nr, nc, dtype, real, cplx, good, well_conditioned, what, width=TINY_WIDTH, exact_input=True):
    fr, fc = eng.proposal_factors()
    worst = 0.0
    if nr:
        cov = eng.covariance_matrix_real
        if exact_input:
            check_input_survived(cov, real, dtype, width)
        worst = max(worst, check_block(fr, cov, dtype, good, False, well_conditioned, what + " real block"))
    if nc:
        cov = eng.covariance_matrix_complex
        if exact_input:
            check_input_survived(cov, cplx, dtype, width)
        worst = max(worst, check_block(fc, cov, dtype, good, True, well_conditioned, what + " complex block"))
    return worst


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc", CASES)
def test_factor_kernels_meet_the_backward_error_bound(nr, nc, dtype):
    """Every matrix class through measure(): ratio <= 1 for every chain, lower-triangular factor with a positive real
    diagonal, and on the well-conditioned classes agreement with the long-double factor to cond_tr(C) gamma_k."""
    n = n_chains_for(nr, nc)
    good = np.ones(n, dtype=bool)
    for index, name in enumerate(cr.CLASSES):
        real, cplx = craft(name, n, nr, nc, dtype, seed=100 + index)
        eng = refresh(nr, nc, dtype, real, cplx, n)
        eng.sync()
        check_engine(eng, nr, nc, dtype, real, cplx, good, name in cr.WELL_CONDITIONED, "(%d,%d) %s" % (nr, nc, name))
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc", [(4, 4), (16, 0)], ids=["cycle-4-4", "cycle-16-0"])
def test_fused_cycle_factorisation_meets_the_bound(nr, nc, dtype):
    """cholesky_packed as instantiated in k_cycle: one sweep moves the chains first, so the matrix read back is the crafted
    one plus the rank-one term -- still exactly what was factorised."""
    n = n_chains_for(nr, nc)
    real, cplx = craft("spd", n, nr, nc, dtype, seed=200)
    eng = refresh(nr, nc, dtype, real, cplx, n, cycle=True, width=1e-3)
    eng.sync()
    check_engine(eng, nr, nc, dtype, real, cplx, np.ones(n, dtype=bool), True, "(%d,%d) cycle" % (nr, nc), exact_input=False)
    for block, crafted in ((eng.covariance_matrix_real, real), (eng.covariance_matrix_complex, cplx)):
        if crafted is not None:                            # the class survived: the added terms are of order width^2 / i
            assert np.allclose(block, crafted, rtol=2e-4, atol=1e-8)


BAD_CASES = [pytest.param(16, 0, id="packed-16-0"), pytest.param(4, 4, id="packed-4-4"), pytest.param(18, 0, id="tile-18"),
             pytest.param(32, 0, id="tile-32"), pytest.param(33, 0, id="tile-33"), pytest.param(64, 0, id="tile-64"),
             pytest.param(65, 0, id="stream-65"), pytest.param(1, 13, id="mixed-1-13"), pytest.param(20, 6, id="mixed-20-6"),
             pytest.param(129, 0, id="runtime-129"), pytest.param(125, 4, id="runtime-complex-125-4")]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc", BAD_CASES)
def test_a_bad_pivot_is_reported_and_leaves_the_other_chains_intact(nr, nc, dtype):
    """Chains 0, 70, 71 and the last one get an indefinite matrix (70 and 71 share a wavefront in every kernel and a lane
    pair / workgroup / LDS slab in k_factor_tile; the last chain sits in the ragged tile).  The failure surfaces once, every
    other chain passes the bound in the same engine, and their factors equal, bit for bit, those of a run without bad chains."""
    n = 2 * 64 + 7
    bad = [0, 70, 71, n - 1]
    good = np.ones(n, dtype=bool)
    good[bad] = False
    real, cplx = craft("spd", n, nr, nc, dtype, seed=300)
    real_bad, cplx_bad = real, cplx
    if nr and nc:              # a mixed space: chains 0 and 71 fail in the real block, 70 and the last in the Hermitian block
        real_bad, cplx_bad = cr.make_indefinite(real, [0, 71]), cr.make_indefinite(cplx, [70, n - 1])
    elif nr:
        real_bad = cr.make_indefinite(real, bad)
    else:
        cplx_bad = cr.make_indefinite(cplx, bad)
    _, _, flagged = cr.reference_factor(real_bad, cplx_bad)
    assert np.array_equal(flagged, ~good)
    eng = refresh(nr, nc, dtype, real_bad, cplx_bad, n)
    with pytest.raises(FloatingPointError):
        eng.sync()
    eng.sync()                                             # reported once, then cleared
    check_engine(eng, nr, nc, dtype, real_bad, cplx_bad, good, True, "(%d,%d) with bad chains" % (nr, nc))
    clean = refresh(nr, nc, dtype, real, cplx, n)
    clean.sync()
    for with_bad, without in zip(eng.proposal_factors(), clean.proposal_factors()):
        assert np.array_equal(with_bad[good], without[good])
    check_engine(clean, nr, nc, dtype, real, cplx, np.ones(n, dtype=bool), True, "(%d,%d) bad chains replaced" % (nr, nc))


@pytest.mark.parametrize("name", ["spd", "graded_up", "graded_down", "scale_small", "scale_large"])
def test_host_factor_of_warm_start_matrices(name):
    """The constructor's covariance matrices are factorised on the host in double and broadcast to every chain."""
    nr, nc, n = 4, 4, 7
    real, cplx = craft(name, 1, nr, nc, "f64", seed=400)
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * nr, [0.1j] * nc, temp=1.0, n_chains=n, dtype="f64",
                              covariance_matrix_real=real[0], covariance_matrix_complex=cplx[0])
    fr, fc = eng.proposal_factors()
    assert np.array_equal(eng.covariance_matrix_real, np.broadcast_to(real, (n, nr, nr)))
    assert np.array_equal(eng.covariance_matrix_complex, np.broadcast_to(cplx, (n, nc, nc)))
    everyone = np.ones(n, dtype=bool)
    well = name in cr.WELL_CONDITIONED
    check_block(fr, np.broadcast_to(real, (n, nr, nr)), "f64", everyone, False, well, "host %s real block" % name)
    check_block(fc, np.broadcast_to(cplx, (n, nc, nc)), "f64", everyone, True, well, "host %s complex block" % name)
