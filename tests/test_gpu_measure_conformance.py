"""GPU conformance of EVERY form of the measure() recursion -- running mean, running observables, the covariance update
C <- C (i-2)/(i-1) + delta delta^H / i + (w^2 / i) I -- entry by entry against tests/measure_reference.py (long double, exact
rationals of i): |got - S| <= gamma_k A with k = 4 (mean), 6 (observables), 8 (covariance), derived there from the
kernels' spelling, and BIT FOR BIT on the two integer classes.  Then the width adaptation of every step-kernel family to
1 ulp of w (1 + ratio (1 - p) / damping) / w (1 - ratio p / damping).

How a kernel is handed chosen inputs (checkpoint surface only, as tests/test_gpu_cholesky_conformance.py): the engine's
``state_dict`` is rewritten -- ``params``, ``mean``, ``obs_mean``, ``cov``, ``width``, ``measure_step_counter`` = i - 1 (loading
``width`` into a mixed engine marks its three rows as split) -- loaded, ``measure()`` called once, every field read back.

Case -> kernel (dispatch: csrc/me_kernels.hip ``measure`` / ``cycle``, csrc/me_runtime_dims.hip ``launch_measure``):

    register   (1,0) (16,0) (17,0) (4,4) (2,7) (0,12)   measure_chain's register path in k_measure, fused with the factor
    stream     (33,0) (64,0) (65,0) (1,13) (0,13) (20,6) covariance_walk through k_measure's STREAM path: (33,0) has rows ending in
                                                         the 16 + 4 + 3 tails, (64,0) a tile-major state, (0,13) the 8-pair batch
    tracked    (4,4) (64,0)                              cov_mode="fixed", track_covariance=True: the recursion without a factor
    fixed      (16,0) (2,7)                              cov_mode="fixed" on a register-resident set: the engine keeps the matrices
                                                         all the same (decide_layout, csrc/me_api.hip), so this is the recursion
                                                         again, never followed by a factor -- the factor field stays bitwise
    nocov      (64,0) (20,6)                             cov_mode="fixed" on a streamed set: no covariance field, the
                                                         no-covariance instantiation of k_measure (means, observables)
    runtime    (129,0) (125,4) reference, (100,12) tracked: k_measure_runtime_cov (runtime_means_and_observables +
               covariance_walk); (130,0) fixed: k_measure_runtime
    threshold  (4,4) at i = 50 (no covariance update, no factor) and i = 51 (49/50 kept, factor refreshed)
    policy     one case per compile-time path with me.set_cache_budget(0) (the NT / NTM instantiations of k_measure, k_cycle
               and the factor kernels) and with a budget between the means and the whole working set (NT without NTM):
               every field bitwise equal to the default-policy run.  The runtime-dimension set has one cache policy.

Every case runs in float32 and float64, over every class of measure_reference.CLASSES (scaled and offset at i = 52,
10^4 + 1 and 10^6 + 3), with a ragged chain count (2 x 64 + 7; 64 + 7 beyond 64 degrees of freedom), and prints its largest ratio
per quantity (``pytest -s``).  x and the widths must come back bitwise untouched, and so must the covariance and the factor
wherever none is due.
"""
import numpy as np
import pytest

import cholesky_reference as cr
import measure_reference as mr
import metropolisengine_amd as me
from metropolisengine_amd import _capi

pytestmark = pytest.mark.gpu
LD = mr.LD
DEFAULT_BUDGET = 224 << 20

REGISTER = [(1, 0), (16, 0), (17, 0), (4, 4), (2, 7), (0, 12)]
STREAM = [(33, 0), (64, 0), (65, 0), (1, 13), (0, 13), (20, 6)]
MODES = {"reference": {}, "tracked": dict(cov_mode="fixed", track_covariance=True), "fixed": dict(cov_mode="fixed")}
CASES = ([pytest.param(nr, nc, "reference", id="register-%d-%d" % (nr, nc)) for nr, nc in REGISTER] +
         [pytest.param(nr, nc, "reference", id="stream-%d-%d" % (nr, nc)) for nr, nc in STREAM] +
         [pytest.param(nr, nc, "tracked", id="tracked-%d-%d" % (nr, nc)) for nr, nc in [(4, 4), (64, 0)]] +
         [pytest.param(nr, nc, "fixed", id="fixed-%d-%d" % (nr, nc)) for nr, nc in [(16, 0), (2, 7)]] +
         [pytest.param(nr, nc, "fixed", id="nocov-%d-%d" % (nr, nc)) for nr, nc in [(64, 0), (20, 6)]] +
         [pytest.param(129, 0, "reference", id="runtime-129-0"), pytest.param(125, 4, "reference", id="runtime-125-4"),
          pytest.param(100, 12, "tracked", id="runtime-tracked-100-12"), pytest.param(130, 0, "fixed", id="runtime-nocov-130-0")])
INPUTS = ([(name, None) for name in mr.EXACT_COUNT] + [(name, count) for name in ("scaled", "offset") for count in mr.SCALED_COUNTS])
QUANTITIES = ("mean", "obs_mean", "cov")


def n_chains_for(nr, nc):
    return 2 * 64 + 7 if nr + 2 * nc <= 64 else 64 + 7


def build_engine(nr, nc, dtype, mode, n=None):
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * nr if nr else None, [0.1 + 0.1j] * nc if nc else None, temp=1.0,
                              n_chains=n or n_chains_for(nr, nc), seed=7, dtype=dtype, sampling_width=0.1, **MODES[mode])
    assert eng.cov_mode == ("reference" if mode == "reference" else "fixed")
    return eng


def marker_factor(n, nr, nc):
    """A recognisable factor to load: (chain + 2) x the identity."""
    return cr.packed_identity(n, nr, nc) * (2.0 + np.arange(n))[:, None]


def keeps_covariance(nr, nc, mode):
    """Which engines keep a per-chain covariance field (csrc/me_api.hip decide_layout): every reference-mode and tracking
    engine, and every register-resident kernel set (at most 160 packed entries) WHATEVER its cov_mode -- those track the
    matrix on the side and never factorise it; a streamed or runtime-dimension set with cov_mode="fixed" keeps none."""
    return mode != "fixed" or (nr + 2 * nc <= 128 and cr.packed_size(nr, nc) <= 160)


def load_inputs(eng, inp, mode, factor=None):
    """The engine's checkpoint rewritten with one measure()'s inputs; returns what was loaded."""
    state = eng.state_dict()
    for key, field in (("params", "x"), ("mean", "mean"), ("obs_mean", "obs_mean"), ("width", "width")):
        assert state[key].shape == inp[field].shape, key
        state[key] = inp[field]
    assert ("cov" in state) == keeps_covariance(inp["nr"], inp["nc"], mode)
    if "cov" in state:
        assert state["cov"].shape == inp["cov"].shape
        state["cov"] = inp["cov"]
    if "factor" in state:
        state["factor"] = marker_factor(eng.n_chains, inp["nr"], inp["nc"]) if factor is None else factor
        state["uses_per_chain_factors"] = True
    state["measure_step_counter"] = inp["count"] - 1
    eng.load_state_dict(state)
    return state


def one_measure(eng, inp, mode):
    loaded = load_inputs(eng, inp, mode)
    eng.measure()
    eng.sync()                                   # raises on a status bit (a bad pivot, a non-finite value)
    assert eng.measure_step_counter == inp["count"]
    return loaded, eng.state_dict()


def check_measure(loaded, after, inp, name, dtype, mode, what, worst):
    """Every field of one measure() against the reference; ``worst`` collects the largest ratio per quantity."""
    ref = mr.reference(inp)
    assert np.array_equal(after["params"], inp["x"]), what
    assert np.array_equal(after["width"], inp["width"]), what
    assert ("cov" in after) == keeps_covariance(inp["nr"], inp["nc"], mode)
    cov_due = "cov" in after and inp["count"] > 50
    factor_due = cov_due and mode == "reference"
    if "cov" in after and not cov_due:
        assert np.array_equal(after["cov"], inp["cov"]), what
    if "factor" in after:
        if factor_due:
            assert np.all(np.isfinite(after["factor"])) and not np.array_equal(after["factor"], loaded["factor"]), what
        else:
            assert np.array_equal(after["factor"], loaded["factor"]), what
    for q in QUANTITIES:
        if q == "cov" and not cov_due:
            continue
        s, a = ref[q]
        if name == "integers_rank_one" or (name == "integers_keep" and q == "cov"):
            same = mr.exact(after[q], s)
            assert same.all(), "%s %s: %d entries differ from the exact value, first (chain, entry) %s" % (
                what, q, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        else:
            r = mr.ratio(after[q], s, a, mr.K[q], dtype)
            worst[q] = max(worst.get(q, 0.0), float(r.max()))
            assert np.all(r <= 1), "%s %s: ratio %.4g at (chain, entry) %s" % (what, q, float(r.max()), np.argwhere(r > 1)[:4].tolist())
    if name == "integers_keep" and cov_due:
        assert np.array_equal(after["cov"] * 64, inp["cov"] * 63), what


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc,mode", CASES)
def test_one_measure_meets_the_per_entry_bounds(nr, nc, mode, dtype):
    eng = build_engine(nr, nc, dtype, mode)
    worst = {}
    for index, (name, count) in enumerate(INPUTS):
        inp = mr.make_inputs(name, eng.n_chains, nr, nc, dtype, count, seed=100 + index)
        loaded, after = one_measure(eng, inp, mode)
        check_measure(loaded, after, inp, name, dtype, mode, "(%d,%d) %s %s %s i=%d" % (nr, nc, mode, dtype, name, inp["count"]), worst)
    eng.close()
    print("(%d,%d) %s %s largest ratios: " % (nr, nc, mode, dtype) + ", ".join("%s %.4f" % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_covariance_threshold_at_the_fiftieth_measure(dtype):
    """(4,4): the measure that makes the counter 50 leaves covariance and factor bitwise alone and updates the means; the one
    that makes it 51 keeps 49/50 of the matrix and refreshes the factor (of the matrix it stored, conj(K) in the
    Hermitian block -- held to the Cholesky module's backward-error bound)."""
    nr, nc = 4, 4
    eng = build_engine(nr, nc, dtype, "reference")
    worst = {}
    inp = mr.make_inputs("scaled", eng.n_chains, nr, nc, dtype, 50, seed=50)
    loaded, after = one_measure(eng, inp, "reference")
    check_measure(loaded, after, inp, "scaled", dtype, "reference", "(4,4) i=50 " + dtype, worst)
    assert np.array_equal(after["cov"], inp["cov"]) and np.array_equal(after["factor"], loaded["factor"])
    assert not np.array_equal(after["mean"], inp["mean"]) and "cov" not in worst
    inp = mr.make_inputs("scaled", eng.n_chains, nr, nc, dtype, 51, seed=51)
    loaded, after = one_measure(eng, inp, "reference")
    check_measure(loaded, after, inp, "scaled", dtype, "reference", "(4,4) i=51 " + dtype, worst)
    assert "cov" in worst
    fr, fc = eng.proposal_factors()
    real, cplx = mr.unpack_blocks(after["cov"], nr, nc)
    assert np.all(cr.backward_error_ratio(fr, real, dtype) <= 1)
    assert np.all(cr.backward_error_ratio(fc, np.conj(cplx), dtype, complex_block=True) <= 1)
    print("(4,4) threshold %s largest ratios: " % dtype + ", ".join("%s %.4f" % kv for kv in sorted(worst.items())))


# ------------------------------------------------------------------------------------------------------ cache policy
@pytest.fixture
def cache_budget():
    """The budget is process-wide: whatever a test sets, the default comes back."""
    try:
        yield me.set_cache_budget
    finally:
        me.set_cache_budget(DEFAULT_BUDGET)


def means_bytes(nr, nc, n, dtype):
    """x + means + observables + their updates of a launch: above it the packed fields go non-temporal (NT), the means not yet."""
    return (2 * (nr + 2 * nc) + 2 * nr + nc) * n * (4 if dtype == "f32" else 8)


def same_fields(a, b):
    assert set(a) == set(b)
    return [key for key in a if not np.array_equal(np.asarray(a[key]), np.asarray(b[key]))]


POLICY_CASES = [pytest.param(2, 7, "reference", id="register-2-7"), pytest.param(20, 6, "reference", id="stream-20-6"),
                pytest.param(64, 0, "reference", id="stream-64-0"), pytest.param(65, 0, "reference", id="stream-65-0"),
                pytest.param(4, 4, "tracked", id="tracked-4-4"), pytest.param(16, 0, "fixed", id="fixed-16-0"),
                pytest.param(64, 0, "fixed", id="nocov-64-0")]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc,mode", POLICY_CASES)
def test_cache_policy_does_not_change_a_bit_of_measure(nr, nc, mode, dtype, cache_budget):
    eng = build_engine(nr, nc, dtype, mode)
    inp = mr.make_inputs("scaled", eng.n_chains, nr, nc, dtype, 10 ** 4 + 1, seed=77)
    loaded, default = one_measure(eng, inp, mode)
    check_measure(loaded, default, inp, "scaled", dtype, mode, "(%d,%d) default policy" % (nr, nc), {})
    for budget in (0, means_bytes(nr, nc, eng.n_chains, dtype)):
        cache_budget(budget)
        _, streamed = one_measure(eng, inp, mode)
        assert same_fields(default, streamed) == [], budget
        cache_budget(DEFAULT_BUDGET)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc", [(4, 4), (16, 0)], ids=["cycle-4-4", "cycle-16-0"])
def test_cache_policy_does_not_change_a_bit_of_cycle(nr, nc, dtype, cache_budget):
    """k_cycle: one sweep with each chain's own factor, then measure_chain -- state, energies, widths, means, observables,
    covariance and factor of the NT / NTM instantiations equal the default ones bit for bit."""
    runs = []
    for budget in (DEFAULT_BUDGET, 0, means_bytes(nr, nc, n_chains_for(nr, nc), dtype)):
        cache_budget(budget)
        eng = build_engine(nr, nc, dtype, "reference")
        inp = mr.make_inputs("scaled", eng.n_chains, nr, nc, dtype, 10 ** 4 + 1, seed=78)
        load_inputs(eng, inp, "reference", factor=cr.packed_identity(eng.n_chains, nr, nc))
        eng.initialize_energy_dict()                        # the energy ledger of the loaded state
        eng.cycle(1)
        assert eng.fused_cycles() == 1
        stats = eng.accept_stats()
        eng.sync()
        runs.append((eng.state_dict(), stats))
        eng.close()
    moved = ~np.all(runs[0][0]["params"] == inp["x"], axis=1)
    assert 0 < moved.sum() < moved.size                     # the sweep decided both ways
    for state, stats in runs[1:]:
        assert same_fields(runs[0][0], state) == [] and stats == runs[0][1]


# ------------------------------------------------------------------------------------------------------ width adaptation
WIDTH_CHAINS = 200
WIDTH_CASES = [
    # id, builder, (nr, nc), dtypes, action
    ("identity", "identity", (16, 0), ("f32", "f64"), "step_all"),                      # k_step, identity shape
    ("register-per-chain", "per_chain", (4, 4), ("f32", "f64"), "step_all"),            # register-resident per-chain factor
    ("streamed-factor", "per_chain", (16, 0), ("f64",), "step_all"),                    # 136 entries > kStreamF64Entries
    ("streamed-factor", "per_chain", (24, 0), ("f32",), "step_all"),                    # 300 entries > 160
    ("runtime", "identity", (130, 0), ("f32", "f64"), "step_all"),                      # k_step_runtime
    ("runtime-lds", "per_chain", (140, 0), ("f32", "f64"), "step_all"),                 # k_step_runtime_lds<CK_PER_CHAIN>
    ("dense64", "dense64", (64, 0), ("f32", "f64"), "step_all"),                        # me_dense_f64.h / split-bf16 on me_dense64.h
    ("magphase", "magphase", (2, 2), ("f32", "f64"), "complex_group"),                  # k_step_magphase
    ("mixed-step-all", "identity", (4, 4), ("f32", "f64"), "step_all"),                 # all three rows end up equal
    ("mixed-real-group", "identity", (4, 4), ("f32", "f64"), "real_group"),
    ("mixed-complex-group", "identity", (4, 4), ("f32", "f64"), "complex_group"),
    ("cycle", "reference", (4, 4), ("f32", "f64"), "cycle"),                            # k_cycle
]
WIDTH_PARAMS = [pytest.param(builder, shape, dtype, action, id="%s-%d-%d-%s" % ((ident,) + shape + (dtype,)))
                for ident, builder, shape, dtypes, action in WIDTH_CASES for dtype in dtypes]


def width_engine(builder, nr, nc, dtype, reject):
    """An engine on the step kernel that ``builder`` selects (as tests/test_gpu_draw_conformance.py selects them), at x = 0
    (z = 1 for the magnitude-phase sampler), whose every proposal is accepted -- a flat energy -- or, with ``reject``, refused
    by the hard wall |x_0| >= 0."""
    wall = me.AbsReal0AtLeast(0.0) if reject else None
    kw = dict(sampling_width=1.0, n_chains=WIDTH_CHAINS, seed=11, dtype=dtype, temp=1.0)
    x0, z0 = [0.0] * nr, ([0j] * nc if nc else None)
    if builder == "identity":
        return me.MetropolisEngine(me.IsoQuadratic(0.0), wall, x0, z0, cov_mode="fixed", **kw)
    if builder == "reference":
        return me.MetropolisEngine(me.IsoQuadratic(0.0), wall, x0, z0, **kw)
    if builder == "magphase":
        return me.MetropolisEngine(me.IsoQuadratic(0.0), wall, x0, [1.0 + 0j] * nc, complex_sample_method="magnitude-phase", **kw)
    if builder == "dense64":
        kw["temp"] = 1e30                                    # exp(-dE / T) rounds to 1: every uphill move is accepted
        return me.MetropolisEngine(me.DenseQuadratic(np.identity(64)), wall, x0, None, cov_mode="fixed", **kw)
    assert builder == "per_chain"
    eng = me.MetropolisEngine(me.IsoQuadratic(0.0), wall, x0, z0, covariance_matrix_real=np.identity(nr) if nr else None,
                              covariance_matrix_complex=np.identity(nc) if nc else None, **kw)
    assert eng.cov_mode == "reference"
    eng._set(_capi.FIELD_FACTOR, cr.packed_identity(1, nr, nc))       # writing a row of the field selects the per-chain kernels
    return eng


def ulp_error(got, ref, dtype):
    """|got - ref| in units in the last place of ``ref`` in ``dtype`` (long double)."""
    _, e = np.frexp(ref)
    return np.abs(got.astype(LD) - ref) / np.ldexp(LD(1), e - (24 if dtype == "f32" else 53))


@pytest.mark.parametrize("builder,shape,dtype,action", WIDTH_PARAMS)
def test_width_adaptation_to_one_ulp(builder, shape, dtype, action):
    """One step through each step-kernel family at 200 chains whose widths spread over 10^-6 .. 10^6: the new width is
    w (1 + ratio (1 - p) / damping) after an accepted proposal and w (1 - ratio p / damping) after a refused one, damping =
    max(measure_step_counter / m, 200), within 1 ulp of the long-double value.  Why 1 ulp: the increment is below w / 8
    (asserted from the engine's ratio), so the float64 spelling's four roundings of the increment weigh 4 u / 8 of w and
    the float32 spelling's host-rounded constant u / 8, plus half an ulp for the final add / fma -- below one ulp for both.
    step_all leaves the three rows of a mixed engine equal; a group step changes its own row only."""
    nr, nc = shape
    rows = mr.n_width_rows(nr, nc)
    rng = np.random.default_rng(4)
    widths = mr._rounded(10.0 ** rng.uniform(-6.0, 6.0, (WIDTH_CHAINS, rows)), dtype)
    if action == "cycle":
        # a step_all of a mixed engine whose rows differ proposes with the group rows and measures with row 0: the rank-one
        # term then dwarfs the epsilon term and the matrix k_cycle goes on to factorise is singular in float32.  Equal rows.
        widths[:] = widths[:, :1]
    worst = 0.0
    for reject in (False, True):
        eng = width_engine(builder, nr, nc, dtype, reject)
        p, ratio = LD(eng.target_acceptance), LD(eng.ratio)
        for counter in (1, 1000 * eng.m + 7):
            damping = LD(max(counter / eng.m, 200.0))
            assert (counter == 1) == (damping == 200) and ratio * max(p, 1 - p) / damping < LD(1) / 8
            state = eng.state_dict()
            state["width"], state["measure_step_counter"] = widths, counter
            eng.load_state_dict(state)
            before = eng.accept_stats()
            if action == "step_all":
                eng.step_all(1)
            elif action == "real_group":
                eng.step_real_group()
            elif action == "complex_group":
                eng.step_complex_group()
            else:
                eng.cycle(1)
                assert eng.fused_cycles() >= 1
            got = eng._get(_capi.FIELD_WIDTH)
            stats = eng.accept_stats()
            eng.sync()
            decisions = 2 if builder == "magphase" else 1
            assert (stats[0] - before[0], stats[1] - before[1]) == (0 if reject else decisions * WIDTH_CHAINS, decisions * WIDTH_CHAINS)
            row = {"step_all": 0, "cycle": 0, "real_group": 1, "complex_group": 2}[action] if rows == 3 else 0
            old = widths[:, row].astype(LD)
            want = old * (1 - ratio * p / damping) if reject else old * (1 + ratio * (1 - p) / damping)
            err = ulp_error(got[:, row], want, dtype)
            worst = max(worst, float(err.max()))
            assert np.all(err <= 1), (reject, counter, float(err.max()))
            assert np.all(got[:, row] < widths[:, row]) if reject else np.all(got[:, row] > widths[:, row])
            for other in range(rows):
                if other != row:
                    if action in ("step_all", "cycle"):
                        assert np.array_equal(got[:, other], got[:, row])
                    else:
                        assert np.array_equal(got[:, other], widths[:, other])
        eng.close()
    print("%s (%d,%d) %s %s: largest width error %.3f ulp" % (builder, nr, nc, dtype, action, worst))
