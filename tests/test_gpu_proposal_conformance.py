"""Every per-chain proposal ``x' = x + w L g`` and every built-in energy ``E(x')``, value by value, against
tests/proposal_reference.py (long double; the criterion, the counted k of each spelling and the input classes are in its
docstring).

The probe is the one of the draw and dense-product modules: crafted x, every ledger row a huge finite value (every proposal
is accepted), the factor field written for all chains (``eng._set(FIELD_FACTOR, rows)`` on an engine built with identity
covariances, cov_mode "reference"; ``set_shared_factor`` for the shared case), one step, ``accept_stats()`` = (n, n) and a
clean ``sync()``, x' read back.  g is what an identity-shape engine of the same space, seed, chain ids and step counter
leaves after one accepted step from x = 0 with the width 2^-4 (``identity_state``).  2 x 64 + 7 chains (3 x 64 + 7 where a
space has more than 135 rows): a ragged last tile is always there.

    case        shapes                                                      path
    register    (4,4) (2,7) (0,12); (13,0) f64; (16,0) (17,0) f32           propose_registers, CK_PER_CHAIN
    budget 0    (4,4) (2,7) with set_cache_budget(0)                        CK_PER_CHAIN_NT: the bits of the default policy
    shared      (16,0) (2,7), cov_mode="pooled" + set_shared_factor         CK_SHARED in the generic k_step
    streamed    (14,0) (16,0) f64; (24,0) f32; (33,0) (64,0) (1,13) (0,13)  the streamed-factor body of k_step: 105 entries (the
                (20,6) both                                                 first float64 size past kStreamF64Entries), rows that
                                                                            end on a chunk edge, complex rows after the triangle
    groups      (4,4) register, (20,6) streamed, (125,4) runtime            step_real_group / step_complex_group: the moving group
                                                                            uses ITS width row, the resting one comes back bitwise
    cycle       (4,4) (16,0) f32, cycle(1) past the 50th measure            k_cycle: x' from the factor as loaded, not the one the
                                                                            same launch refreshes
    runtime     (129,0) (130,0) (125,4) (100,12) (140,0)                    k_step_runtime_lds<CK_PER_CHAIN>: row tails of 1 and 2, a
                                                                            Philox block across the end of the real parameters, the
                                                                            8-row complex batch with its tail, shadow lanes
    injected    (4,4) (2,7) f64, class integers, all three step kinds       the INJECT instantiations
    magphase    (2,2) both dtypes, (0,3) f64                                k_step_magphase, magnitude stage (see the two tests)

Energy leg, same probe with the width 2^-100 / 2^-200 (x' = x bit for bit; the ledger read back is the kernel's E(x)):
EnergyIso / EnergyDiag at (16,0) (3,0) (2,1) (4,4) (33,0) and (33,0) through the streamed-factor body; the streamed loops of
k_step_runtime at (130,0) (101,0) (60,25) with the group steps, of k_step_runtime_lds at (140,0); EnergyLandau and
EnergyLandauTerms at (2,1); EnergyCylinder at (1,2) and (2,2) -- (1,2) stands in for (1,3), which no kernel set of the
build has; ``initialize_energy_dict()`` (k_init_energy, k_init_energy_runtime) on the same states to the same bound.

Run with -s for the largest |got - S| / (gamma_k A) per path, dtype, block and class (PROPOSAL_GPU / ENERGY_GPU lines)."""
import functools

import numpy as np
import pytest

import proposal_reference as pr
import metropolisengine_amd as me
from metropolisengine_amd import _capi, build

pytestmark = pytest.mark.gpu
LD = pr.LD
SEED = 20261021
OFFSET = (1 << 33) + 29
W0 = 2.0 ** -4
DEFAULT_BUDGET = 224 << 20
BIG = {"f32": 1e30, "f64": 1e300}
TINY_WIDTH = {"f32": 2.0 ** -100, "f64": 2.0 ** -200}
BOTH = ("f32", "f64")
STEPS = {"all": "step_all", "real": "step_real_group", "complex": "step_complex_group"}
GROUP_ROW = {"all": 0, "real": 1, "complex": 2}


def n_chains_for(nr, nc):
    return 3 * 64 + 7 if nr + 2 * nc > 135 else 2 * 64 + 7


def set_step(eng, step, measures=None):
    eng._check(eng._lib.me_set_counters(eng._handle, step, eng._counters()[1] if measures is None else measures))


def zeros(nr, nc):
    return dict(initial_real_params=[0.0] * nr if nr else None, initial_complex_params=[0j] * nc if nc else None)


def make_engine(nr, nc, dtype, mode, energy=None, n=None, **kw):
    """mode: "identity" (cov_mode fixed), "per_chain" (identity covariances: cov_mode reference), "pooled"."""
    if mode == "per_chain":
        kw.update(covariance_matrix_real=np.identity(nr) if nr else None, covariance_matrix_complex=np.identity(nc) if nc else None)
    else:
        kw.update(cov_mode="fixed" if mode == "identity" else "pooled")
    kw.setdefault("temp", 1.0)
    eng = me.MetropolisEngine(me.IsoQuadratic(0.0) if energy is None else energy, None, sampling_width=W0,
                              n_chains=n or n_chains_for(nr, nc), seed=SEED, dtype=dtype, chain_offset=OFFSET, **zeros(nr, nc), **kw)
    assert eng.cov_mode == {"identity": "fixed", "per_chain": "reference", "pooled": "pooled"}[mode]
    return eng


def accepted_step(eng, step, x, width, terms=None):
    """One step from (x, width) in which every chain accepts; returns (x', widths after)."""
    n = eng.n_chains
    set_step(eng, 0)
    before = eng.accept_stats()
    eng._set(_capi.FIELD_PARAMS, x)
    eng._set(_capi.FIELD_ENERGY, np.full((n, len(eng.energy_term_names)), BIG[eng.dtype]) if terms is None else terms)
    eng._set(_capi.FIELD_WIDTH, width)
    step()
    after = eng.accept_stats()
    assert (after[0] - before[0], after[1] - before[1]) == (n, n)
    eng.sync()                                   # raises if a status bit is set
    return eng._get(_capi.FIELD_PARAMS), eng._get(_capi.FIELD_WIDTH)


@functools.lru_cache(maxsize=None)
def identity_state(nr, nc, dtype, n):
    """W0 g (W0 fl(g fl(1/sqrt 2)) in the complex coordinates) of every chain at step 0: computed once per space."""
    eng = make_engine(nr, nc, dtype, "identity", n=n)
    x, _ = accepted_step(eng, eng.step_all, np.zeros((n, nr + 2 * nc)), np.full((n, pr.n_width_rows(nr, nc)), W0))
    eng.close()
    assert np.all(np.isfinite(x)) and np.all(x != 0) and 0.5 < np.std(x[:, :nr] / W0 if nr else x * np.sqrt(2) / W0) < 1.5
    x.setflags(write=False)
    return x


def report(path, nr, nc, dtype, name, r, group="all"):
    print("\nPROPOSAL_GPU path=%s (%d,%d) dtype=%s group=%s class=%s real=%.3f hermitian=%.3f"
          % (path, nr, nc, dtype, group, name, r[:, :nr].max(initial=0), r[:, nr:].max(initial=0)))


def exact_widths(n, nr, nc):
    """Powers of two, another one per group row: [4 W0, W0, 2 W0] (mixed engines use rows 1 and 2 once widths were loaded)."""
    return np.tile(np.array([4 * W0, W0, 2 * W0])[:pr.n_width_rows(nr, nc)], (n, 1)) if nr and nc else np.full((n, 1), W0)


def check_rest(got, widths_after, x, width, nr, nc, group, what):
    """A group step leaves the other group's coordinates and every width row but its own bitwise alone."""
    if group == "all":
        return
    rest = slice(nr, None) if group == "real" else slice(0, nr)
    assert np.array_equal(got[:, rest], x[:, rest]), what
    others = [row for row in range(3) if row != GROUP_ROW[group]]
    assert np.array_equal(widths_after[:, others], width[:, others]), what
    assert not np.array_equal(widths_after[:, GROUP_ROW[group]], width[:, GROUP_ROW[group]]), what      # (its own row adapted)


def run_classes(eng, path, spelling, nr, nc, dtype, group="all", load=None, classes=("one_per_row", "scaled", "cancelling")):
    """The three classes through one engine.  ``load(rows)``: how the factor gets in (default: the per-chain field)."""
    n, d = eng.n_chains, nr + 2 * nc
    ident = identity_state(nr, nc, dtype, n)
    g = ident / W0                                               # exact: W0 is a power of two
    gr, zre, zim = g[:, :nr], g[:, nr:nr + nc], g[:, nr + nc:]
    step = getattr(eng, STEPS[group])
    load = load or (lambda rows: eng._set(_capi.FIELD_FACTOR, rows))
    rest = np.random.default_rng(9).standard_normal((n, d))      # what a resting group holds
    out = {}
    for name in classes:
        if name == "one_per_row":
            rows, width = pr.one_per_row(n, nr, nc), exact_widths(n, nr, nc)
            x = np.zeros((n, d))
        elif name == "scaled":
            x, width, rows = pr.scaled_case(n, nr, nc, dtype, seed=31)
        else:
            x, width, rows = pr.cancelling_case(n, nr, nc, dtype, 32, gr, zre, zim)
        if group != "all":
            keep = slice(nr, None) if group == "real" else slice(0, nr)
            x[:, keep] = pr.to_dtype(rest[:, keep], dtype)
        load(rows)
        got, widths_after = accepted_step(eng, step, x, width)
        what = "%s (%d,%d) %s %s %s" % (path, nr, nc, dtype, group, name)
        check_rest(got, widths_after, x, width, nr, nc, group, what)
        w_r, w_c = pr.widths_used(width, nr, nc)      # (loaded widths of a mixed engine count as split: step_all reads rows 1, 2 too)
        if name == "one_per_row":
            scaled_ident = ident * np.concatenate((w_r[:, None] / W0 * np.ones(nr), w_c[:, None] / W0 * np.ones(2 * nc)), axis=1)
            want = pr.one_per_row_expected(rows, scaled_ident, nr, nc, group, x)
            same = got == want
            assert same.all(), "%s: %d values differ from the exact one, first (chain, coordinate) %s" % (
                what, int((~same).sum()), np.argwhere(~same)[:4].tolist())
        else:
            s, a = pr.proposal_reference(x, w_r, w_c, rows, gr, zre, zim, nr, nc, group)
            r = pr.ratio(got, s, a, pr.k_proposal(spelling, nr, nc), dtype)
            report(path, nr, nc, dtype, name, r, group)
            assert np.all(r <= 1), "%s: ratio %.4g at (chain, coordinate) %s" % (what, float(r.max()), np.argwhere(r > 1)[:4].tolist())
        out[name] = got
    return out


def cases(*groups):
    return [pytest.param(nr, nc, dtype, id="%d-%d-%s" % (nr, nc, dtype)) for shapes, dtypes in groups for nr, nc in shapes for dtype in dtypes]


# ------------------------------------------------------------------------------------------------------ the proposal
@pytest.mark.parametrize("nr,nc,dtype", cases(([(4, 4), (2, 7), (0, 12)], BOTH), ([(13, 0)], ("f64",)), ([(16, 0), (17, 0)], ("f32",))))
def test_register_resident_factor(nr, nc, dtype):
    eng = make_engine(nr, nc, dtype, "per_chain")
    run_classes(eng, "register", "registers", nr, nc, dtype)
    eng.close()


@pytest.mark.parametrize("nr,nc,dtype", cases(([(4, 4), (2, 7)], BOTH)))
def test_register_resident_factor_read_non_temporally(nr, nc, dtype):
    """set_cache_budget(0) sends every launch to CK_PER_CHAIN_NT: the same bits as the default policy, class by class."""
    eng = make_engine(nr, nc, dtype, "per_chain")
    default = run_classes(eng, "register", "registers", nr, nc, dtype)
    try:
        me.set_cache_budget(0)
        streamed = run_classes(eng, "register-nt", "registers", nr, nc, dtype)
    finally:
        me.set_cache_budget(DEFAULT_BUDGET)
    for name in default:
        assert np.array_equal(default[name], streamed[name]), name
    eng.close()


@pytest.mark.parametrize("nr,nc,dtype", cases(([(16, 0), (2, 7)], BOTH)))
def test_shared_factor_in_the_generic_kernel(nr, nc, dtype):
    """One factor for all chains: the one_per_row pattern of chain t is loaded for t = 0 .. max(nr, 2 nc - 1) - 1, one step
    each, so that every packed slot is the live one in some step; the float classes share the row of chain 0."""
    eng = make_engine(nr, nc, dtype, "pooled")
    n, d = eng.n_chains, nr + 2 * nc
    ident = identity_state(nr, nc, dtype, n)
    width = exact_widths(n, nr, nc)
    w_r, w_c = pr.widths_used(width, nr, nc)
    scaled_ident = ident * np.concatenate((w_r[:, None] / W0 * np.ones(nr), w_c[:, None] / W0 * np.ones(2 * nc)), axis=1)
    patterns = pr.one_per_row(max(nr, 2 * nc - 1), nr, nc)
    assert (patterns != 0).any(axis=0).all()
    for t, row in enumerate(patterns):
        eng.set_shared_factor(row)
        got, _ = accepted_step(eng, eng.step_all, np.zeros((n, d)), width)
        same = got == pr.one_per_row_expected(np.tile(row, (n, 1)), scaled_ident, nr, nc)
        assert same.all(), "pattern %d: first (chain, coordinate) %s" % (t, np.argwhere(~same)[:4].tolist())
    shared = lambda rows: eng.set_shared_factor(rows[0])
    g = ident / W0
    for name in ("scaled", "cancelling"):
        if name == "scaled":
            x, width, rows = pr.scaled_case(n, nr, nc, dtype, seed=31)
        else:
            x, width, rows = pr.cancelling_case(n, nr, nc, dtype, 32, g[:, :nr], g[:, nr:nr + nc], g[:, nr + nc:])
        rows = np.tile(rows[0], (n, 1))
        if name == "cancelling":                                  # (x cancels the SHARED row's proposal)
            s0, _ = pr.proposal_reference(np.zeros((n, d)), *pr.widths_used(width, nr, nc), rows, g[:, :nr], g[:, nr:nr + nc], g[:, nr + nc:], nr, nc)
            x = pr.to_dtype(-np.asarray(s0, dtype=np.float64), dtype)
        shared(rows)
        got, _ = accepted_step(eng, eng.step_all, x, width)
        w_r, w_c = pr.widths_used(width, nr, nc)
        s, a = pr.proposal_reference(x, w_r, w_c, rows, g[:, :nr], g[:, nr:nr + nc], g[:, nr + nc:], nr, nc)
        r = pr.ratio(got, s, a, pr.k_proposal("registers", nr, nc), dtype)
        report("shared", nr, nc, dtype, name, r)
        assert np.all(r <= 1), (name, float(r.max()))
    eng.close()


STREAMED = cases(([(14, 0), (16, 0)], ("f64",)), ([(24, 0)], ("f32",)), ([(33, 0), (64, 0), (1, 13), (0, 13), (20, 6)], BOTH))


@pytest.mark.parametrize("nr,nc,dtype", STREAMED)
def test_streamed_factor_body(nr, nc, dtype):
    p = pr.packed_size(nr, nc)
    assert p > 160 or (dtype == "f64" and nc == 0 and p > 96)          # the streamed-factor form of k_step
    eng = make_engine(nr, nc, dtype, "per_chain")
    run_classes(eng, "streamed", "registers", nr, nc, dtype)
    eng.close()


@pytest.mark.parametrize("group", ["real", "complex"])
@pytest.mark.parametrize("path,spelling,nr,nc,dtype", [pytest.param(path, spelling, nr, nc, dtype, id="%s-%d-%d-%s" % (path, nr, nc, dtype))
                                                       for path, spelling, nr, nc in (("register", "registers", 4, 4), ("streamed", "registers", 20, 6),
                                                                                      ("runtime", "runtime", 125, 4)) for dtype in BOTH])
def test_group_steps_move_their_group_with_their_width(path, spelling, nr, nc, dtype, group):
    eng = make_engine(nr, nc, dtype, "per_chain")
    run_classes(eng, path + "-group", spelling, nr, nc, dtype, group)
    eng.close()


@pytest.mark.parametrize("nr,nc", [(4, 4), (16, 0)], ids=["4-4", "16-0"])
def test_cycle_proposes_with_the_factor_as_loaded(nr, nc):
    """k_cycle, float32: cycle(1) taking the 61st measure refreshes the factor field in the SAME launch; x' is the one of
    the factor that was loaded."""
    dtype = "f32"
    eng = make_engine(nr, nc, dtype, "per_chain")
    loaded = {}

    def load(rows):
        eng._set(_capi.FIELD_FACTOR, rows)
        set_step(eng, 0, measures=60)
        loaded["rows"], loaded["fused"] = rows, eng.fused_cycles()

    def cycle():
        eng.cycle(1)
        assert eng.fused_cycles() == loaded["fused"] + 1 and eng.measure_step_counter == 61
        after = eng._get(_capi.FIELD_FACTOR)
        assert np.all(np.isfinite(after)) and not np.array_equal(after, loaded["rows"])

    eng.step_all = cycle                                          # (run_classes steps through STEPS["all"])
    run_classes(eng, "cycle", "registers", nr, nc, dtype, load=load)
    eng.close()


@pytest.mark.parametrize("nr,nc,dtype", cases(([(129, 0), (130, 0), (125, 4), (100, 12), (140, 0)], BOTH)))
def test_runtime_dimension_per_chain_factor(nr, nc, dtype, monkeypatch):
    if nr + 2 * nc <= build.MAX_COMPILED_DOF:
        # per-chain shapes between 96 and 128 degrees of freedom: the runtime-dimension set instead of a compiled one, as
        # tests/test_gpu_runtime_dims.py has it
        monkeypatch.setattr(build, "MAX_COMPILED_DOF", build.MAX_REGISTER_DOF)
        monkeypatch.setattr(build, "build_dims", lambda *a, **k: pytest.fail("the runtime-dimension set needs no compiled kernel set"))
    eng = make_engine(nr, nc, dtype, "per_chain")
    run_classes(eng, "runtime", "runtime", nr, nc, dtype)
    eng.close()


@pytest.mark.parametrize("group", ["all", "real", "complex"])
@pytest.mark.parametrize("nr,nc", [(4, 4), (2, 7)], ids=["4-4", "2-7"])
def test_injected_integers(nr, nc, group):
    """The INJECT instantiations, float64: integer L, g, x and power-of-two widths -- the real rows exact in any order, the
    Hermitian rows (fl(1/sqrt 2) is no short dyadic fraction) within the bound counted from g itself."""
    dtype = "f64"
    eng = make_engine(nr, nc, dtype, "per_chain")
    n = eng.n_chains
    x, width, rows, g = pr.integers_case(n, nr, nc, seed=41)
    kind = {"all": _capi.STEP_ALL, "real": _capi.STEP_REAL_GROUP, "complex": _capi.STEP_COMPLEX_GROUP}[group]
    eng._set(_capi.FIELD_FACTOR, rows)
    got, widths_after = accepted_step(eng, lambda: eng.step_injected(g[None], np.full((1, n), 0.5), kind=kind), x, width)
    check_rest(got, widths_after, x, width, nr, nc, group, "injected")
    c = LD(pr.INV_SQRT2[dtype])
    w_r, w_c = pr.widths_used(width, nr, nc)
    s, a = pr.proposal_reference(x, w_r, w_c, rows, g[:, :nr], g[:, nr:nr + nc].astype(LD) * c, g[:, nr + nc:].astype(LD) * c, nr, nc, group)
    assert np.array_equal(got[:, :nr].astype(LD), s[:, :nr])
    if group != "complex":
        assert np.any(got[:, :nr] != x[:, :nr])
    r = pr.ratio(got, s, a, pr.k_proposal("registers", nr, nc, raw_normals=True), dtype)
    report("injected", nr, nc, dtype, "integers", r, group)
    assert np.all(r <= 1), float(r.max())
    eng.close()


# ------------------------------------------------------------------------------------------------------ magnitude-phase
def magphase_inputs(n, nr, nc, dtype, theta=None):
    """(x, width, K_jj [n, nc], covariance rows): magnitudes in [1/2, 2] with either sign along the direction theta_j (a
    random direction per chain and parameter where theta is None), |z_0| = 0 in every ninth chain; another K_jj per
    chain and parameter at cdiag of the covariance field, decoys in every other slot of the Hermitian block."""
    rng = np.random.default_rng([61, nr, nc])
    mag = rng.uniform(0.5, 2.0, (n, nc)) * rng.choice([-1.0, 1.0], (n, nc))
    mag[::9, 0] = 0.0
    angle = rng.uniform(-np.pi, np.pi, (n, nc)) if theta is None else np.tile(theta, (n, 1))
    x = np.concatenate((rng.standard_normal((n, nr)), mag * np.cos(angle), mag * np.sin(angle)), axis=1)
    width = 2.0 ** rng.uniform(-2, 0, (n, pr.n_width_rows(nr, nc)))
    kdiag = rng.uniform(0.5, 2.0, (n, nc))
    prr = nr * (nr + 1) // 2
    cov = pr.packed_identity(n, nr, nc)
    cov[:, prr:] = 5.0 + rng.uniform(0, 1, (n, nc * nc))
    x, width, kdiag, cov = (pr.to_dtype(v, dtype) for v in (x, width, kdiag, cov))
    cov[:, [pr.cdiag(prr, j) for j in range(nc)]] = kdiag
    return x, width, kdiag, cov


def magphase_step(eng, x, width, cov, g, phases):
    """One magnitude-phase step in which the magnitude stage accepts: float64 with injected draws (g, the phases as
    uniforms), float32 on the engine's own Philox stream.  Returns (x', widths after, accepted)."""
    n, nc = eng.n_chains, eng.num_complex_params
    set_step(eng, 0)
    eng._set(_capi.FIELD_COV, cov)
    eng._set(_capi.FIELD_PARAMS, x)
    eng._set(_capi.FIELD_ENERGY, np.full((n, 1), BIG[eng.dtype]))
    eng._set(_capi.FIELD_WIDTH, width)
    if eng.dtype == "f64":
        uniforms = np.column_stack((np.full(n, 0.5), phases, np.full(n, 0.5)))
        eng.step_injected(g[None], uniforms[None], kind=_capi.STEP_COMPLEX_MAGNITUDE_PHASE)
    else:
        eng.step_complex_group()
    accepted, proposed = eng.accept_stats()
    assert proposed == 2 * n
    eng.sync()
    return eng._get(_capi.FIELD_PARAMS), eng._get(_capi.FIELD_WIDTH), accepted


@pytest.mark.parametrize("dtype", BOTH)
def test_magnitude_stage_keeps_the_direction(dtype):
    """(2,2): z' = (|z| + (w^2 K_jj) g) z / |z| part by part, w the complex group's width row, K_jj at cdiag of the chain's
    covariance field.  The state is read after the MAGNITUDE stage: the engine runs at T = 0 with a dense energy whose 2 x 2
    block of parameter j has its smaller eigenvalue along the direction theta_j every chain holds z_j in, so the magnitude
    stage goes downhill from the huge ledger and every redrawn phase goes uphill and is rejected (a wall on |x_0| cannot
    tell the stages apart: the real parameters rest in both).  theta_0 = 0, so that the chains with |z_0| = 0 propose the
    direction (1, 0) along the valley as well.  Normals: injected in float64; in float32 the stream's normals 0 and 1, which
    the identity-shape engine of the same space leaves in its two real coordinates."""
    nr, nc = 2, 2
    theta, lo, hi = np.array([0.0, 0.7]), 1.0, 3.0
    a = np.diag([1.0, 1.0, 0, 0, 0, 0])
    for j, (c, s) in enumerate(zip(np.cos(theta), np.sin(theta))):
        a[2 + j, 2 + j], a[4 + j, 4 + j] = lo * c * c + hi * s * s, lo * s * s + hi * c * c
        a[2 + j, 4 + j] = a[4 + j, 2 + j] = (lo - hi) * c * s
    eng = make_engine(nr, nc, dtype, "per_chain", energy=me.DenseQuadratic(a), temp=0.0, complex_sample_method="magnitude-phase")
    n = eng.n_chains
    x, width, kdiag, cov = magphase_inputs(n, nr, nc, dtype, theta)
    rng = np.random.default_rng(62)
    g = rng.standard_normal((n, nc)) if dtype == "f64" else identity_state(nr, nc, dtype, n)[:, :nc] / W0
    got, widths_after, accepted = magphase_step(eng, x, width, cov, g, rng.uniform(0.05, 0.95, (n, nc)))
    assert accepted == n                                           # the magnitude stage of every chain, no phase stage
    assert np.array_equal(got[:, :nr], x[:, :nr]) and np.array_equal(widths_after[:, :2], width[:, :2])
    assert not np.array_equal(widths_after[:, 2], width[:, 2])
    s, amp, direction = pr.magphase_reference(x, width[:, 2], kdiag, g, nr, nc)
    r = pr.ratio(got[:, nr:], np.tile(s, 2) * direction, np.tile(amp, 2) * np.abs(direction), pr.K_MAGPHASE, dtype)
    print("\nPROPOSAL_GPU path=magphase (2,2) dtype=%s class=magnitude ratio=%.3f" % (dtype, float(r.max())))
    assert np.all(r <= 1), (float(r.max()), np.argwhere(r > 1)[:4].tolist())
    assert np.all(got[::9, nr] != 0) and not got[::9, nr + nc].any()       # |z_0| = 0: the direction (1, 0)
    wrong = pr.magphase_reference(x, width[:, 0], kdiag, g, nr, nc)         # sharp: the shared width row does not pass
    assert pr.ratio(got[:, nr:], np.tile(wrong[0], 2) * direction, np.tile(wrong[1], 2) * np.abs(direction), pr.K_MAGPHASE, dtype).max() > 1
    eng.close()


def test_magnitude_stage_without_real_parameters():
    """(0,3), float64, injected: no real parameter and no dense energy in this kernel set, so the phase stage cannot be
    made to reject; it is given the phase 0 (u = 1/2) and accepts, leaving (|z'|, 0) -- the magnitude within
    K_MAGPHASE_AFTER_PHASE.  (Float32 has no injected form, and its own phases would bring v_sin / v_cos into a bound
    that has no derivation for them: float32 is held at (2,2).)"""
    nr, nc, dtype = 0, 3, "f64"
    eng = make_engine(nr, nc, dtype, "per_chain", complex_sample_method="magnitude-phase")
    n = eng.n_chains
    x, width, kdiag, cov = magphase_inputs(n, nr, nc, dtype)
    g = np.random.default_rng(63).standard_normal((n, nc))
    got, _, accepted = magphase_step(eng, x, width, cov, g, np.full((n, nc), 0.5))
    assert accepted == 2 * n
    s, amp, _ = pr.magphase_reference(x, width[:, 0], kdiag, g, nr, nc)
    r = pr.ratio(got[:, :nc], np.abs(s), amp, pr.K_MAGPHASE_AFTER_PHASE, dtype)
    print("\nPROPOSAL_GPU path=magphase (0,3) dtype=%s class=magnitude ratio=%.3f" % (dtype, float(r.max())))
    assert np.all(r <= 1), float(r.max())
    assert not got[:, nc:].any()
    eng.close()


# ------------------------------------------------------------------------------------------------------ the energies
def energy_spec(kind, nr, nc, cf):
    if kind == "iso":
        return me.IsoQuadratic(cf[0])
    if kind == "diag":
        return me.DiagQuadratic(cf[:nr], cf[nr:nr + nc])
    if kind in ("landau", "landau_terms"):
        return me.LandauToy(*cf, terms=kind == "landau_terms")
    return me.CylinderSurrogate(*cf)


def report_energy(path, kind, nr, nc, dtype, name, what, r):
    print("\nENERGY_GPU path=%s kind=%s (%d,%d) dtype=%s class=%s %s=%.3f" % (path, kind, nr, nc, dtype, name, what, float(np.max(r))))


def check_energy(kind, nr, nc, dtype, path, mode="identity", runtime=False, groups=("all",)):
    classes = pr.ENERGY_CLASSES if kind in ("landau", "landau_terms") else pr.ENERGY_CLASSES[:2]
    n = n_chains_for(nr, nc)
    k = pr.k_energy(kind, nr, nc, runtime)
    for name in classes:
        x, cf = pr.energy_case(kind, name, n, nr, nc, dtype, seed=51)
        eng = make_engine(nr, nc, dtype, mode, energy=energy_spec(kind, nr, nc, cf))
        terms = len(eng.energy_term_names)
        if mode == "per_chain":
            eng._set(_capi.FIELD_FACTOR, pr.packed_identity(n, nr, nc) * 2.0)
        width = np.full((n, pr.n_width_rows(nr, nc)), TINY_WIDTH[dtype])
        for group in groups:
            ledger = np.full((n, terms), BIG[dtype])
            marker = pr.to_dtype(12345.678 + np.arange(n), dtype)
            if kind == "landau_terms" and group == "complex":
                ledger[:, 1] = marker                            # row "area": the complex group cannot change it
            x1, _ = accepted_step(eng, getattr(eng, STEPS[group]), x, width, ledger)
            assert np.array_equal(x1[x != 0], x[x != 0])
            e = eng._get(_capi.FIELD_ENERGY)
            s, a = pr.energy_reference(kind, x1, nr, nc, cf)
            s, a = s.reshape(n, -1), a.reshape(n, -1)
            rows = [0] if kind == "landau_terms" and group == "complex" else range(terms)
            if kind == "landau_terms" and group == "complex":
                assert np.array_equal(e[:, 1], marker)
            if name == "integers":
                assert np.array_equal(e[:, rows].astype(LD), s[:, rows]), (kind, group)
            else:
                r = pr.ratio(e, s, a, k, dtype)[:, rows]
                report_energy(path, kind, nr, nc, dtype, name, "step_" + group, r)
                assert np.all(r <= 1), (kind, name, group, float(r.max()))
        # initialize_energy_dict() at the same state
        eng.initialize_energy_dict()
        eng.sync()
        again = eng._get(_capi.FIELD_ENERGY)
        if name == "integers":
            assert np.array_equal(again.astype(LD), s)
        else:
            r = pr.ratio(again, s, a, k, dtype)
            report_energy(path, kind, nr, nc, dtype, name, "init", r)
            assert np.all(r <= 1), (kind, name, "init", float(r.max()))
        if groups[-1] == "all":
            print("ENERGY_GPU path=%s kind=%s (%d,%d) dtype=%s class=%s init is %s the in-step value"
                  % (path, kind, nr, nc, dtype, name, "bitwise" if np.array_equal(again, e) else "NOT bitwise"))
        eng.close()


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kind", ["iso", "diag"])
@pytest.mark.parametrize("nr,nc", [(16, 0), (3, 0), (2, 1), (4, 4), (33, 0)], ids=lambda v: str(v))
def test_quadratic_energy_functors(nr, nc, kind, dtype):
    check_energy(kind, nr, nc, dtype, "functor", groups=("real", "complex", "all") if nr and nc else ("all",))


@pytest.mark.parametrize("dtype", BOTH)
def test_energy_functor_in_the_streamed_factor_body(dtype):
    check_energy("diag", 33, 0, dtype, "streamed", mode="per_chain")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kind", ["iso", "diag"])
@pytest.mark.parametrize("nr,nc", [(130, 0), (101, 0), (60, 25)], ids=lambda v: str(v))
def test_runtime_dimension_energy_loops(nr, nc, kind, dtype):
    check_energy(kind, nr, nc, dtype, "runtime", runtime=True, groups=("real", "complex", "all") if nc else ("all",))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kind", ["iso", "diag"])
def test_runtime_dimension_energy_loop_with_per_chain_factors(kind, dtype):
    check_energy(kind, 140, 0, dtype, "runtime-lds", mode="per_chain", runtime=True)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kind", ["landau", "landau_terms"])
def test_landau_energies(kind, dtype):
    """Both ledger rows of the term form within their bounds; a complex-group step rewrites row "field" only (row "area"
    comes back bitwise), a real-group step and step_all both."""
    check_energy(kind, 2, 1, dtype, "functor", groups=("complex", "real", "all"))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("nr,nc", [(1, 2), (2, 2)], ids=lambda v: str(v))
def test_cylinder_energy(nr, nc, dtype):
    check_energy("cylinder", nr, nc, dtype, "functor")
