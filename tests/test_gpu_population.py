"""Population annealing on the GPU (me_set_temperature, me_population_resample and friends).

One stage is ``tests/population_reference.py``; a resampled-and-stepped engine follows a ``ManyChainOracle`` driven by
that reference at 1e-9 (float64), as in test_gpu_replica_exchange.py."""
import importlib.util
import os

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi
from oracle import energies
from oracle.manychain import ManyChainOracle
from population_reference import (PopulationReference, ambiguous_slots, ancestors, ledger_energy, stage_uniform,
                                  stage_weights)

pytestmark = pytest.mark.gpu
TOL = 1e-9
SEED, OFFSET = 2026, (1 << 33) + 17
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
KEPT = (_capi.FIELD_WIDTH, _capi.FIELD_MEAN, _capi.FIELD_OBS_MEAN, _capi.FIELD_COV, _capi.FIELD_FACTOR)


def _fields(eng, fields):
    out = {}
    for f in fields:
        try:
            out[f] = eng._get(f)
        except NotImplementedError:
            pass
    return out


def _exact_stage(eng, t_new, seed, offset, energy_scale=4.0, data_seed=0):
    """Random x and ledger on a fresh engine (every family still its founder), one stage, and the comparison with the
    reference: ancestors away from rounding-close boundaries, the moved fields bit for bit, the kept fields untouched."""
    rng = np.random.default_rng(data_seed)
    n = eng.n_chains
    d = eng._get(_capi.FIELD_PARAMS, 0, 1).shape[1]
    n_terms = eng._get(_capi.FIELD_ENERGY, 0, 1).shape[1]
    eng._set(_capi.FIELD_PARAMS, rng.standard_normal((n, d)))
    ledger = rng.gamma(2.0, energy_scale / n_terms, (n, n_terms)) - rng.uniform(0, 1, (n, n_terms))
    eng._set(_capi.FIELD_ENERGY, ledger)
    x0, e0 = eng._get(_capi.FIELD_PARAMS), eng._get(_capi.FIELD_ENERGY)
    kept0 = _fields(eng, KEPT)
    fam0 = eng.families()
    assert np.array_equal(fam0, offset + np.arange(n))
    t_old = eng.temp
    eng.resample(t_new)
    assert eng.temp == t_new
    w = stage_weights(ledger_energy(e0, eng.dtype), t_old, t_new)
    u = stage_uniform(seed, offset, 0)
    want = ancestors(w, u)
    amb = ambiguous_slots(w, u)
    # (a window of 1e-9 N around N boundaries holds ~2e-9 N^2 slots: the populations here stay below 2^14 chains)
    assert amb.sum() <= max(1.0, 1e-4 * n), amb.sum()
    fam = eng.families()
    anc = fam - offset
    assert np.all(np.diff(fam) >= 0) and np.all((anc >= 0) & (anc < n))
    assert np.array_equal(anc[~amb], want[~amb]), np.flatnonzero((anc != want) & ~amb)[:10]
    assert np.array_equal(eng._get(_capi.FIELD_PARAMS), x0[anc])
    assert np.array_equal(eng._get(_capi.FIELD_ENERGY), e0[anc])
    for f, v in _fields(eng, KEPT).items():
        assert np.array_equal(v, kept0[f]), f
    st = eng.population_stats()
    assert st["stages"] == 1 and st["temps"].tolist() == [t_new] and st["n_finite"].tolist() == [n]
    assert np.isclose(st["log_weight"][0], w["log_weight"], rtol=1e-12, atol=0)
    assert np.isclose(st["neff_fraction"][0], w["neff_fraction"], rtol=1e-12, atol=0)
    assert eng.n_families() == len(np.unique(anc))
    return w


# ---------------------------------------------------------------------------------------------------- 1. mechanics
# name -> (spec, real0, cplx0, dtype); D < 16: component-major state, D >= 16: tile-major
CASES = {
    "real_4_f64": (me.DiagQuadratic((1, 2, 4, 8)), [0.1] * 4, None, "f64"),
    "mixed_2_2_f32": (me.DiagQuadratic((1, 3), (2, 0.5)), [0.2, -0.1], [0.1j, 0.2], "f32"),
    "mixed_2_2_f64": (me.DiagQuadratic((1, 3), (2, 0.5)), [0.2, -0.1], [0.1j, 0.2], "f64"),
    "iso_16_f64": (me.IsoQuadratic(1.0), [0.0] * 16, None, "f64"),
    "iso_16_f32": (me.IsoQuadratic(1.0), [0.0] * 16, None, "f32"),
    "landau_terms_f64": (me.LandauToy(1.0, -1.0, 0.5, terms=True), [0.0, 0.0], [0j], "f64"),
    "landau_terms_f32": (me.LandauToy(1.0, -1.0, 0.5, terms=True), [0.0, 0.0], [0j], "f32"),
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [5000, 6 * 2048 + 64])
def test_one_stage_follows_the_reference(name, n):
    spec, real0, cplx0, dtype = CASES[name]
    eng = me.MetropolisEngine(spec, None, real0, cplx0, n_chains=n, seed=SEED, dtype=dtype, chain_offset=OFFSET, temp=1.0)
    for _ in range(3):
        eng.step_all(2)
        eng.measure()
    w = _exact_stage(eng, 0.6, SEED, OFFSET)
    assert 0.05 < w["neff_fraction"] < 0.95            # the stage did reweight
    if name.startswith("landau"):
        assert eng._get(_capi.FIELD_ENERGY).shape[1] > 1


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_collapsed_weights_follow_the_reference(dtype):
    # a steep step: a few chains own runs of tens to thousands of slots (written by whole wavefronts), then all of them
    n = 6 * 2048 + 64
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=n, seed=SEED, dtype=dtype,
                              chain_offset=OFFSET, temp=1.0)
    w = _exact_stage(eng, 0.05, SEED, OFFSET)
    counts = np.bincount(eng.families() - OFFSET, minlength=n)
    assert w["neff_fraction"] < 0.01 and counts.max() > 64
    one = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=n, seed=SEED, dtype=dtype, temp=1.0)
    e = np.random.default_rng(5).gamma(2.0, 1.0, (n, 1))
    e[777, 0] = -100.0
    one._set(_capi.FIELD_ENERGY, e)
    x0 = one._get(_capi.FIELD_PARAMS)
    one.resample(0.5)
    assert np.array_equal(one.families(), np.full(n, 777)) and one.n_families() == 1
    assert np.array_equal(one._get(_capi.FIELD_PARAMS), np.repeat(x0[777:778], n, axis=0))
    assert np.all(one._get(_capi.FIELD_ENERGY) == e[777, 0])


def test_non_finite_energies_get_no_offspring():
    n = 4096
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=n, seed=3, dtype="f64", temp=1.0)
    e = np.random.default_rng(1).gamma(2.0, 1.0, (n, 1))
    bad = np.zeros(n, dtype=bool)
    bad[::7] = True
    e[bad, 0] = np.where(np.arange(bad.sum()) % 2, np.inf, np.nan)
    eng._set(_capi.FIELD_ENERGY, e)
    eng.resample(0.5)
    anc = eng.families()
    assert not np.isin(np.flatnonzero(bad), anc).any()
    assert eng.population_stats()["n_finite"][0] == n - bad.sum()
    # nothing finite: the population stays, the stage records -inf
    eng._set(_capi.FIELD_ENERGY, np.full((n, 1), np.nan))
    fam, x = eng.families(), eng._get(_capi.FIELD_PARAMS)
    eng.resample(0.4)
    st = eng.population_stats()
    assert st["log_weight"][1] == -np.inf and st["neff_fraction"][1] == 0.0 and st["n_finite"][1] == 0
    assert np.array_equal(eng.families(), fam) and np.array_equal(eng._get(_capi.FIELD_PARAMS), x)
    assert eng.temp == 0.4


# ---------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("name", ["mixed_2_2_f32", "iso_16_f64", "landau_terms_f64"])
def test_resampling_at_the_same_temperature_is_the_identity(name):
    spec, real0, cplx0, dtype = CASES[name]
    eng = me.MetropolisEngine(spec, None, real0, cplx0, n_chains=5000, seed=4, dtype=dtype, temp=0.8)
    for _ in range(60):
        eng.step_all(2)
        eng.measure()
    fields = (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY) + KEPT
    before = _fields(eng, fields)
    eng.resample(0.8)
    after = _fields(eng, fields)
    for f in before:
        assert np.array_equal(before[f], after[f]), f
    st = eng.population_stats()
    assert st["log_weight"][0] == 0.0 and st["neff_fraction"][0] == 1.0
    assert np.array_equal(eng.families(), np.arange(5000)) and eng.n_families() == 5000


# ---------------------------------------------------------------------------------------------------- 3. oracle parity
def test_annealing_follows_the_oracle():
    n, t0 = 256, 1.0
    spec, oen = me.DiagQuadratic((1, 2), (3,)), energies.diag_quadratic(2, 1, (1, 2), (3,))
    eng = me.MetropolisEngine(spec, None, [0.2, 0.1], [0.1j], n_chains=n, seed=SEED, dtype="f64", chain_offset=OFFSET,
                              temp=t0)
    o = ManyChainOracle(2, 1, oen, n, seed=SEED, temp=t0, initial_real_params=[0.2, 0.1], initial_complex_params=[0.1j],
                        chain_offset=OFFSET)
    ref = PopulationReference(o, SEED, OFFSET)
    eng.step_all(10)
    o.step(10)
    temps = t0 * 0.3 ** (np.arange(1, 21) / 20)
    for k, t in enumerate(temps):
        eng.resample(t)
        ref.resample(t)
        eng.step_all(5)
        o.step(5)
        if k % 5 == 4:
            assert np.array_equal(eng.families(), ref.families)
            assert np.allclose(eng._get(_capi.FIELD_PARAMS), o.x, rtol=0, atol=TOL)
            assert np.allclose(eng.energy_total, o.energy, rtol=0, atol=TOL)
            assert np.allclose(eng._get(_capi.FIELD_WIDTH)[:, 0], o.width_all, rtol=0, atol=TOL)
    st = eng.population_stats()
    assert st["stages"] == 20 and np.array_equal(st["temps"], temps)
    assert np.allclose(st["log_weight"], ref.log_weight, rtol=1e-12, atol=1e-15)
    assert np.allclose(st["neff_fraction"], ref.neff_fraction, rtol=1e-12, atol=0)
    assert st["n_finite"].tolist() == ref.n_finite
    assert np.allclose(st["log_z"], np.cumsum(ref.log_weight), rtol=1e-12, atol=1e-14)
    assert eng.accept_stats() == (o.accepted, o.proposed)
    assert 1 < eng.n_families() < n


# ---------------------------------------------------------------------------------------------------- 4. free energy
def _anneal_quadratic(spec, real0, cplx0, coef, seed, n=1 << 18, t_hot=10.0, t_cold=0.1, stages=40, sweeps=10):
    """Start from the exact Boltzmann law at t_hot (x_k ~ N(0, T / 2 coef_k)), then anneal geometrically to t_cold.  The
    proposal width starts at 2.4 sigma / sqrt(D) and follows sqrt(T) from stage to stage, as the Boltzmann width of a
    quadratic energy does (the width adaptation alone, at its damping of 1/200 per step, lags a hundredfold cooling by
    far: with a fixed start of 1.0 the 16-dimensional population froze and log_z came out 1-2 too low)."""
    coef = np.asarray(coef, dtype=np.float64)
    width = 2.4 * np.sqrt(t_hot / (2 * np.median(coef))) / np.sqrt(coef.size)
    eng = me.MetropolisEngine(spec, None, real0, cplx0, width, n_chains=n, seed=seed, dtype="f64", temp=t_hot)
    x = np.random.default_rng(seed).standard_normal((n, coef.size)) * np.sqrt(t_hot / (2 * coef))
    eng._set(_capi.FIELD_PARAMS, x)
    eng.initialize_energy_dict()
    eng.step_all(50)
    t_prev = t_hot
    for t in t_hot * (t_cold / t_hot) ** (np.arange(1, stages + 1) / stages):
        eng.resample(t)
        eng._set(_capi.FIELD_WIDTH, eng._get(_capi.FIELD_WIDTH) * np.sqrt(t / t_prev))
        eng.step_all(sweeps)
        t_prev = t
    return eng


# log_z - exact measured on the MI355X over seeds 1..4 with this protocol: IsoQuadratic D = 16: -0.033, -0.020, -0.025,
# -0.028 (std 0.005); DiagQuadratic 2 + 2: -0.016, -0.015, -0.012, -0.011 (std 0.002).  The estimate sits slightly low
# (a finite population's ln of a mean weight is biased low); 0.05 covers that bias plus more than 5x the spread.
LOG_Z_TOL = 0.05


@pytest.mark.parametrize("seed", [1, 2])
def test_free_energy_of_the_isotropic_quadratic(seed):
    """ln Z(0.1) / Z(10) of E = |x|^2 over D = 16 real coordinates is (D / 2) ln(0.01) = -36.841.  Measured (seeds 1-4):
    -36.874, -36.861, -36.866, -36.869; final pooled variance / (T / 2) 1.0006, 0.9997, 1.0026, 1.0003."""
    d = 16
    eng = _anneal_quadratic(me.IsoQuadratic(1.0), [0.0] * d, None, [1.0] * d, seed)
    st = eng.population_stats()
    exact = d / 2 * np.log(0.01)
    assert abs(st["log_z"][-1] - exact) < LOG_Z_TOL, (st["log_z"][-1], exact)
    assert eng.temp == pytest.approx(0.1) and np.all(st["n_finite"] == 1 << 18)
    x = eng._get(_capi.FIELD_PARAMS)
    var = x.var(axis=0)
    assert abs(var.mean() / (0.1 / 2) - 1) < 0.01, var.mean()
    assert np.all(np.abs(var / (0.1 / 2) - 1) < 0.03)


def test_free_energy_of_a_mixed_diagonal_quadratic():
    """2 real (a = 1, 2) + 2 complex (b = 3, 0.5) parameters, D_eff = 6: ln Z(0.1) / Z(10) = 3 ln(0.01) = -13.816.
    Measured (seeds 1-4): -13.831, -13.831, -13.828, -13.827."""
    coef = np.array([1, 2, 3, 0.5, 3, 0.5])          # real, real, Re z1, Re z2, Im z1, Im z2
    eng = _anneal_quadratic(me.DiagQuadratic((1, 2), (3, 0.5)), [0.1, 0.1], [0.1j, 0.1], coef, 3)
    st = eng.population_stats()
    exact = 3 * np.log(0.01)
    assert abs(st["log_z"][-1] - exact) < LOG_Z_TOL, (st["log_z"][-1], exact)
    x = eng._get(_capi.FIELD_PARAMS)
    ratio = x.var(axis=0) / (0.1 / (2 * coef))
    assert abs(ratio.mean() - 1) < 0.01 and np.all(np.abs(ratio - 1) < 0.03), ratio


# ---------------------------------------------------------------------------------------------------- 5. double well
def _demo():
    spec = importlib.util.spec_from_file_location("demo_population_annealing",
                                                  os.path.join(EXAMPLES, "demo_population_annealing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_double_well_annealing_populates_both_wells(capsys):
    demo = _demo()
    assert demo.T_HOT == 4.0 and demo.T_COLD == 0.1 and demo.SCHEDULE[-1] == pytest.approx(0.1)
    annealed, cold = demo.main()
    assert abs(demo.right_well_fraction(annealed) - 0.5) < 0.02
    assert demo.right_well_fraction(cold) < 0.01        # local moves alone never leave the starting well
    st = annealed.population_stats()
    assert abs(st["log_z"][-1] - demo.log_z_quadrature(demo.T_HOT, demo.T_COLD)) < 0.05
    assert "quadrature" in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- 6. reproducibility
def test_same_seed_is_bitwise_reproducible_and_offsets_draw_their_own_uniform():
    def run(offset):
        eng = me.MetropolisEngine(me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j], n_chains=1 << 14, seed=5,
                                  dtype="f32", chain_offset=offset, temp=2.0)
        eng.step_all(20)
        eng.anneal(2.0 * 0.5 ** (np.arange(1, 9) / 8), n_sweeps=3)
        return eng
    a, b = run(0), run(0)
    for f in (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY, _capi.FIELD_WIDTH):
        assert np.array_equal(a._get(f), b._get(f))
    assert np.array_equal(a.families(), b.families())
    sa, sb = a.population_stats(), b.population_stats()
    for key in ("log_weight", "neff_fraction", "n_finite", "temps"):
        assert np.array_equal(sa[key], sb[key]), key
    # the same population at another chain_offset: another uniform, other ancestors, each as the reference says
    assert stage_uniform(5, 0, 0) != stage_uniform(5, 1 << 20, 0)
    ancs = []
    for offset in (0, 1 << 20):
        eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=4096, seed=5, dtype="f64",
                                  chain_offset=offset, temp=1.0)
        _exact_stage(eng, 0.5, 5, offset, data_seed=3)
        ancs.append(eng.families() - offset)
    assert not np.array_equal(ancs[0], ancs[1])


# ---------------------------------------------------------------------------------------------------- 7. checkpoint
def test_checkpoint_continues_bitwise():
    kw = dict(n_chains=4096, seed=8, dtype="f64", temp=2.0)
    args = (me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j])
    temps = 2.0 * 0.1 ** (np.arange(1, 21) / 20)

    def drive(e, ts):
        for t in ts:
            e.resample(t)
            e.step_all(3)
            e.measure()

    assert not {"temp", "families", "population_log_weight"} & set(me.MetropolisEngine(*args, **kw).state_dict())
    whole = me.MetropolisEngine(*args, **kw)
    part = me.MetropolisEngine(*args, **kw)
    drive(whole, temps)
    drive(part, temps[:10])
    state = part.state_dict()
    assert state["temp"] == temps[9] and state["population_log_weight"].shape == (10,)
    assert state["families"].shape == (4096,)
    resumed = me.MetropolisEngine(*args, **kw)
    with pytest.raises(ValueError):
        resumed.load_state_dict(dict(state, families=state["families"][:10]))
    assert resumed.population_stats()["stages"] == 0          # refused before anything was written
    resumed.load_state_dict(state)
    assert resumed.temp == temps[9]
    drive(resumed, temps[10:])
    for f in (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY, _capi.FIELD_WIDTH, _capi.FIELD_MEAN, _capi.FIELD_COV,
              _capi.FIELD_FACTOR, _capi.FIELD_OBS_MEAN):
        assert np.array_equal(whole._get(f), resumed._get(f)), f
    assert np.array_equal(whole.families(), resumed.families())
    sw, sr = whole.population_stats(), resumed.population_stats()
    for key in ("temps", "log_weight", "neff_fraction", "n_finite", "log_z"):
        assert np.array_equal(sw[key], sr[key]), key
    assert whole.accept_stats() == resumed.accept_stats()


def test_a_checkpoint_from_before_the_first_stage_resets_the_population():
    kw = dict(n_chains=1024, seed=9, dtype="f64", temp=2.0)
    args = (me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j])
    fresh = me.MetropolisEngine(*args, **kw)
    fresh.step_all(5)
    old = fresh.state_dict()
    assert "temp" not in old
    eng = me.MetropolisEngine(*args, **kw)
    eng.anneal([1.5, 1.0, 0.5], n_sweeps=2)
    assert eng.n_families() < 1024
    eng.load_state_dict(old)
    assert eng.temp == 2.0 and eng.population_stats()["stages"] == 0
    assert np.array_equal(eng.families(), np.arange(1024)) and eng.n_families() == 1024
    assert not {"temp", "families", "population_log_weight"} & set(eng.state_dict())
    # ... and it continues exactly as the engine the checkpoint came from
    fresh.step_all(5)
    eng.step_all(5)
    for f in (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY, _capi.FIELD_WIDTH):
        assert np.array_equal(fresh._get(f), eng._get(f)), f
    eng.resample(1.0)                              # the stage count starts over: stage 0's uniform again
    fresh.resample(1.0)
    assert np.array_equal(fresh.families(), eng.families())


# ---------------------------------------------------------------------------------------------------- 8. other kernel sets
def test_dense_64_matrix_core_engine():
    q = np.random.default_rng(2).standard_normal((64, 64))
    eng = me.MetropolisEngine(me.DenseQuadratic(q @ q.T / 64 + np.identity(64)), None, [0.0] * 64, None, n_chains=4096,
                              cov_mode="fixed", seed=6, temp=1.0)
    eng.step_all(4)
    _exact_stage(eng, 0.5, 6, 0)


def test_runtime_dimension_engine():
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 140, None, n_chains=1 << 12, cov_mode="fixed", seed=7,
                              temp=1.0)
    eng.step_all(4)
    _exact_stage(eng, 0.5, 7, 0)
    eng.step_all(4)                                  # and it keeps stepping at the new temperature
    assert np.all(np.isfinite(eng.energy_total))


# ---------------------------------------------------------------------------------------------------- 9. refusals, set_temp
def test_refusals():
    ladder = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=128, temperatures=[1.0, 2.0])
    with pytest.raises(ValueError, match="ladder"):
        ladder.resample(0.5)
    with pytest.raises(ValueError, match="ladder"):
        ladder.set_temp(0.5)
    assert ladder._lib.me_population_resample(ladder._handle, 0.5) == _capi.ME_ERR_STATE
    assert ladder._lib.me_set_temperature(ladder._handle, 0.5) == _capi.ME_ERR_STATE
    cold = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=128)
    with pytest.raises(ValueError, match="temp = 0"):
        cold.resample(0.5)
    assert cold._lib.me_population_resample(cold._handle, 0.5) == _capi.ME_ERR_STATE
    ledgers = me.MetropolisEngine(me.LandauToy(), None, [0.0, 0.0], [0j], n_chains=128, reference_energy_ledgers=True,
                                  temp=1.0)
    with pytest.raises(NotImplementedError, match="LEDGERS"):
        ledgers.resample(0.5)
    warm = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=128, temp=1.0)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            warm.resample(bad)
        assert warm._lib.me_population_resample(warm._handle, bad) == _capi.ME_ERR_INVALID
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            warm.set_temp(bad)
        assert warm._lib.me_set_temperature(warm._handle, bad) == _capi.ME_ERR_INVALID
    assert warm.population_stats()["stages"] == 0 and warm.temp == 1.0
    with pytest.raises(ValueError):
        warm.set_temperatures([1.0, 2.0])       # a scalar-temp engine cannot take a ladder (as before)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_set_temp_then_step_equals_an_engine_built_at_that_temperature(dtype):
    kw = dict(n_chains=1024, seed=12, dtype=dtype)
    args = (me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j])
    built = me.MetropolisEngine(*args, temp=0.35, **kw)
    changed = me.MetropolisEngine(*args, temp=3.0, **kw)
    changed.set_temp(0.35)
    assert changed.temp == 0.35
    for _ in range(60):
        for e in (built, changed):
            e.step_all(2)
            e.step_real_group()
            e.measure()
    for f in (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY, _capi.FIELD_WIDTH, _capi.FIELD_MEAN, _capi.FIELD_COV):
        assert np.array_equal(built._get(f), changed._get(f)), f
    assert built.accept_stats() == changed.accept_stats()
    # simulated annealing from temp = 0 upwards works too, and the checkpoint now carries temp
    zero = me.MetropolisEngine(*args, **kw)
    zero.set_temp(0.5)
    zero.step_all(5)
    assert zero.state_dict()["temp"] == 0.5
