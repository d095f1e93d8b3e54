"""Temperature ladders and replica exchange on the GPU (me_set_temperature_ladder, me_replica_exchange).

Rung k of a ladder engine (K rungs of M chains) is ``ManyChainOracle(temp=T_k, chain_offset=offset + k*M, n_chains=M)``;
swaps are ``tests/replica_reference.py``.  float64 checks at 1e-9 as in test_gpu_parity.py."""
import importlib.util
import os

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi
from oracle import energies
from oracle.manychain import ManyChainOracle
from replica_reference import ReplicaReference

pytestmark = pytest.mark.gpu
TOL = 1e-9
SEED, OFFSET = 2026, (1 << 33) + 17
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")

# name -> (nr, nc, product spec, oracle energy, real0, cplx0, ladder)
CASES = {
    "real_4": (4, 0, me.DiagQuadratic((1, 2, 4, 8)), energies.diag_quadratic(4, 0, (1, 2, 4, 8)), [0.1, 0.2, -0.1, 0.0],
               None, [0.3, 0.5, 0.8, 1.3]),
    "mixed_2_2": (2, 2, me.DiagQuadratic((1, 3), (2, 0.5)), energies.diag_quadratic(2, 2, (1, 3), (2, 0.5)), [0.2, -0.1],
                  [0.1j, 0.2 - 0.1j], [0.3, 0.5, 0.8, 1.3]),
    "landau_terms": (2, 1, me.LandauToy(1.0, -1.0, 0.5, terms=True), energies.landau_toy(1.0, -1.0, 0.5), [0.0, 0.0], [0j],
                     [0.05, 0.1, 0.2, 0.4]),
}


def _pair(name, m=64, **kw):
    nr, nc, spec, oen, real0, cplx0, temps = CASES[name]
    eng = me.MetropolisEngine(spec, None, real0, cplx0, n_chains=m * len(temps), seed=SEED, dtype="f64",
                              chain_offset=OFFSET, temperatures=temps, **kw)
    oras = [ManyChainOracle(nr, nc, oen, m, seed=SEED, temp=t, initial_real_params=real0, initial_complex_params=cplx0,
                            chain_offset=OFFSET + k * m) for k, t in enumerate(temps)]
    return eng, oras


def _cat(oras, name):
    return np.concatenate([getattr(o, name) for o in oras], axis=0)


def _assert_follows(eng, oras, full=True):
    nr, nc = eng.num_real_params, eng.num_complex_params
    assert np.allclose(eng._get(_capi.FIELD_PARAMS), _cat(oras, "x"), rtol=0, atol=TOL)
    assert np.allclose(eng.energy_total, _cat(oras, "energy"), rtol=0, atol=TOL)
    w = eng._get(_capi.FIELD_WIDTH)
    if nr and nc:
        want = np.stack([_cat(oras, "width_all"), _cat(oras, "width_real"), _cat(oras, "width_complex")], axis=1)
        assert np.allclose(w, want, rtol=0, atol=TOL)
    else:
        assert np.allclose(w[:, 0], _cat(oras, "width_real" if nr else "width_complex"), rtol=0, atol=TOL)
    if not full:
        return
    assert np.allclose(eng._get(_capi.FIELD_MEAN), _cat(oras, "mean"), rtol=0, atol=TOL)
    assert np.allclose(eng._get(_capi.FIELD_OBS_MEAN), _cat(oras, "observables_mean"), rtol=0, atol=TOL)
    if nr:
        assert np.allclose(eng.covariance_matrix_real, _cat(oras, "cov_real"), rtol=0, atol=TOL)
    if nc:
        assert np.allclose(eng.covariance_matrix_complex, _cat(oras, "cov_complex"), rtol=0, atol=TOL)
    fr, fc = eng.proposal_factors()
    if nr:
        assert np.allclose(fr, _cat(oras, "factor_real"), rtol=0, atol=1e-8)
    if nc:
        assert np.allclose(fc, _cat(oras, "factor_complex"), rtol=0, atol=1e-8)


# ---------------------------------------------------------------------------------------------------- 1. ladder, no swaps
@pytest.mark.parametrize("name, mode", [("real_4", "step"), ("mixed_2_2", "step"), ("mixed_2_2", "groups"),
                                        ("real_4", "cycle"), ("mixed_2_2", "cycle"), ("mixed_2_2", "magphase")])
def test_each_rung_follows_the_oracle_at_its_temperature(name, mode):
    kw = {"complex_sample_method": "magnitude-phase"} if mode == "magphase" else {}
    eng, oras = _pair(name, **kw)
    assert eng.temp == 0 and np.array_equal(eng.temperatures, CASES[name][6])
    assert np.array_equal(eng.chain_temperatures(), np.repeat(CASES[name][6], 64))
    for k in range(60):                            # across the 50-measure threshold: per-chain shapes from measure 51 on
        if mode == "cycle":
            eng.cycle(2)
        elif mode == "groups":
            eng.step_all(1)
            eng.step_real_group(1)
            eng.step_complex_group(1)
        elif mode == "magphase":
            eng.step_all(1)
            eng.step_complex_group(1)
        else:
            eng.step_all(2)
        if mode != "cycle":
            eng.measure()
        for o in oras:
            if mode == "groups":
                o.step(1)
                o.step(1, group="real")
                o.step(1, group="complex")
            elif mode == "magphase":
                o.step(1)
                o.step_magnitude_phase(1)
            else:
                o.step(2)
            o.measure()
        if k % 20 == 19:
            _assert_follows(eng, oras)
    if mode == "cycle":
        assert eng.fused_cycles() == 60
    acc, prop = eng.accept_stats()
    assert (acc, prop) == (sum(o.accepted for o in oras), sum(o.proposed for o in oras))


# ---------------------------------------------------------------------------------------------------- 2. swaps
@pytest.mark.parametrize("name", sorted(CASES))
def test_swaps_follow_the_reference(name):
    eng, oras = _pair(name)
    ref = ReplicaReference(oras, CASES[name][6], SEED)
    for k in range(60):
        eng.step_all(3)
        eng.replica_exchange()
        eng.measure()
        for o in oras:
            o.step(3)
        ref.exchange()
        for o in oras:
            o.measure()
        if k % 20 == 19:
            _assert_follows(eng, oras)
            rnd, att, acc = eng.swap_stats()
            assert rnd == ref.round and att.tolist() == ref.attempted.tolist() and acc.tolist() == ref.accepted.tolist()
    assert np.all(ref.accepted > 0)                # the swaps did happen
    eng.replica_exchange(3)
    ref.exchange(3)
    _assert_follows(eng, oras, full=False)
    assert eng.swap_stats()[0] == ref.round == 63


# ---------------------------------------------------------------------------------------------------- 3. one rung
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_one_rung_is_the_scalar_temperature_bitwise(dtype):
    kw = dict(n_chains=256, seed=4, dtype=dtype)
    a = me.MetropolisEngine(me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j], temp=0.7, **kw)
    b = me.MetropolisEngine(me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j], temperatures=[0.7], **kw)
    for _ in range(60):
        for e in (a, b):
            e.step_all(2)
            e.step_real_group()
            e.measure()
    b.replica_exchange(2)                          # one rung has no pair: nothing moves
    for field in (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY, _capi.FIELD_WIDTH, _capi.FIELD_MEAN, _capi.FIELD_COV,
                  _capi.FIELD_FACTOR):
        assert np.array_equal(a._get(field), b._get(field)), field
    assert a.accept_stats() == b.accept_stats()
    assert b.swap_stats()[0] == 2 and b.swap_stats()[1].shape == (0,)


# ---------------------------------------------------------------------------------------------------- 4. physics
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_iso_quadratic_ladder_variances_and_swap_acceptance(dtype):
    d, a, k_rungs, n = 16, 1.0, 8, 1 << 16
    temps = 0.5 * 1.25 ** np.arange(k_rungs)
    m = n // k_rungs
    eng = me.MetropolisEngine(me.IsoQuadratic(a), None, [0.0] * d, None, n_chains=n, seed=31, dtype=dtype,
                              temperatures=temps)
    for _ in range(300):                           # burn-in with swaps (the widths adapt on the way)
        eng.step_all(10)
        eng.replica_exchange()
    mom = eng.pooled_moments_by_rung()
    assert mom.shape == (k_rungs, 1 + d + d * (d + 1) // 2 + 2 * d + 2)
    il = np.tril_indices(d)
    diag = np.flatnonzero(il[0] == il[1])
    for k in range(k_rungs):
        cnt, sx, sxx = mom[k, 0], mom[k, 1:1 + d], mom[k, 1 + d:1 + d + d * (d + 1) // 2]
        assert cnt == m
        var = np.mean(sxx[diag] / cnt - (sx / cnt) ** 2)
        want = temps[k] / (2 * a)
        assert abs(var - want) < 5 * want * np.sqrt(2.0 / (d * m)), (k, var, want)
    # swap acceptance per pair against E[min(1, exp(dbeta (E_lo - E_hi)))], E_k ~ Gamma(D/2, T_k) exactly
    eng.set_temperatures(temps)                    # counters start over; the state stays
    per_round = []
    last = np.zeros((2, k_rungs - 1))
    for _ in range(40):
        eng.step_all(20)
        eng.replica_exchange()
        _, att, acc = eng.swap_stats()
        per_round.append(np.where(att > last[0], (acc - last[1]) / np.maximum(att - last[0], 1), np.nan))
        last = np.array([att, acc], dtype=float)
    _, att, acc = eng.swap_stats()
    assert np.all(att == 20 * m)
    rng = np.random.default_rng(1)
    for k in range(k_rungs - 1):
        e_lo, e_hi = rng.gamma(d / 2, temps[k] / a, 1 << 20), rng.gamma(d / 2, temps[k + 1] / a, 1 << 20)
        want = np.mean(np.minimum(1.0, np.exp((1 / temps[k] - 1 / temps[k + 1]) * (e_lo - e_hi))))
        got = acc[k] / att[k]
        rounds = np.array([r[k] for r in per_round if not np.isnan(r[k])])
        se = max(np.std(rounds) / np.sqrt(rounds.size), np.sqrt(want * (1 - want) / att[k]))
        assert abs(got - want) < 5 * se, (k, got, want, se)
    assert np.allclose(eng.swap_acceptance(), acc / att)


# ---------------------------------------------------------------------------------------------------- 5. mixing
def _demo():
    spec = importlib.util.spec_from_file_location("demo_parallel_tempering", os.path.join(EXAMPLES, "demo_parallel_tempering.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_double_well_cold_rung_mixes_only_with_swaps(capsys):
    demo = _demo()
    assert abs(demo.BARRIER / demo.LADDER[0] - 40) < 1e-9
    with_swaps, without = demo.main()
    assert abs(demo.right_well_fraction(with_swaps)[0] - 0.5) < 0.05
    assert demo.right_well_fraction(without)[0] < 0.05
    assert np.all(with_swaps.swap_acceptance() > 0.05)
    assert "fraction at x > 0" in capsys.readouterr().out


# ---------------------------------------------------------------------------------------------------- 6. checkpoint
def test_checkpoint_continues_bitwise():
    kw = dict(n_chains=256, seed=8, dtype="f64")
    args = (me.DiagQuadratic((1, 2), (3,)), None, [0.2, 0.1], [0.1j])
    temps = [0.4, 0.7, 1.1, 1.6]

    def drive(e, cycles):
        for _ in range(cycles):
            e.step_all(2)
            e.replica_exchange()
            e.measure()

    whole = me.MetropolisEngine(*args, temperatures=temps, **kw)
    part = me.MetropolisEngine(*args, temperatures=temps, **kw)
    drive(whole, 55)
    drive(part, 30)
    state = part.state_dict()
    assert np.array_equal(state["temperatures"], temps) and state["replica_round"] == 30
    assert state["swap_attempted"].shape == (3,)
    scalar = me.MetropolisEngine(*args, temp=1.0, **kw).state_dict()
    assert not {"temperatures", "replica_round", "swap_attempted", "swap_accepted"} & set(scalar)
    resumed = me.MetropolisEngine(*args, **kw)     # created without a ladder: the checkpoint brings it
    bad = dict(state, swap_accepted=state["swap_attempted"] + 1)
    with pytest.raises(ValueError):
        resumed.load_state_dict(bad)
    assert resumed.temperatures is None            # refused before anything was written
    resumed.load_state_dict(state)
    drive(resumed, 25)
    for field in (_capi.FIELD_PARAMS, _capi.FIELD_ENERGY, _capi.FIELD_WIDTH, _capi.FIELD_MEAN, _capi.FIELD_COV,
                  _capi.FIELD_FACTOR, _capi.FIELD_OBS_MEAN):
        assert np.array_equal(whole._get(field), resumed._get(field)), field
    w, r = whole.swap_stats(), resumed.swap_stats()
    assert w[0] == r[0] == 55 and np.array_equal(w[1], r[1]) and np.array_equal(w[2], r[2])
    assert whole.accept_stats() == resumed.accept_stats()


# ---------------------------------------------------------------------------------------------------- 7. refusals, moments
def test_engines_without_ladders_refuse_them():
    rng = np.random.default_rng(2)
    q = rng.standard_normal((64, 64))
    dense = me.MetropolisEngine(me.DenseQuadratic(q @ q.T / 64 + np.identity(64)), None, [0.0] * 64, None, n_chains=128,
                                cov_mode="fixed")
    with pytest.raises(NotImplementedError, match="dense"):
        dense.set_temperatures([1.0, 2.0])
    with pytest.raises(NotImplementedError, match="runtime-dimension"):
        me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 130, None, n_chains=128, cov_mode="fixed",
                            temperatures=[1.0, 2.0])
    ledgers = me.MetropolisEngine(me.LandauToy(), None, [0.0, 0.0], [0j], n_chains=128, reference_energy_ledgers=True)
    with pytest.raises(NotImplementedError, match="LEDGERS"):
        ledgers.set_temperatures([1.0, 2.0])
    assert ledgers.temperatures is None
    plain = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0], None, n_chains=128)
    with pytest.raises(Exception):
        plain.replica_exchange()                   # no ladder: ME_ERR_STATE


@pytest.mark.parametrize("nr, nc, dtype", [(4, 0, "f64"), (16, 0, "f32"), (2, 2, "f64")])
def test_pooled_moments_by_rung_equal_numpy_on_rung_slices(nr, nc, dtype):
    temps = [0.5, 1.0, 2.0]
    d = nr + 2 * nc
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * nr if nr else None, [0.1j] * nc if nc else None,
                              n_chains=3 * 128, seed=3, dtype=dtype, temperatures=temps)
    for _ in range(20):
        eng.step_all(5)
        eng.replica_exchange()
    mom = eng.pooled_moments_by_rung()
    x = eng._get(_capi.FIELD_PARAMS)
    il = np.tril_indices(d)
    for k in range(3):
        s = x[k * 128:(k + 1) * 128]
        z = s[:, nr:nr + nc] + 1j * s[:, nr + nc:]
        obs = np.concatenate((np.abs(s[:, :nr]), np.abs(z), s[:, :nr] ** 2), axis=1)
        want = np.concatenate(([128.0], s.sum(0), np.einsum("ni,nj->ij", s, s)[il], obs.sum(0), [0.0, 0.0]))
        assert np.allclose(mom[k], want, rtol=1e-12 if dtype == "f64" else 1e-5, atol=1e-12 if dtype == "f64" else 1e-4), k
    assert np.array_equal(mom, eng.pooled_moments_by_rung())      # reproducible bit for bit
