"""Population annealing without a GPU: the numpy restatement of one resampling stage (tests/population_reference.py) --
identity, conservation and order of the offspring, unbiasedness of systematic resampling, non-finite energies, the
Boltzmann law after a stage -- the Python-side validation, and the separation of the stage's uniform from the step and
swap draws."""
import numpy as np
import pytest

import metropolisengine_amd as me
from oracle import energies, philox
from oracle.manychain import ManyChainOracle
from population_reference import (CHUNK, POP_BLOCK, PopulationReference, ambiguous_slots, ancestors, ledger_energy,
                                  offspring_counts, stage_uniform, stage_weights)
from replica_reference import SWAP_BLOCK


def _energies(n, seed=0, scale=3.0):
    return np.random.default_rng(seed).gamma(2.0, scale, n)


# ---------------------------------------------------------------------------------------------------- the stage


@pytest.mark.parametrize("n", [1, 64, 3000, 2 * CHUNK + 5])
def test_same_temperature_is_the_identity(n):
    e = _energies(n) - 4.0                       # both signs: l = -0 * E is +-0
    w = stage_weights(e, 0.7, 0.7)
    assert w["log_weight"] == 0.0 and w["neff_fraction"] == 1.0 and w["W"] == n
    assert np.array_equal(w["C"], np.arange(1, n + 1, dtype=np.float64))
    for u in (1e-10, 0.5, 1 - 1e-10, stage_uniform(3, 17, 0)):
        assert np.array_equal(ancestors(w, u), np.arange(n))


@pytest.mark.parametrize("n, t_old, t_new", [(3000, 2.0, 1.0), (2 * CHUNK + 77, 1.0, 0.3), (500, 1.0, 1.5),
                                             (CHUNK, 1.0, 0.01)])
def test_offspring_sum_to_n_and_ancestors_are_monotone(n, t_old, t_new):
    w = stage_weights(_energies(n, 1), t_old, t_new)
    for stage in range(8):
        u = stage_uniform(9, 0, stage)
        anc = ancestors(w, u)
        assert anc.shape == (n,) and np.all(np.diff(anc) >= 0)
        counts = offspring_counts(w, u)
        assert counts.sum() == n
        # systematic resampling: every count is the floor or the ceiling of its expectation N w_i / W
        expect = n * np.diff(np.concatenate(([0.0], w["C"]))) / w["W"]
        assert np.all(counts >= np.floor(expect) - 1e-9) and np.all(counts <= np.ceil(expect) + 1e-9)


def test_mean_offspring_is_n_w_over_w():
    n = 3000
    e = _energies(n, 2)
    w = stage_weights(e, 1.0, 0.5)
    # the textbook weights, exp(l_i - M) summed in one piece: the block-wise ones agree to a few ulps
    l = -(1 / 0.5 - 1 / 1.0) * e
    wt = np.exp(l - l.max())
    expect = n * wt / wt.sum()
    k = 4096
    mean = np.zeros(n)
    for j in range(k):
        mean += offspring_counts(w, (j + 0.5) / k)
    mean /= k
    assert np.max(np.abs(mean - expect)) <= 1.0 / k + 1e-9
    assert np.isclose(w["log_weight"], np.log(np.mean(np.exp(l))), rtol=1e-13)
    assert np.isclose(w["neff_fraction"], wt.sum() ** 2 / (n * np.sum(wt * wt)), rtol=1e-13)


def test_non_finite_energies_get_no_offspring():
    n = 700
    e = _energies(n, 3)
    bad = np.zeros(n, dtype=bool)
    bad[[0, 5, 6, 100, 699]] = True
    e[bad] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    w = stage_weights(e, 1.0, 0.5)
    assert w["n_finite"] == n - bad.sum()
    for stage in range(16):
        counts = offspring_counts(w, stage_uniform(1, 0, stage))
        assert counts.sum() == n and not counts[bad].any()
    # nothing finite: the population is left as it is
    none = stage_weights(np.full(n, np.nan), 1.0, 0.5)
    assert none["n_finite"] == 0 and none["log_weight"] == -np.inf and none["neff_fraction"] == 0.0
    assert np.array_equal(ancestors(none, 0.3), np.arange(n))


def test_ledger_energy_sums_rows_in_the_device_dtype():
    rows = np.array([[1.0, 1e-8, -1.0], [0.1, 0.2, 0.3]])
    assert ledger_energy(rows, "f64")[1] == (0.1 + 0.2) + 0.3
    want = np.float32(np.float32(np.float32(1.0) + np.float32(1e-8)) + np.float32(-1.0))
    assert ledger_energy(rows, "f32")[0] == np.float64(want)
    assert np.array_equal(ledger_energy(rows[:, 0]), rows[:, 0])


def test_ambiguous_slots_are_rare():
    n = 1 << 14
    w = stage_weights(_energies(n, 4), 1.0, 0.5)
    assert ambiguous_slots(w, stage_uniform(5, 0, 0)).mean() <= 1e-4


# ---------------------------------------------------------------------------------------------------- physics


def test_resampled_gaussian_population_keeps_the_boltzmann_variance():
    # E = a |x|^2 at temperature T: x_k ~ N(0, T / 2a).  Draw the population exactly at T_old, resample to T_new and step:
    # the variance must be T_new / 2a (resampling alone gets it in expectation; the sweeps restore the diversity)
    a, d, n, t_old, t_new = 1.0, 2, 1 << 13, 1.0, 0.7
    o = ManyChainOracle(d, 0, energies.iso_quadratic(d, 0, a), n, seed=5, temp=t_old, initial_real_params=[0.0] * d,
                        sampling_width=0.5)
    o.x = np.random.default_rng(8).normal(0.0, np.sqrt(t_old / (2 * a)), (n, d))
    o.energy = np.asarray(o.energy_fn(o.x), dtype=np.float64)
    ref = PopulationReference(o, seed=5)
    ref.resample(t_new)
    var0 = o.x.var()
    o.step(20)
    var = o.x.var()
    want = t_new / (2 * a)
    se = want * np.sqrt(2.0 / (n * d))
    assert abs(var0 - want) < 8 * se / np.sqrt(ref.neff_fraction[0])
    assert abs(var - want) < 8 * se, (var, want)
    # the estimate of ln Z(T_new) / Z(T_old) = (D / 2) ln(T_new / T_old)
    assert abs(ref.log_weight[0] - d / 2 * np.log(t_new / t_old)) < 0.02
    assert o.temp == t_new and ref.stage == 1 and np.all(np.diff(ref.families) >= 0)


# ---------------------------------------------------------------------------------------------------- Python validation


@pytest.mark.parametrize("temp", [0.0, -1.0, np.inf, np.nan])
def test_bad_resample_temperatures_are_refused_before_the_library(temp):
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)     # no device: validation comes first
    with pytest.raises(ValueError):
        eng.resample(temp)


@pytest.mark.parametrize("temp", [-1.0, np.inf, np.nan])
def test_bad_scalar_temperatures_are_refused_before_the_library(temp):
    eng = me.MetropolisEngine.__new__(me.MetropolisEngine)
    with pytest.raises(ValueError):
        eng.set_temp(temp)


# ---------------------------------------------------------------------------------------------------- random streams


def test_stage_uniform_never_meets_the_step_or_swap_draws():
    # a step of the compiled kernel sets uses Philox blocks 0 .. 32 (tests/test_replica_cpu.py), the runtime-dimension set
    # (D + 1) / 4 + 1 blocks, far below 0xfffe for any D it accepts; swaps use block 0xffff
    assert POP_BLOCK not in (SWAP_BLOCK,) and POP_BLOCK >= 33 and (290 + 1 + 3) // 4 < POP_BLOCK
    for offset in (0, 64, (1 << 32) + 5):
        for stage in (0, 1, 17, (1 << 32) + 2):
            u_word = philox.step_block(2026, np.array([offset], dtype=np.uint64), stage, POP_BLOCK)[0][0]
            c3 = (((stage >> 32) & 0xFFFF) << 16) | POP_BLOCK
            assert all(c3 != ((((stage >> 32) & 0xFFFF) << 16) | b) for b in range(33))
            assert c3 != ((((stage >> 32) & 0xFFFF) << 16) | SWAP_BLOCK)
            step = philox.step_words(2026, np.array([offset], dtype=np.uint64), stage, 4 * 33)
            assert not np.any(step == u_word)
            swap = philox.step_block(2026, np.array([offset], dtype=np.uint64), stage, SWAP_BLOCK)[0]
            assert swap[0] != u_word
    u = stage_uniform(9, 12, 4)
    assert u == philox.unit_open(philox.step_block(9, np.array([12], dtype=np.uint64), 4, 0xFFFE)[0])[0]
    assert 0 < u < 1
    # a shard at another chain_offset draws another uniform
    assert stage_uniform(9, 0, 4) != stage_uniform(9, 1 << 20, 4)
