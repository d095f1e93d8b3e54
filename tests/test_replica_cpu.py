"""Temperature ladders and replica exchange, without a GPU: the Python-side validation of a ladder, the swap move of the
numpy reference (tests/replica_reference.py) against exact Boltzmann energy distributions, and the separation of the swap
draws from the step draws of the same chain."""
import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd.engine import validate_ladder
from oracle import philox
from replica_reference import SWAP_BLOCK, ReplicaReference, swap_decisions, swap_uniforms

# ---------------------------------------------------------------------------------------------------- validation


@pytest.mark.parametrize("temps, n_chains", [
    ([1.0, 0.5, 2.0], 192),            # not increasing
    ([1.0, 1.0], 128),                 # not strictly increasing
    ([0.0, 1.0], 128),                 # T = 0
    ([-1.0, 1.0], 128),                # negative
    ([1.0, np.inf], 128),              # not finite
    ([1.0, np.nan], 128),
    ([], 64),                          # empty
    ([[1.0, 2.0]], 128),               # not 1-D
    ([1.0, 2.0], 192),                 # 192 chains are not 2 rungs of whole 64-chain tiles
    ([1.0, 2.0, 4.0], 64 * 3 + 1),
])
def test_bad_ladders_are_refused_before_the_engine_exists(temps, n_chains):
    with pytest.raises(ValueError):
        validate_ladder(temps, n_chains)
    # the constructor checks before it loads the library or creates anything on a device
    with pytest.raises(ValueError):
        me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, n_chains=n_chains, temperatures=temps)


def test_temperatures_and_a_nonzero_temp_exclude_each_other():
    with pytest.raises(ValueError, match="temp"):
        me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * 4, None, temp=1.0, n_chains=128, temperatures=[1.0, 2.0])


def test_good_ladders_pass_validation():
    t = validate_ladder([0.5, 1.0, 2.0, 4.0], 4 * 64 * 3)
    assert t.dtype == np.float64 and t.shape == (4,)
    assert validate_ladder((3.0,), 64).tolist() == [3.0]


# ---------------------------------------------------------------------------------------------------- the swap move


def _chi2(sample, reference, n_bins=24):
    """Chi-square of `sample` against bins of equal mass under `reference` (a much larger sample of the target law)."""
    edges = np.quantile(reference, np.linspace(0, 1, n_bins + 1)[1:-1])
    obs = np.bincount(np.searchsorted(edges, sample), minlength=n_bins)
    exp = np.bincount(np.searchsorted(edges, reference), minlength=n_bins) / reference.size * sample.size
    return float(np.sum((obs - exp) ** 2 / exp))


@pytest.mark.parametrize("dim, t_lo, t_hi", [(16, 1.0, 1.5), (4, 0.5, 2.0)])
def test_swap_keeps_the_product_of_the_boltzmann_energy_laws(dim, t_lo, t_hi):
    # E = a |x|^2 over D real coordinates at temperature T is Gamma(D/2, scale T), whatever a: draw the two rungs' energies
    # exactly from their laws, apply one swap, and the pair must still follow the same product law
    rng = np.random.default_rng(11)
    n = 1 << 17
    e_lo = rng.gamma(dim / 2, t_lo, n)
    e_hi = rng.gamma(dim / 2, t_hi, n)
    u = swap_uniforms(2026, np.arange(n, dtype=np.uint64), 3)
    acc = swap_decisions(e_lo, e_hi, t_lo, t_hi, u)
    assert 0.05 < acc.mean() < 0.95          # the move does something
    new_lo = np.where(acc, e_hi, e_lo)
    new_hi = np.where(acc, e_lo, e_hi)
    ref_lo = rng.gamma(dim / 2, t_lo, 1 << 21)
    ref_hi = rng.gamma(dim / 2, t_hi, 1 << 21)
    # 23 degrees of freedom: 60 is beyond the 1e-5 tail
    assert _chi2(new_lo, ref_lo) < 60
    assert _chi2(new_hi, ref_hi) < 60
    # ... and a move that always swaps would not (control: the test has the power to see a wrong rule)
    assert _chi2(e_hi, ref_lo) > 1000


def test_swap_acceptance_matches_its_expectation_under_the_product_law():
    dim, t_lo, t_hi = 8, 1.0, 1.3
    rng = np.random.default_rng(3)
    n = 1 << 18
    e_lo, e_hi = rng.gamma(dim / 2, t_lo, n), rng.gamma(dim / 2, t_hi, n)
    expected = np.mean(np.minimum(1.0, np.exp((1 / t_lo - 1 / t_hi) * (e_lo - e_hi))))
    acc = swap_decisions(e_lo, e_hi, t_lo, t_hi, swap_uniforms(7, np.arange(n, dtype=np.uint64), 0))
    assert abs(acc.mean() - expected) < 5 * np.sqrt(expected * (1 - expected) / n)


def test_non_finite_energies_never_swap():
    e_lo = np.array([np.nan, 1.0, np.inf, 5.0])
    e_hi = np.array([0.0, np.nan, 0.0, 0.0])
    assert not swap_decisions(e_lo, e_hi, 1.0, 2.0, np.full(4, 1e-9))[:3].any()
    assert swap_decisions(e_lo, e_hi, 1.0, 2.0, np.full(4, 1e-9))[3]      # E_a > E_b: delta > 0, always


class _Rung:
    def __init__(self, x, energy, chain_ids):
        self.x, self.energy, self.chain_ids = x, energy, chain_ids


def test_reference_rounds_alternate_pairs_and_count_exactly():
    k_rungs, m = 4, 64
    rng = np.random.default_rng(0)
    rungs = [_Rung(rng.standard_normal((m, 3)), rng.gamma(1.5, 1.0 + k, m), np.arange(k * m, (k + 1) * m, dtype=np.uint64))
             for k in range(k_rungs)]
    before = [(r.x.copy(), r.energy.copy()) for r in rungs]
    ref = ReplicaReference(rungs, [1.0, 2.0, 3.0, 4.0], seed=5)
    ref.exchange(1)          # round 0: pairs (0, 1) and (2, 3)
    assert ref.round == 1 and ref.attempted.tolist() == [m, 0, m]
    # configurations moved as (x, energy) units, and only between partners
    for k, (lo, hi) in enumerate([(0, 1), (2, 3)]):
        swapped = ~np.isclose(rungs[lo].energy, before[lo][1])
        assert swapped.sum() == ref.accepted[2 * k]
        assert np.array_equal(rungs[lo].x[swapped], before[hi][0][swapped])
        assert np.array_equal(rungs[hi].energy[swapped], before[lo][1][swapped])
    ref.exchange(1)          # round 1: pair (1, 2)
    assert ref.attempted.tolist() == [m, m, m]
    assert np.all(ref.accepted <= ref.attempted)


# ---------------------------------------------------------------------------------------------------- random streams


def test_swap_draws_never_meet_the_step_draws_of_the_same_chain():
    # Ladders exist on the compiled kernel sets (at most 128 degrees of freedom): a Gaussian step uses words 0 .. 128, the
    # magnitude-phase pair at most 2 * 32 + 64 + 2 words -- 33 Philox blocks either way, blocks 0 .. 32.
    max_blocks = max((2 * ((128 + 1) // 2) + 1 + 3) // 4, (2 * ((64 + 1) // 2) + 64 + 2 + 3) // 4)
    assert max_blocks == 33 and SWAP_BLOCK >= max_blocks
    ids = np.array([0, 1, 63, 64, (1 << 32) + 5, (1 << 40) + 3], dtype=np.uint64)
    for rnd in (0, 1, 17, (1 << 32) + 2):
        swap = philox.step_block(2026, ids, rnd, SWAP_BLOCK)[0]
        # the counter differs in its block field from every step block of step `rnd` ...
        c3_swap = (((rnd >> 32) & 0xFFFF) << 16) | SWAP_BLOCK
        assert all(c3_swap != ((((rnd >> 32) & 0xFFFF) << 16) | b) for b in range(max_blocks))
        # ... and the words themselves are not among that step's words
        step = philox.step_words(2026, ids, rnd, 4 * max_blocks)
        assert not np.any(step == swap[:, None])
    # the uniform is the open-interval map of word 0 of that block
    u = swap_uniforms(9, ids, 4)
    assert np.array_equal(u, philox.unit_open(philox.step_block(9, ids, 4, 0xFFFF)[0]))
    assert np.all((u > 0) & (u < 1))
