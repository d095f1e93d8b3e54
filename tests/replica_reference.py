"""Replica exchange restated in numpy on per-rung ``ManyChainOracle``s -- TEST INFRASTRUCTURE ONLY.

A ladder engine of K rungs x M chains is K oracles: rung k is ``ManyChainOracle(temp=T_k, chain_offset=offset + k*M,
n_chains=M)``.  A swap round ``r`` pairs rung k with rung k+1 for every ``k = r (mod 2)``; slot j of the two rungs swaps its
configuration (x and the energy) when ``delta = (1/T_k - 1/T_{k+1}) (E_a - E_b) >= 0`` or ``u <= exp(delta)``, ``u`` = word 0
of Philox block 0xffff at (global id of the rung-k chain, round ``r``); a non-finite energy never swaps.  Everything else an
oracle holds (widths, means, covariances, factors, counters) stays where it is.
"""
import numpy as np

from oracle import philox

SWAP_BLOCK = 0xFFFF


def swap_uniforms(seed, chain_ids, rnd):
    """The accept uniform of swap round ``rnd`` for the pairs whose lower-rung chains are ``chain_ids``."""
    return philox.unit_open(philox.step_block(seed, chain_ids, rnd, SWAP_BLOCK)[0])


def swap_decisions(e_lo, e_hi, t_lo, t_hi, u):
    """Accept mask of one pair of rungs: energies of the rung-k / rung-(k+1) chains, their temperatures, the uniforms."""
    e_lo = np.asarray(e_lo, dtype=np.float64)
    e_hi = np.asarray(e_hi, dtype=np.float64)
    delta = (1.0 / t_lo - 1.0 / t_hi) * (e_lo - e_hi)
    with np.errstate(over="ignore", invalid="ignore"):
        ok = (delta >= 0) | (u <= np.exp(np.minimum(delta, 0.0)))
    return np.isfinite(e_lo) & np.isfinite(e_hi) & ok


class ReplicaReference:
    """Drives the swap rounds of a list of per-rung oracles (``oracles[k]`` at ``temperatures[k]``)."""

    def __init__(self, oracles, temperatures, seed):
        self.oracles = list(oracles)
        self.temperatures = np.asarray(temperatures, dtype=np.float64)
        assert len(self.oracles) == self.temperatures.size
        self.seed = int(seed)
        self.round = 0
        self.attempted = np.zeros(max(len(self.oracles) - 1, 0), dtype=np.int64)
        self.accepted = np.zeros_like(self.attempted)

    def exchange(self, n_rounds=1):
        for _ in range(n_rounds):
            r = self.round
            for k in range(r % 2, len(self.oracles) - 1, 2):
                lo, hi = self.oracles[k], self.oracles[k + 1]
                u = swap_uniforms(self.seed, lo.chain_ids, r)
                acc = swap_decisions(lo.energy, hi.energy, self.temperatures[k], self.temperatures[k + 1], u)
                x_lo, e_lo = lo.x[acc].copy(), lo.energy[acc].copy()
                lo.x[acc], lo.energy[acc] = hi.x[acc], hi.energy[acc]
                hi.x[acc], hi.energy[acc] = x_lo, e_lo
                self.attempted[k] += acc.size
                self.accepted[k] += int(np.count_nonzero(acc))
            self.round += 1

    # the engine's view of the whole ladder
    def field(self, name):
        return np.concatenate([getattr(o, name) for o in self.oracles], axis=0)
