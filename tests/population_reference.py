"""One population-annealing stage restated in numpy -- TEST INFRASTRUCTURE ONLY.

The same arithmetic as ``metropolisengine_amd/csrc/me_population.hip`` (whose header comment states it):

* ``E_i`` = the chain's ledger rows summed in row order in the engine's dtype; ``l_i = -(1/T_new - 1/T_old) E_i`` in float64;
  a non-finite ``l_i`` has weight 0.
* The chains are cut into blocks of ``CHUNK`` consecutive chains.  Per block ``b``: ``m_b`` = the max of its finite ``l_i``,
  ``v_i = exp(l_i - m_b)``, ``Q_i`` = the running sum of ``v`` inside the block, ``s_b`` = its last value, ``q_b = sum v_i^2``.
* ``M = max m_b``, ``f_b = exp(m_b - M)``; block offsets ``O_0 = 0``, ``O_{b+1} = O_b + f_b s_b`` and
  ``S2 = sum_b (f_b f_b) q_b``, both added sequentially in block order; ``W = O_B``; ``C_i = O_b + f_b Q_i``.
* ``log_weight = M + ln(W / N)``, ``neff_fraction = W^2 / (N S2)``.
* Slot boundaries ``B_i = ceil((N C_i) / W - u)`` clamped to ``[0, hi]``, ``hi = B(W)``; chain ``i`` owns the slots
  ``[B_{i-1}, B_i)``; slots ``>= hi`` take the ancestor of slot ``hi - 1``.  ``u`` = word 0 of Philox block 0xfffe at
  counter ``(chain_offset, stage)``.
* ``n_finite = 0``: nothing moves, ``log_weight = -inf``, ``neff_fraction = 0``.

The kernel sums inside a block in another association order than ``np.cumsum`` and its ``exp`` may differ from numpy's in
the last bit, so ``C`` agrees to a few ulps, not bit for bit: a slot whose ``j + u`` lies within rounding of a boundary
``N C_i / W`` may get the neighbouring ancestor (:func:`ambiguous_slots`).
"""
import numpy as np

from oracle import philox

POP_BLOCK = 0xFFFE
CHUNK = 2048          # chains per block of the weight and scan passes (kPopChunk)


def stage_uniform(seed, chain_offset, stage):
    """The stage's single uniform in (0, 1)."""
    word = philox.step_block(seed, np.array([chain_offset], dtype=np.uint64), stage, POP_BLOCK)[0]
    return float(philox.unit_open(word)[0])


def ledger_energy(ledger, dtype="f64"):
    """``E_i``: the ledger rows ``ledger[:, t]`` added in row order in the device dtype, returned as float64."""
    ledger = np.asarray(ledger, dtype=np.float64)
    if ledger.ndim == 1:
        ledger = ledger[:, None]
    ft = np.float32 if dtype in ("f32", "float32") else np.float64
    with np.errstate(over="ignore", invalid="ignore"):
        e = ledger[:, 0].astype(ft)
        for t in range(1, ledger.shape[1]):
            e = e + ledger[:, t].astype(ft)
    return e.astype(np.float64)


def stage_weights(energy, t_old, t_new):
    """Weights, sums and the stage record of a population with energies ``energy`` (float64, the dtype's values)."""
    e = np.asarray(energy, dtype=np.float64)
    n = e.size
    neg_dbeta = -(1.0 / float(t_new) - 1.0 / float(t_old))
    with np.errstate(over="ignore", invalid="ignore"):
        l = neg_dbeta * e
    valid = np.isfinite(l)
    n_finite = int(np.count_nonzero(valid))
    n_blocks = (n + CHUNK - 1) // CHUNK
    block = np.arange(n) // CHUNK
    lv = np.where(valid, l, -np.inf)
    m = np.full(n_blocks, -np.inf)
    np.maximum.at(m, block, lv)
    v = np.zeros(n)
    v[valid] = np.exp(l[valid] - m[block[valid]])
    q_run = np.empty(n)
    s = np.zeros(n_blocks)
    sq = np.zeros(n_blocks)
    for b in range(n_blocks):
        sl = slice(b * CHUNK, min(n, (b + 1) * CHUNK))
        q_run[sl] = np.cumsum(v[sl])
        s[b] = q_run[sl][-1]
        sq[b] = np.sum(v[sl] * v[sl])
    out = {"l": l, "valid": valid, "n_finite": n_finite, "v": v}
    if n_finite == 0:
        out.update(M=-np.inf, W=0.0, S2=0.0, C=None, log_weight=-np.inf, neff_fraction=0.0)
        return out
    big_m = float(np.max(m))
    f = np.where(m > -np.inf, np.exp(m - big_m), 0.0)
    offsets = np.zeros(n_blocks + 1)
    o = 0.0
    s2 = 0.0
    for b in range(n_blocks):             # sequentially, in block order
        o = o + f[b] * s[b]
        s2 = s2 + (f[b] * f[b]) * sq[b]
        offsets[b + 1] = o
    w_total = o
    c = offsets[block] + f[block] * q_run
    out.update(M=big_m, W=w_total, S2=s2, C=c, f=f, offsets=offsets,
               log_weight=big_m + np.log(w_total / n), neff_fraction=(w_total * w_total) / (n * s2))
    return out


def _bound(c, n, w_total, u, hi):
    t = np.ceil((float(n) * np.asarray(c, dtype=np.float64)) / w_total - u)
    return np.clip(t, 0, hi).astype(np.int64)


def ancestors(weights, u):
    """``a_j`` for every slot (the identity when no weight is finite)."""
    n = weights["l"].size
    if weights["n_finite"] == 0:
        return np.arange(n, dtype=np.int64)
    w_total = weights["W"]
    hi = int(_bound(np.array([w_total]), n, w_total, u, n)[0])
    upper = _bound(weights["C"], n, w_total, u, hi)
    lower = np.concatenate(([0], upper[:-1]))
    counts = upper - lower
    assert np.all(counts >= 0)
    anc = np.repeat(np.arange(n, dtype=np.int64), counts)
    assert anc.size == hi
    if hi < n:
        anc = np.concatenate((anc, np.full(n - hi, anc[hi - 1], dtype=np.int64)))
    return anc


def offspring_counts(weights, u):
    return np.bincount(ancestors(weights, u), minlength=weights["l"].size)


def ambiguous_slots(weights, u, rel=1e-9):
    """Slots ``j`` whose ``j + u`` lies within ``rel * N`` of some boundary ``N C_i / W``: where a few ulps in ``C`` may
    move the slot to the neighbouring ancestor."""
    n = weights["l"].size
    if weights["n_finite"] == 0:
        return np.zeros(n, dtype=bool)
    t = (float(n) * weights["C"]) / weights["W"]
    pos = np.arange(n) + u
    k = np.searchsorted(t, pos)
    near = np.zeros(n, dtype=bool)
    for kk in (k - 1, k):
        ok = (kk >= 0) & (kk < n)
        near[ok] |= np.abs(t[kk[ok]] - pos[ok]) <= rel * n
    return near


class PopulationReference:
    """Resampling stages applied to a ``ManyChainOracle`` (``x``, ``energy``, ``temp``) plus its family ids."""

    def __init__(self, oracle, seed, chain_offset=0, dtype="f64"):
        self.oracle = oracle
        self.seed = int(seed)
        self.chain_offset = int(chain_offset)
        self.dtype = dtype
        self.stage = 0
        self.families = np.arange(oracle.n_chains, dtype=np.int64) + self.chain_offset
        self.log_weight, self.neff_fraction, self.n_finite, self.temps = [], [], [], []

    def resample(self, t_new):
        o = self.oracle
        w = stage_weights(ledger_energy(o.energy, self.dtype), o.temp, t_new)
        u = stage_uniform(self.seed, self.chain_offset, self.stage)
        anc = ancestors(w, u)
        o.x = o.x[anc].copy()
        o.energy = o.energy[anc].copy()
        self.families = self.families[anc].copy()
        o.temp = float(t_new)
        self.stage += 1
        self.log_weight.append(w["log_weight"])
        self.neff_fraction.append(w["neff_fraction"])
        self.n_finite.append(w["n_finite"])
        self.temps.append(float(t_new))
        return anc
