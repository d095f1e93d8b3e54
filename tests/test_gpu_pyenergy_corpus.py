"""The Python-energy corpus (tests/pyenergy_corpus.py) on the GPU: every traceable energy is one term of a term-dictionary
plugin per parameter shape -- (3, 0), (0, 3), (2, 3) and (2, 7), the last with D = 16 and tile-major state -- and every
ledger row is compared with a long-double evaluation of the traced graph at the state the engine holds, within
``k * eps * A(x)`` (A: the rounding scale of tests/pyenergy_eval.py), in float64 and float32: once after
``initialize_energy_dict()`` (the init kernel) and once after three sweeps (the terms as inlined into the step kernel).
The (2, 3) plugin also carries a traced reject condition and follows the many-chain oracle, which calls the Python
callables themselves."""
import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi
from metropolisengine_amd import pyenergy as pe
from oracle.manychain import ManyChainOracle

import pyenergy_corpus as corpus                                                                  # noqa: E402
from pyenergy_eval import error_ratio, evaluate_scaled                                            # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = 4096 + 37                                          # a ragged last tile
BOUND = {"f64": (np.float64, 64), "f32": (np.float32, 256)}
INITIAL = {(3, 0): ([0.3, 0.5, 0.7], None), (0, 3): (None, [0.5 + 0.2j, 0.3 + 0.6j, 0.4 + 0.1j]),
           (2, 3): ([0.3, -0.2], [0.1 + 0.2j, -0.3j, 0.5]),
           (2, 7): ([0.4, 0.6], [0.5 + 0.5j, 0.3 + 0.7j, 0.6 + 0.2j, 0.2 + 0.4j, 0.7 + 0.3j, 0.4 + 0.6j, 0.5 + 0.1j])}


def _states(shape, rng):
    """N rows: the edge states of the domain where every term of the plugin is defined, then random states of it."""
    domain = corpus.plugin_domain(shape)
    edges = corpus.edge_states(domain, shape, rng)
    return np.vstack([edges, corpus.random_states(domain, shape, N - len(edges), rng)])


def _worst_ratio(eng, shape, dtype, k):
    """The largest |E_gpu - E_ref| / (eps A + tiny) over every ledger row and term whose state lies in the term's domain."""
    energy = corpus.plugin_dictionary(shape)
    domains = corpus.plugin_domains(shape)
    x = eng._get(_capi.FIELD_PARAMS)
    ledger = eng._get(_capi.FIELD_ENERGY)
    assert ledger.shape == (N, len(eng.energy_term_names))
    worst = 0.0
    for t, name in enumerate(eng.energy_term_names):
        ref, scale = evaluate_scaled(pe.trace_energy(energy["all"][name], *shape), x.astype(LD))
        mask = corpus.in_domain(x, domains[name])
        assert mask.sum() >= 64, name
        ratio = error_ratio(ledger[mask, t], np.broadcast_to(ref, (N,))[mask], np.broadcast_to(scale, (N,))[mask], dtype)
        i = int(np.argmax(ratio))
        worst = max(worst, float(ratio[i]))
        assert ratio[i] <= k, "%s: %r vs %r (ratio %.3g) at %s" % (
            name, ledger[mask, t][i], np.broadcast_to(ref, (N,))[mask][i], float(ratio[i]), x[mask][i].tolist())
    return worst


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("shape", corpus.GPU_SHAPES, ids=["%d_%d" % s for s in corpus.GPU_SHAPES])
def test_ledger_at_set_states_and_after_steps(shape, dtype_name):
    assert np.finfo(LD).nmant >= 63
    dtype, k = BOUND[dtype_name]
    energy, nr, nc, reject = corpus.PLUGINS[corpus.GPU_SHAPES.index(shape)]
    r0, c0 = INITIAL[shape]
    eng = me.MetropolisEngine(energy, reject, r0, c0, temp=100.0, n_chains=N, seed=31, dtype=dtype_name,
                              sampling_width=0.2)
    assert eng.energy_term_names == sorted(energy["all"])
    x = _states(shape, np.random.default_rng(41))
    eng._set(_capi.FIELD_PARAMS, x)
    eng.initialize_energy_dict()
    held = eng._get(_capi.FIELD_PARAMS)
    assert held.shape == x.shape and np.allclose(held, x, rtol=np.finfo(dtype).eps, atol=0)
    init = _worst_ratio(eng, shape, dtype, k)

    eng.step_all(3)                                    # the terms as inlined into the step kernel
    moved = np.any(eng._get(_capi.FIELD_PARAMS) != held, axis=1)
    assert moved.sum() >= 200, moved.sum()
    step = _worst_ratio(eng, shape, dtype, k)
    ledger = eng._get(_capi.FIELD_ENERGY)
    assert np.allclose(eng.energy_total, ledger.sum(axis=1), rtol=1e-12, atol=0, equal_nan=True)
    print("\nPYENERGY_CORPUS_RATIO shape=%d_%d dtype=%s init=%.3f step=%.3f" % (nr, nc, dtype_name, init, step))


def test_reject_plugin_follows_the_oracle():
    """The (2, 3) plugin with its traced reject condition, float64, against the oracle calling the Python callables."""
    shape = (2, 3)
    energy, nr, nc, reject = corpus.PLUGINS[corpus.GPU_SHAPES.index(shape)]
    assert reject is not None
    terms = list(energy["all"].values())
    n, seed = 128, 77
    r0, c0 = INITIAL[shape]

    def total(x):
        return np.array([sum(corpus.call(fn, row, shape) for fn in terms) for row in x])

    def rejected(x):
        return np.array([bool(corpus.call(reject, row, shape)) for row in x])

    eng = me.MetropolisEngine(energy, reject, r0, c0, temp=1.0, n_chains=n, seed=seed, dtype="f64", sampling_width=0.3)
    ora = ManyChainOracle(nr, nc, total, n, seed=seed, temp=1.0, initial_real_params=r0, initial_complex_params=c0,
                          sampling_width=0.3, reject=rejected)
    for _ in range(3):
        eng.step_all(10)
        ora.step(10)
        eng.measure()
        ora.measure()
    assert np.allclose(eng._get(_capi.FIELD_PARAMS), ora.x, rtol=0, atol=1e-9)
    assert np.allclose(eng.energy_total, ora.energy, rtol=0, atol=1e-9)
    accepted, proposed = eng.accept_stats()
    assert (accepted, proposed) == (ora.accepted, ora.proposed)
    assert 0 < accepted < proposed
    assert not np.any(rejected(eng._get(_capi.FIELD_PARAMS)))
