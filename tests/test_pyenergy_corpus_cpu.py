"""The corpus of reference-style Python energies (tests/pyenergy_corpus.py) against metropolisengine_amd/pyenergy.py on
the CPU: every traceable energy's recorded graph equals the callable on float64 / complex128 numbers, at random and edge
states of its domain; every traceable reject condition agrees as a boolean away from ties; everything the tracer cannot
record is refused with a TraceError and nothing else; and the source the emitter writes -- compiled for the host with
g++ against tests/native/metropolis_user_energy.h -- matches a long-double evaluation of the graph term by term, in
float64 and float32.  The plugins of tests/test_gpu_pyenergy_corpus.py are built here too."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from metropolisengine_amd import pyenergy as pe

import pyenergy_corpus as corpus                                                                  # noqa: E402
from pyenergy_eval import comparison_margin, error_ratio, evaluate, evaluate_scaled               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LD = np.longdouble
N_RANDOM = 256


def _ids(entries):
    return ["%s-%s" % (e.kind, e.name) for e in entries]


def _numeric(fn, x, shape):
    return np.array([corpus.call(fn, row, shape) for row in x])


def _assert_graph_equals_callable(node, fn, x, shape, what):
    want = _numeric(fn, x, shape)
    got, scale = evaluate_scaled(node, x)
    got = np.broadcast_to(got, want.shape)
    with np.errstate(all="ignore"):
        tol = 1e-12 * np.abs(want) + 64 * np.finfo(np.float64).eps * scale
        ok = (np.abs(got - want) <= tol) | (np.isnan(got) & np.isnan(want)) | (np.isinf(want) & (got == want))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: graph %r != callable %r at %s" % (what, got[bad[0]], want[bad[0]], x[bad[0]].tolist())


def test_corpus_size():
    assert len(corpus.entries("energy")) + len(corpus.entries("dict")) >= 40
    assert len(corpus.entries("reject")) >= 10
    for shape in corpus.GPU_SHAPES:
        assert 1 <= len(corpus.entries("energy", "trace", shape)) <= 12


@pytest.mark.parametrize("entry", corpus.entries("energy", "trace"), ids=_ids(corpus.entries("energy", "trace")))
def test_traced_energy_equals_the_callable(entry):
    nr, nc = entry.shape
    node = pe.trace_energy(entry.fn, nr, nc)
    x = corpus.states(entry.domain, entry.shape, N_RANDOM, np.random.default_rng(17))
    _assert_graph_equals_callable(node, entry.fn, x, entry.shape, entry.name)
    source, names = pe.generate_source(entry.fn, nr, nc)       # the self-check at construction accepts it
    assert names == ("total",) and "me_user_energy" in source


@pytest.mark.parametrize("entry", corpus.entries("dict", "trace"), ids=_ids(corpus.entries("dict", "trace")))
def test_traced_term_dictionary_equals_every_group_callable(entry):
    nr, nc = entry.shape
    source, names = pe.generate_source(entry.fn, nr, nc)
    assert names == tuple(sorted(set().union(*entry.fn.values())))
    x = corpus.states(entry.domain, entry.shape, N_RANDOM, np.random.default_rng(18))
    for name in names:
        groups = [g for g in ("all", "real", "complex") if name in entry.fn.get(g, {})]
        node = pe.trace_energy(entry.fn[groups[0]][name], nr, nc)
        for g in groups:
            _assert_graph_equals_callable(node, entry.fn[g][name], x, entry.shape, "%s[%s][%s]" % (entry.name, g, name))


@pytest.mark.parametrize("entry", corpus.entries("reject", "trace"), ids=_ids(corpus.entries("reject", "trace")))
def test_traced_reject_agrees_away_from_ties(entry):
    nr, nc = entry.shape
    node = pe.trace_reject(entry.fn, nr, nc)
    x = corpus.states(entry.domain, entry.shape, N_RANDOM, np.random.default_rng(19))
    x = np.vstack([x, np.random.default_rng(20).uniform(-3.0, 3.0, size=(N_RANDOM, x.shape[1]))])
    want = _numeric(entry.fn, x, entry.shape).astype(bool)
    got = np.broadcast_to(evaluate(node, x), want.shape)
    clear = comparison_margin(node, x) > 1e-9
    assert clear.sum() > 0.9 * len(x)
    assert np.array_equal(got[clear], want[clear])
    assert 0 < want.sum() < len(x)                              # a predicate that never (or always) rejects tests nothing


@pytest.mark.parametrize("entry", corpus.entries(expect="refuse"), ids=_ids(corpus.entries(expect="refuse")))
def test_refused_with_a_trace_error(entry):
    nr, nc = entry.shape
    with pytest.raises(pe.TraceError):
        if entry.kind == "reject":
            pe.generate_source(lambda r, c: 0.0, nr, nc, reject=entry.fn)
        else:
            pe.generate_source(entry.fn, nr, nc)


def test_self_check_refuses_a_graph_that_is_not_the_callable():
    """An idiom that records something other than what numpy computes is caught by the numeric check at construction --
    here a callable that answers symbols and numbers differently -- and so is one that is wrong only at the initial
    state."""
    def two_faced(r, c):
        return np.sum(r ** 2) + (0.0 if isinstance(r, pe.SymArray) else 1e-3)
    pe.trace_energy(two_faced, 2, 0)
    with pytest.raises(pe.TraceError, match="records differently"):
        pe.generate_source(two_faced, 2, 0)

    def wrong_at_three(r, c):
        return r[0] ** 2 if isinstance(r, pe.SymArray) else (r[0] ** 2 if r[0] != 3.0 else 0.0)
    pe.generate_source(wrong_at_three, 1, 0)
    with pytest.raises(pe.TraceError, match="records differently"):
        pe.generate_source(wrong_at_three, 1, 0, initial=[3.0])


def test_unexpected_exceptions_become_trace_errors_naming_the_cause():
    with pytest.raises(pe.TraceError, match="log1p") as info:
        pe.trace_energy(lambda r, c: np.log1p(r[0]), 1, 0)
    assert info.value.__cause__ is not None and not isinstance(info.value.__cause__, pe.TraceError)
    with pytest.raises(pe.TraceError, match="ZeroDivisionError"):
        pe.trace_energy(lambda r, c: r[0] + 1 / 0, 1, 0)


def test_complex_array_views_act_element_by_element():
    """The advisor's case: sum(re^2 + im^2) was recorded as sum(re^2 - im^2)."""
    fn = lambda r, c: np.sum(c.real ** 2 + c.imag ** 2)                                           # noqa: E731
    node = pe.trace_energy(fn, 0, 3)
    x = np.random.default_rng(4).standard_normal(6)
    assert np.isclose(evaluate(node, x), np.sum(x ** 2), rtol=1e-14)
    real, cplx = pe._inputs(1, 2)
    assert all(v is w.re for v, w in zip(cplx.real, cplx)) and all(v is w.im for v, w in zip(np.imag(cplx), cplx))
    assert isinstance((cplx * cplx.conj()).real, pe.SymArray) and real.imag[0].op == "const"


# ---------------------------------------------------------------------------------------------- the emitter on the host
def _host_plugin(shape, tmp):
    energy, nr, nc, reject = corpus.PLUGINS[corpus.GPU_SHAPES.index(shape)]
    source, names = pe.generate_source(energy, nr, nc, reject)
    header = os.path.join(tmp, "plugin_%d_%d.h" % shape)
    with open(header, "w") as fh:
        fh.write(source)
    lib_path = os.path.join(tmp, "libplugin_%d_%d.so" % shape)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", NATIVE,
                    "-DME_PYENERGY_SOURCE=\"%s\"" % header, os.path.join(NATIVE, "pyenergy_host.cpp"), "-o", lib_path],
                   check=True)
    lib = ctypes.CDLL(lib_path)
    lib.me_host_term_groups.restype = ctypes.c_uint
    return lib, energy, names, reject


def plugin_states(shape, n_random, rng):
    """Random and edge states of every domain the shape's plugin uses."""
    domains = sorted(set(corpus.plugin_domains(shape).values()) | {corpus.ANY})
    return np.vstack([corpus.states(d, shape, n_random, rng) for d in domains])


@pytest.mark.parametrize("shape", corpus.GPU_SHAPES, ids=["%d_%d" % s for s in corpus.GPU_SHAPES])
def test_emitted_source_compiled_for_the_host_matches_long_double(shape, tmp_path):
    assert np.finfo(LD).nmant >= 63
    lib, energy, names, reject = _host_plugin(shape, str(tmp_path))
    nr, nc = shape
    assert lib.me_host_n_terms() == len(names)
    assert all(lib.me_host_term_groups(t) == (1 if nr else 0) | (2 if nc else 0) for t in range(len(names)))
    x = plugin_states(shape, N_RANDOM, np.random.default_rng(23))
    n, d = x.shape
    domains = corpus.plugin_domains(shape)
    for dtype, fn_name, k in ((np.float64, "me_host_terms_f64", 64), (np.float32, "me_host_terms_f32", 256)):
        xin = np.ascontiguousarray(x, dtype=dtype)
        out = np.empty((n, len(names)), dtype=dtype)
        getattr(lib, fn_name)(n, d, xin.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        exact = xin.astype(LD)
        for t, name in enumerate(names):
            ref, scale = evaluate_scaled(pe.trace_energy(energy["all"][name], nr, nc), exact)
            mask = corpus.in_domain(xin.astype(np.float64), domains[name])
            assert mask.sum() >= 32, name
            ratio = error_ratio(out[mask, t], np.broadcast_to(ref, (n,))[mask], np.broadcast_to(scale, (n,))[mask], dtype)
            worst = int(np.argmax(ratio))
            assert ratio[worst] <= k, "%s %s: %r vs %r at %s" % (np.dtype(dtype).name, name, out[mask, t][worst],
                                                                 np.broadcast_to(ref, (n,))[mask][worst],
                                                                 xin[mask][worst].tolist())
    if reject is not None:
        flags = np.empty(n, dtype=np.uint8)
        x64 = np.ascontiguousarray(x)
        assert lib.me_host_reject_f64(n, d, x64.ctypes.data_as(ctypes.c_void_p), flags.ctypes.data_as(ctypes.c_void_p)) == 1
        node = pe.trace_reject(reject, nr, nc)
        clear = comparison_margin(node, x64.astype(LD)) > 1e-12
        assert np.array_equal(flags[clear].astype(bool), np.broadcast_to(evaluate(node, x64.astype(LD)), (n,))[clear])


def test_corpus_plugins_compile_for_gfx950():
    """hipcc for each corpus plugin, as the engine's constructor does on first use (and __graft_entry__.build()); the GPU
    side finds them up to date."""
    for energy, nr, nc, reject in corpus.PLUGINS:
        spec = pe.PythonEnergy(energy, reject=reject)
        plugin = spec.build_plugin(nr, nc)
        assert os.path.exists(plugin) and spec.name in plugin
        assert len(spec.term_names) == len(energy["all"])
