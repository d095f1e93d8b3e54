"""The Newton solver for the ladder free energies without a GPU: the numpy restatement of the iteration and of its policy
(tests/mbar_newton_reference.py) on the seven ladders of the README's table, the argument checks that run before the library
is touched, and the C ABI's new symbols.  The GPU side is tests/test_gpu_mbar_newton.py."""
import os
import re

import numpy as np
import pytest

import mbar_newton_reference as nref
import mbar_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# iterations and fallback passes of the float64 restatement at tol = 1e-10, as the README's table has them
EXPECTED = [(8, 0), (8, 0), (8, 0), (9, 0), (9, 0), (10, 0), (15, 2)]


@pytest.mark.parametrize("index", range(len(nref.LADDERS)))
def test_reference_converges_quadratically(index):
    f, iterations, residual, gradient, kinds = nref.solved(index)
    assert f.dtype == np.float64 and residual <= 1e-10 and iterations <= 20
    assert (iterations, nref.fallbacks(kinds)) == EXPECTED[index]
    assert kinds[:2] == [nref.SC, nref.SC] and len(kinds) == iterations
    assert f[0] == 0.0 and gradient <= 1e-6
    error = np.max(np.abs(f.astype(np.longdouble) - nref.fixed_point(index)))
    print("ladder %s: %d iterations, %d fallbacks, |f - f*| = %.2e" % (nref.LADDERS[index], iterations, nref.fallbacks(kinds), error))
    assert error <= 1e-12


@pytest.mark.parametrize("index", range(len(nref.LADDERS)))
def test_golden_fixed_points_are_fixed_points(index):
    """One more long-double iteration leaves the stored f* within the tolerance it was solved to (and the two cheapest are
    solved again from f = 0)."""
    e, r, t = nref.ladder(*nref.LADDERS[index])
    star = nref.fixed_point(index)
    assert star.dtype == np.longdouble and star[0] == 0
    assert ref.iterate(e, r, t, star, np.longdouble)[1] <= 1e-14
    if index in (0, 4):
        assert np.array_equal(nref.compute_fixed_point(index), star)


def test_reference_falls_back_on_the_poorly_overlapping_ladder():
    kinds = nref.solved(6)[4]
    assert nref.fallbacks(kinds) >= 1
    for i, kind in enumerate(kinds):
        if kind == nref.WITHDRAWN:
            assert kinds[i - 1] == nref.NEWTON               # only a Newton step is withdrawn


def test_reference_long_double_agrees():
    e, r, t = nref.ladder(*nref.LADDERS[0])
    f64 = nref.solve(e, r, t)[0]
    f80 = nref.solve(e, r, t, dtype=np.longdouble)[0]
    assert f80.dtype == np.longdouble and np.max(np.abs(f80 - f64)) <= 1e-12


def test_reference_single_rung_and_limits():
    e = np.array([1.0, 2.0, np.nan])
    f, iterations, residual, gradient, _ = nref.solve(e, np.zeros(3, dtype=np.int32), [0.7])
    assert f.tolist() == [0.0] and iterations == 1 and residual == 0.0 and gradient == 0.0
    e, r, t = nref.ladder(*nref.LADDERS[0])
    f, iterations, residual, _, kinds = nref.solve(e, r, t, max_iter=3)
    assert iterations == 3 and residual > 1e-10 and kinds == [nref.SC, nref.SC, nref.NEWTON]
    with pytest.raises(ValueError):
        nref.solve(e, np.where(r == 3, 2, r), t)             # rung 3 left empty


def test_cholesky_solve_and_pivot_failure():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(9, 9))
    h = a @ a.T + 9 * np.eye(9)
    b = rng.normal(size=9)
    assert np.max(np.abs(nref.cholesky_solve(h, b) - np.linalg.solve(h, b))) <= 1e-12
    h[4, 4] = -1.0
    assert nref.cholesky_solve(h, b) is None
    h[4, 4] = np.nan
    assert nref.cholesky_solve(h, b) is None


def test_unknown_method_is_refused_before_anything_is_loaded(monkeypatch):
    from metropolisengine_amd import _capi, engine, statistics

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_capi, "load", no_load)
    e, r, t = nref.ladder(8, 16, 16, 1.3)
    with pytest.raises(ValueError, match="method"):
        statistics.mbar_free_energies(e, r, t, method="bogus")
    eng = object.__new__(engine.MetropolisEngine)            # no library, no handle: the check comes first
    with pytest.raises(ValueError, match="method"):
        eng.ladder_free_energies(method="bogus")
    assert statistics.MBAR_METHODS == ("self-consistent", "newton")


def test_new_symbols_are_declared_and_bound():
    from metropolisengine_amd import _capi, build
    with open(os.path.join(ROOT, "include", "metropolis_engine.h")) as fh:
        header = fh.read()
    for name, n_args in (("me_mbar_solve_newton", 10), ("me_mbar_solve_newton_samples", 15)):
        declaration = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert declaration, name
        assert len(declaration.group(1).split(",")) == n_args
        assert len(_capi.SYMBOLS[name][1]) == n_args
    assert "me_mbar_newton" in [unit for unit, _ in build.HOST_UNITS]
    assert os.path.exists(os.path.join(ROOT, "metropolisengine_amd", "csrc", "me_mbar_newton.hip"))
