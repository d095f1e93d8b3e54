"""The Newton solver for the ladder free energies on the GPU (csrc/me_mbar_newton.hip: S and W^T W in one pass on the matrix
cores, the Cholesky step in one wavefront) against the numpy restatement tests/mbar_newton_reference.py and against the
long-double self-consistent fixed point.  Every figure is printed before it is asserted (run with -s);
profiles/mbar_newton.txt holds the values measured on the MI355X.

Bounds.  |f - f*| <= 1e-11 against the long-double fixed point: 14 times the worst error of the float64 restatement on these
ladders (7.1e-13) and 20 times below the best the self-consistent solver reaches at tol = 1e-10 (2.3e-10), so a path that ran
the old iteration fails it.  The same 1e-11 against the float64 restatement where that is the yardstick (both are float64
Newton iterates from the same start whose last step is below 1e-10 and which converge quadratically)."""
import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_newton_reference as nref
import mbar_reference as ref

pytestmark = pytest.mark.gpu
TOL = 1e-10
F_BOUND = 1e-11
NEW_KEYS = {"gradient", "newton_steps", "fallback_steps"}
OLD_KEYS = {"f", "ln_z", "iterations", "residual", "converged", "n_samples"}


def newton(e, r, t, **kw):
    return statistics.mbar_free_energies(e, r, t, method="newton", **kw)


def check_against(out, reference, bound=F_BOUND):
    f, iterations, residual, gradient, kinds = reference
    error = np.max(np.abs(out["f"] - f))
    print("  %d iterations (reference %d), residual %.2e, gradient %.2e, %d Newton steps, %d fallbacks (reference %d), "
          "|f - reference| = %.2e" % (out["iterations"], iterations, out["residual"], out["gradient"], out["newton_steps"],
                                       out["fallback_steps"], nref.fallbacks(kinds), error))
    assert out["converged"] and out["residual"] <= TOL
    assert error <= bound
    assert abs(out["iterations"] - iterations) <= 2
    assert out["f"][0] == 0.0 and np.array_equal(out["ln_z"], -out["f"])
    return error


# ------------------------------------------------------------------------------------------------ 1. the seven ladders


@pytest.mark.parametrize("index", range(len(nref.LADDERS)))
def test_seven_ladders(index):
    k, per_rung = nref.LADDERS[index][:2]
    e, r, t = nref.ladder(*nref.LADDERS[index])
    out = newton(e, r, t, tol=TOL)
    reference = nref.solved(index)
    print("ladder %s" % (nref.LADDERS[index],))
    check_against(out, reference)
    error = np.max(np.abs(out["f"].astype(np.longdouble) - nref.fixed_point(index)))
    print("  |f - f*| = %.2e" % error)
    assert set(out) == OLD_KEYS | NEW_KEYS
    assert error <= F_BOUND
    assert out["iterations"] <= 20
    assert out["gradient"] <= 1e-6
    assert out["iterations"] == 2 + out["newton_steps"] + out["fallback_steps"]      # every pass is one of the three
    assert np.array_equal(out["n_samples"], np.full(k, per_rung)) and out["n_samples"].dtype == np.int64
    plain = statistics.mbar_free_energies(e, r, t, tol=TOL)
    print("  the self-consistent solver: %d iterations, |f - f*| = %.2e"
          % (plain["iterations"], np.max(np.abs(plain["f"].astype(np.longdouble) - nref.fixed_point(index)))))
    assert plain["converged"] and plain["iterations"] >= 5 * out["iterations"]


# ------------------------------------------------------------------------------------------------------------ 2. tails


def spanning_ladder(k, per_rung, seed=11):
    energies, temps = ref.gamma_ladder(per_rung, n_rungs=k, seed=seed, ratio=(1.3 ** 7) ** (1.0 / max(k - 1, 1)))
    return energies.ravel(), np.repeat(np.arange(k, dtype=np.int32), per_rung), temps


def test_unequal_rungs_no_multiple_of_anything():
    sizes = 37 + 11 * np.arange(8)
    assert sizes.sum() == 604
    temps = 0.5 * 1.3 ** np.arange(8)
    rng = np.random.default_rng(3)
    e = np.concatenate([rng.gamma(8.0, t, size=n) for t, n in zip(temps, sizes)])
    r = np.repeat(np.arange(8, dtype=np.int32), sizes)
    order = rng.permutation(e.size)                                # the rungs interleaved
    out = newton(e[order], r[order], temps)
    check_against(out, nref.solve(e[order], r[order], temps))
    assert np.array_equal(out["n_samples"], sizes)


def test_single_rung():
    out = newton(np.array([0.3, 1.5, np.nan, 2.0]), np.zeros(4, dtype=np.int32), [0.8])
    assert out["f"].tolist() == [0.0] and out["ln_z"].tolist() == [0.0] and out["iterations"] == 1 and out["converged"]
    assert out["residual"] == 0.0 and out["gradient"] == 0.0 and out["newton_steps"] == 0 and out["fallback_steps"] == 0
    assert out["n_samples"].tolist() == [3]


@pytest.mark.parametrize("k", [17, 33])
def test_one_column_in_the_next_tile(k):
    e, r, t = spanning_ladder(k, 64)
    out = newton(e, r, t)
    check_against(out, nref.solve(e, r, t))
    assert np.array_equal(out["n_samples"], np.full(k, 64))


# --------------------------------------------------------------------------------------------- 3. more tiles than blocks


def test_tile_loop_wraps():
    n = 2048 * 2048 + 3 * 2048 + 5
    temps = 0.5 * 1.3 ** np.arange(8)
    rng = np.random.default_rng(5)
    r = (np.arange(n) % 8).astype(np.int32)
    e = rng.gamma(8.0, 1.0, size=n) * temps[r]
    out = newton(e, r, temps)
    check_against(out, nref.solve(e, r, temps))
    assert out["n_samples"].sum() == n


# ------------------------------------------------------------------------------------------------ 4. non-finite energies


def test_non_finite_energies_are_skipped():
    e, r, t = nref.ladder(*nref.LADDERS[0])
    rng = np.random.default_rng(9)
    holes = np.sort(rng.choice(e.size, size=e.size // 10, replace=False))
    holes = np.union1d(holes, np.arange(8) * 512 + 5)               # every rung has at least one
    bad = e.copy()
    bad[holes] = np.resize(np.array([np.nan, np.inf, -np.inf]), holes.size)
    keep = np.ones(e.size, dtype=bool)
    keep[holes] = False
    out = newton(bad, r, t)
    clean = newton(e[keep], r[keep], t)
    error = np.max(np.abs(out["f"] - clean["f"]))
    print("  %d of %d samples not finite; |f - f without them| = %.2e" % (holes.size, e.size, error))
    assert np.array_equal(out["n_samples"], np.bincount(r[keep], minlength=8))
    assert out["converged"] and clean["converged"]
    assert error <= 1e-12
    bad[r == 3] = np.nan
    with pytest.raises(_capi.MetropolisLibraryError, match="rung 3"):
        newton(bad, r, t)
    with pytest.raises(_capi.MetropolisLibraryError, match="rung 3"):
        statistics.mbar_free_energies(bad, r, t)                    # as today


# ---------------------------------------------------------------------------------------------- 5. bitwise reproducible


def same_bits(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def test_bitwise_reproducible_and_engine_form():
    k, m, records = 16, 64, 4                                      # (an engine's rung is a run of whole 64-chain tiles)
    energies, temps = ref.gamma_ladder(m * records, n_rungs=k, dim=64, seed=11, ratio=1.35)
    samples = energies.reshape(k, records, m).transpose(1, 0, 2).reshape(records, k * m)      # column c in rung c // m
    rungs = np.tile(np.repeat(np.arange(k, dtype=np.int32), m), records)
    first = newton(samples.ravel(), rungs, temps)
    second = newton(samples.ravel(), rungs, temps)
    same_bits(first, second)
    assert first["converged"] and first["fallback_steps"] >= 1    # (the ladder whose Newton steps get withdrawn)
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=k * m, seed=5, dtype="f64", temperatures=temps)
    eng.record_energies(records)
    eng.set_energy_samples(samples)
    same_bits(eng.ladder_free_energies(method="newton"), first)
    same_bits(eng.ladder_free_energies(method="newton"), first)


# ------------------------------------------------------------------------------------------------------------ 6. limits


def test_iteration_limits():
    e, r, t = nref.ladder(*nref.LADDERS[0])
    out = newton(e, r, t, max_iter=3)
    f, iterations, residual, _, kinds = nref.solve(e, r, t, max_iter=3)
    assert out["iterations"] == 3 and not out["converged"] and out["residual"] > TOL
    assert out["newton_steps"] == 1 and out["fallback_steps"] == 0
    assert np.max(np.abs(out["f"] - f)) <= F_BOUND and abs(out["residual"] - residual) <= F_BOUND
    loose = newton(e, r, t, tol=1e-3)
    f, iterations, residual, _, _ = nref.solve(e, r, t, tol=1e-3)
    print("  tol 1e-3: %d iterations (reference %d), residual %.2e (reference %.2e)"
          % (loose["iterations"], iterations, loose["residual"], residual))
    assert loose["converged"] and loose["iterations"] == iterations < 16          # the first iterate that met it, not the batch's last
    assert loose["residual"] <= 1e-3 and abs(loose["residual"] - residual) <= F_BOUND
    assert np.max(np.abs(loose["f"] - f)) <= F_BOUND
    with pytest.raises(ValueError):
        newton(e, r, t, tol=0.0)
    with pytest.raises(ValueError):
        newton(e, r, t, max_iter=0)


# ------------------------------------------------------------------------------------------------------ 7. default path


def test_default_method_is_unchanged():
    e, r, t = nref.ladder(*nref.LADDERS[0])
    default = statistics.mbar_free_energies(e, r, t)
    explicit = statistics.mbar_free_energies(e, r, t, method="self-consistent")
    same_bits(default, explicit)
    assert set(default) == OLD_KEYS
    f, iterations, residual, _ = ref.solve(e, r, t)
    assert default["iterations"] == iterations and np.max(np.abs(default["f"] - f)) <= 1e-8
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=8 * 64, seed=5, dtype="f64", temperatures=t)
    eng.record_energies(8)
    eng.set_energy_samples(e.reshape(8, 8, 64).transpose(1, 0, 2).reshape(8, 512))
    same_bits(eng.ladder_free_energies(), eng.ladder_free_energies(method="self-consistent"))
    assert set(eng.ladder_free_energies()) == OLD_KEYS
    with pytest.raises(ValueError, match="method"):
        eng.ladder_free_energies(method="bogus")
