"""Energy samples, MBAR free energies and temperature reweighting on the GPU (csrc/me_mbar.hip) against the numpy
restatement in tests/mbar_reference.py and against exact results.  Every figure is printed before it is asserted (run with
-s); profiles/mbar_solve.txt holds the values measured on the MI355X."""
import importlib.util
import os

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref

pytestmark = pytest.mark.gpu
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
DIM = 16
TOL = 1e-10
F_BOUND = 1e-8          # the project's bound for float64 quantities that pass through iterated arithmetic
LADDER8 = 0.5 * 1.3 ** np.arange(8)
# Relative errors of energy_var and neff_fraction against the long-double reference as measured on the MI355X
# (profiles/mbar_solve.txt); the tests assert ten times these, capped at 1e-8.
MEASURED_VAR_ERROR = 5.4e-16
MEASURED_NEFF_ERROR = 3.5e-16
N_SUBSETS = 16


def _ladder_engine(temps, m, dtype="f64", spec=None, real0=(0.1,), cplx0=None, **kw):
    spec = me.IsoQuadratic(1.0) if spec is None else spec
    return me.MetropolisEngine(spec, None, list(real0) if real0 else None, cplx0, n_chains=m * len(temps), seed=5, dtype=dtype,
                               temperatures=temps, **kw)


def _rungs(k, m, records):
    return np.tile(np.repeat(np.arange(k), m), records)


def _synthetic(k, m, records, seed=17):
    """Gamma samples of the D = 16 quadratic form laid out as a store: ``(records, k * m)``, column c in rung c // m.  The
    ladder spans 0.5 ... 0.5 1.3^7 geometrically for every k (k = 8: 0.5 1.3^j): neighbouring rungs of a longer ladder overlap
    more, and the self-consistent iteration converges in about the same number of iterations."""
    temps = 0.5 * (1.3 ** 7) ** (np.arange(k) / (k - 1.0))
    rng = np.random.default_rng(seed)
    samples = np.stack([np.concatenate([rng.gamma(DIM / 2.0, t, size=m) for t in temps]) for _ in range(records)])
    return temps, samples


def _loaded_engine(k, m, records, seed=17):
    temps, samples = _synthetic(k, m, records, seed)
    eng = _ladder_engine(temps, m)
    eng.record_energies(records)
    eng.set_energy_samples(samples)
    return eng, temps, samples


# ------------------------------------------------------------------------------------------------------ 1. the store


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_records_are_the_chain_energies_in_order(dtype):
    eng = _ladder_engine(LADDER8, 64, dtype, real0=[0.1] * 4)
    assert eng.n_energy_records == 0
    with pytest.raises(Exception):
        eng.record_energy()                              # never enabled
    eng.record_energies(3)
    rows = []
    for _ in range(3):
        eng.step_all(4)
        eng.record_energy()
        rows.append(np.array(eng.energy_total))
        got = eng.energy_samples()
        assert got.shape == (len(rows), eng.n_chains) and got.dtype == np.float64
        assert np.array_equal(got[-1], rows[-1])         # bit for bit
    assert np.array_equal(eng.energy_samples(), np.array(rows))        # rows keep their order
    assert eng.n_energy_records == 3
    with pytest.raises(Exception):
        eng.record_energy()                              # full
    assert eng.n_energy_records == 3
    eng.record_energies(2)                               # a new store forgets the records
    assert eng.n_energy_records == 0 and eng.energy_samples().shape == (0, eng.n_chains)
    eng.record_energies(0)
    with pytest.raises(Exception):
        eng.record_energy()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_term_dictionary_rows_are_summed_in_row_order_in_the_device_dtype(dtype):
    eng = me.MetropolisEngine(me.LandauToy(1.0, -1.0, 0.5, terms=True), None, [0.3, 0.2], [0.4 + 0.1j], n_chains=256, seed=9,
                              dtype=dtype, temp=0.7)
    eng.record_energies(1)
    eng.step_all(20)
    eng.record_energy()
    ledger = eng._get(_capi.FIELD_ENERGY).astype(np.float32 if dtype == "f32" else np.float64)
    assert ledger.shape[1] > 1
    total = ledger[:, 0].copy()
    for t in range(1, ledger.shape[1]):
        total = total + ledger[:, t]
    assert np.array_equal(eng.energy_samples()[0], total.astype(np.float64))


def test_set_round_trips_and_a_new_ladder_clears_the_count():
    eng = _ladder_engine(LADDER8, 64)
    eng.record_energies(4)
    samples = np.random.default_rng(1).standard_normal((3, eng.n_chains))
    samples[1, 5], samples[2, 7] = np.inf, np.nan
    eng.set_energy_samples(samples)
    assert eng.n_energy_records == 3
    assert np.array_equal(eng.energy_samples(), samples, equal_nan=True)
    assert np.array_equal(np.signbit(eng.energy_samples()), np.signbit(samples))
    with pytest.raises(ValueError):
        eng.set_energy_samples(np.zeros((5, eng.n_chains)))              # beyond the capacity
    with pytest.raises(ValueError):
        eng.set_energy_samples(np.zeros((2, eng.n_chains - 1)))
    eng.record_energy()                                                   # appends after the rows that were set
    assert eng.n_energy_records == 4
    eng.set_temperatures(LADDER8 * 1.5)
    assert eng.n_energy_records == 0
    eng.record_energy()
    assert eng.n_energy_records == 1


def test_stores_work_without_a_ladder_and_not_with_reference_ledgers():
    plain = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.2], None, n_chains=128, temp=1.0)
    plain.record_energies(1)
    plain.record_energy()
    assert np.array_equal(plain.energy_samples()[0], plain.energy_total)
    with pytest.raises(Exception):
        plain.ladder_free_energies()                     # no ladder
    ladder = _ladder_engine(LADDER8, 64)
    with pytest.raises(Exception):
        ladder.ladder_free_energies()                    # no records
    ledgers = me.MetropolisEngine(me.LandauToy(), None, [0.0, 0.0], [0j], n_chains=128, reference_energy_ledgers=True)
    with pytest.raises(NotImplementedError, match="LEDGERS"):
        ledgers.record_energies(4)


# ------------------------------------------------------------------------------------- 2. the solver against the reference


@pytest.mark.parametrize("k, m, records", [(8, 4096, 8), (33, 64, 64)])
def test_solver_matches_the_reference(k, m, records):
    eng, temps, samples = _loaded_engine(k, m, records)
    rungs = _rungs(k, m, records)
    out = eng.ladder_free_energies(tol=TOL)
    f_ref, it_ref, _, counts = ref.solve(samples, rungs, temps, tol=TOL)
    f_tight, it_tight, _, _ = ref.solve(samples, rungs, temps, tol=1e-13)
    f_next, moved = ref.iterate(samples, rungs, temps, out["f"], dtype=np.longdouble)
    err = float(np.max(np.abs(out["f"] - f_tight)))
    print("K=%d: iterations device %d reference %d (tol 1e-13: %d); residual %.3e; one long-double iteration moves f by "
          "%.3e; max |f_device - f_reference(1e-13)| = %.3e" % (k, out["iterations"], it_ref, it_tight, out["residual"],
                                                             float(moved), err))
    assert out["converged"] and out["residual"] <= TOL
    assert np.array_equal(out["n_samples"], counts) and np.all(counts == m * records)
    assert abs(out["iterations"] - it_ref) <= 2
    assert float(moved) <= 2 * TOL
    assert err <= F_BOUND
    assert out["f"][0] == 0.0 and np.array_equal(out["ln_z"], -out["f"])


def test_iteration_limit_is_honoured():
    eng, _, _ = _loaded_engine(8, 256, 4)
    out = eng.ladder_free_energies(tol=1e-14, max_iter=5)
    assert out["iterations"] == 5 and not out["converged"] and out["residual"] > 1e-14
    out = eng.ladder_free_energies(tol=1e-3, max_iter=40)      # stops inside a batch of launches, at the first iterate that meets it
    assert out["converged"] and out["iterations"] < 40 and out["residual"] <= 1e-3


# ---------------------------------------------------------------------------------------------- 3. bitwise reproducible


def test_two_solves_are_bitwise_equal():
    eng, temps, _ = _loaded_engine(8, 4096, 8)
    a, b = eng.ladder_free_energies(), eng.ladder_free_energies()
    assert np.array_equal(a["f"], b["f"]) and a["residual"] == b["residual"] and a["iterations"] == b["iterations"]
    targets = np.concatenate([temps, 0.5 * (temps[:-1] + temps[1:])])
    ra, rb = eng.reweight(targets, a["f"]), eng.reweight(targets, b["f"])
    for key in ("ln_z", "energy_mean", "energy_var", "heat_capacity", "neff_fraction"):
        assert np.array_equal(ra[key], rb[key]), key


# ------------------------------------------------------------------------------------------------ 4. non-finite energies


def test_non_finite_energies_are_skipped_and_counted():
    k, m, records = 8, 1024, 4
    temps, samples = _synthetic(k, m, records, seed=23)
    dirty = samples.copy()
    dirty[0, :3] = np.inf                 # rung 0
    dirty[1, 2 * m + 5] = np.nan          # rung 2
    dirty[3, 7 * m:7 * m + 10] = -np.inf  # rung 7
    eng = _ladder_engine(temps, m)
    eng.record_energies(records)
    eng.set_energy_samples(dirty)
    out = eng.ladder_free_energies()
    expect = np.full(k, m * records)
    expect[[0, 2, 7]] -= [3, 1, 10]
    assert np.array_equal(out["n_samples"], expect)
    rungs = _rungs(k, m, records)
    f_tight, _, _, counts = ref.solve(dirty, rungs, temps, tol=1e-13)
    err = float(np.max(np.abs(out["f"] - f_tight)))
    print("with non-finite energies: max |f_device - f_reference(1e-13)| = %.3e" % err)
    assert np.array_equal(counts, expect) and out["converged"] and err <= F_BOUND
    rw = eng.reweight([0.9], out["f"])
    expect_rw = ref.reweight(dirty, rungs, temps, out["f"], [0.9], dtype=np.longdouble)
    assert abs(rw["ln_z"][0] - float(expect_rw[0, 0])) <= 1e-9 * abs(float(expect_rw[0, 0]))
    dirty[:, 4 * m:5 * m] = np.nan        # rung 4 has nothing left
    eng.set_energy_samples(dirty)
    with pytest.raises(Exception, match="rung 4"):
        eng.ladder_free_energies()
    with pytest.raises(Exception, match="rung 4"):
        eng.reweight([1.0], out["f"])


# ------------------------------------------------------------------------------------------------------- 5. reweighting


@pytest.mark.parametrize("k, m, records", [(8, 4096, 8), (33, 64, 64)])
def test_reweighting_matches_the_long_double_reference(k, m, records):
    eng, temps, samples = _loaded_engine(k, m, records)
    rungs = _rungs(k, m, records)
    f = eng.ladder_free_energies()["f"]
    # 9 temperatures: five rungs and four points between rungs.  T_0 is not among them: ln Z(T_0) / Z(T_0) is 0 by the
    # normalisation f_0 = 0 and comes out as the stopping error (1e-11), a difference of two numbers of order 10, so a relative
    # bound means nothing there; it is held to an absolute bound below instead.
    targets = np.array([temps[1], 0.57, temps[k // 4], 0.8, temps[k // 2], 1.5, temps[3 * k // 4], 2.6, temps[-1]])
    got = eng.reweight(targets, f)
    want = ref.reweight(samples, rungs, temps, f, targets, dtype=np.longdouble)
    rel = {}
    for row, key in enumerate(("ln_z", "energy_mean", "energy_var", "neff_fraction")):
        w = want[row].astype(np.float64)
        scale = np.where(w != 0, np.abs(w), 1.0)
        rel[key] = float(np.max(np.abs((got[key].astype(np.longdouble) - want[row]).astype(np.float64)) / scale))
    print("K=%d reweighting, largest relative error against long double: %s" % (k, rel))
    assert np.array_equal(got["heat_capacity"], got["energy_var"] / targets ** 2)
    assert np.all((got["neff_fraction"] > 0) & (got["neff_fraction"] <= 1))
    assert rel["ln_z"] <= 1e-9 and rel["energy_mean"] <= 1e-9
    assert rel["energy_var"] <= min(10 * MEASURED_VAR_ERROR, 1e-8)
    assert rel["neff_fraction"] <= min(10 * MEASURED_NEFF_ERROR, 1e-8)
    # at T_0: |ln_z| is the stopping error; device and reference differ by the rounding of M + ln W, |M| of order 10
    at_t0 = eng.reweight([temps[0]], f)["ln_z"][0]
    want_t0 = float(ref.reweight(samples, rungs, temps, f, [temps[0]], dtype=np.longdouble)[0, 0])
    print("K=%d: ln_z(T_0) device %.3e reference %.3e" % (k, at_t0, want_t0))
    assert abs(at_t0) <= 2 * TOL and abs(at_t0 - want_t0) <= 1e-13
    # the fixed-point identity on the device: reweighting to a rung gives -f
    at_rungs = eng.reweight(temps, f)
    print("K=%d: max |ln_z(T_k) + f_k| = %.3e" % (k, np.max(np.abs(at_rungs["ln_z"] + f))))
    assert np.max(np.abs(at_rungs["ln_z"] + f)) <= 2 * TOL


def test_more_targets_than_one_pass_holds():
    eng, temps, _ = _loaded_engine(8, 256, 4)
    f = eng.ladder_free_energies()["f"]
    grid = np.geomspace(temps[0], temps[-1], 19)
    whole = eng.reweight(grid, f)
    for i in (0, 7, 8, 18):
        one = eng.reweight([grid[i]], f)
        for key in ("ln_z", "energy_mean", "energy_var", "neff_fraction"):
            assert one[key][0] == whole[key][i], (key, i)


# --------------------------------------------------------------------------------------------------- 6. engine-less form


def test_engine_less_form_equals_the_engine_bit_for_bit():
    eng, temps, _ = _loaded_engine(8, 1024, 4)
    m = eng.n_chains // temps.size
    samples = eng.energy_samples()
    rungs = np.broadcast_to(np.arange(eng.n_chains) // m, samples.shape)
    a = eng.ladder_free_energies()
    b = statistics.mbar_free_energies(samples, rungs, temps)
    assert np.array_equal(a["f"], b["f"]) and a["residual"] == b["residual"] and a["iterations"] == b["iterations"]
    assert np.array_equal(a["n_samples"], b["n_samples"]) and a["converged"] == b["converged"]
    targets = [0.6, 1.0, temps[4]]
    ra, rb = eng.reweight(targets, a["f"]), statistics.mbar_reweight(samples, rungs, temps, b["f"], targets)
    for key in ra:
        assert np.array_equal(ra[key], rb[key]), key
    with pytest.raises(Exception, match="rung 3"):
        statistics.mbar_free_energies(samples[rungs != 3], rungs[rungs != 3], temps)


# -------------------------------------------------------------------------------------------------------- 7. end to end


def _burn_in(eng, rounds, sweeps=5):
    """``rounds`` x (step_all + replica_exchange); returns the rung means of the widths after 9/10 of them and at the end."""
    k = eng.temperatures.size
    early = None
    for r in range(rounds):
        eng.step_all(sweeps)
        eng.replica_exchange()
        if r + 1 == rounds - rounds // 10:
            early = np.asarray(eng.sampling_width).reshape(k, -1).mean(axis=1)
    return early, np.asarray(eng.sampling_width).reshape(k, -1).mean(axis=1)


def _record(eng, n_records=64, sweeps=5, rounds_per_record=2):
    eng.record_energies(n_records)
    for _ in range(n_records):
        for _ in range(rounds_per_record):
            eng.step_all(sweeps)
            eng.replica_exchange()
        eng.record_energy()


def _subset_estimates(eng, targets):
    """MBAR per independent sub-ensemble (slots j mod 16): ``(ln_z at the rungs, heat capacity at targets)``."""
    temps = eng.temperatures
    m = eng.n_chains // temps.size
    energies = eng.energy_samples().reshape(-1, temps.size, m)
    ln_z, heat = [], []
    for s in range(N_SUBSETS):
        sub = energies[:, :, s::N_SUBSETS]
        rungs = np.broadcast_to(np.arange(temps.size)[None, :, None], sub.shape)
        out = statistics.mbar_free_energies(sub, rungs, temps)
        assert out["converged"]
        ln_z.append(out["ln_z"])
        heat.append(statistics.mbar_reweight(sub, rungs, temps, out["f"], targets)["heat_capacity"])
    return np.array(ln_z), np.array(heat)


BURN_IN_ROUNDS = 600


def _check(name, estimates, exact):
    ok, mean, se = ref.within_5_se(estimates, exact)
    print(name, "mean", mean, "exact", np.asarray(exact), "se", se, "deviation / se",
          np.abs(mean - exact) / np.where(se > 0, se, 1.0))
    assert np.all(ok), name


def test_quadratic_ladder_end_to_end():
    """IsoQuadratic(1.0) in 16 real dimensions on T_k = 0.5 1.3^k: ln Z(T_k)/Z(T_0) = 8 ln(T_k/T_0) and C = 8, from 64
    records 10 sweeps apart after a burn-in of BURN_IN_ROUNDS = 600 rounds of (5 sweeps + one swap round), by which the
    rung means of the Robbins-Monro widths change by less than 1 % over the last tenth.

    Measured on the MI355X (profiles/mbar_solve.txt): the estimates sit 1.8 to 2.3 standard errors ABOVE the exact values at
    every rung, a common relative excess of 0.13 % that the heat capacity shows too (8.02, 8.006, 8.016).  The solver
    reproduces exact Gamma samples within 0.6 standard errors (tests/test_mbar_cpu.py), so the excess belongs to the
    sampler: its width adaptation keeps a constant gain of 1/200 per step, which leaves the chain slightly off its target
    distribution."""
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * DIM, None, n_chains=8 * 4096, seed=41, dtype="f64",
                              temperatures=LADDER8)
    early, late = _burn_in(eng, BURN_IN_ROUNDS)
    print("rung means of the widths at 9/10 of the burn-in", early, "and at its end", late, "relative change",
          np.abs(late / early - 1))
    assert np.all(np.abs(late / early - 1) < 0.01)
    _record(eng)
    targets = np.array([0.6, 1.0, 2.2])
    ln_z, heat = _subset_estimates(eng, targets)
    _check("ln_z", ln_z, DIM / 2.0 * np.log(LADDER8 / LADDER8[0]))
    _check("heat_capacity", heat, np.full(3, DIM / 2.0))


def _load_example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(EXAMPLES, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_double_well_ladder_end_to_end():
    """The same protocol on the double well E = 4 (x^2 - 1)^2 of the parallel-tempering example (ladder 0.1 1.8^k) against a
    quadrature of Z(T); BURN_IN_ROUNDS = 600 rounds of burn-in as above."""
    demo = _load_example("demo_ladder_free_energy")
    temps = demo.LADDER
    eng = me.MetropolisEngine(demo.double_well, None, [-1.0], None, n_chains=8 * 4096, seed=43, temperatures=temps, dtype="f64")
    early, late = _burn_in(eng, BURN_IN_ROUNDS)
    print("rung means of the widths at 9/10 of the burn-in", early, "and at its end", late)
    assert np.all(np.abs(late / early - 1) < 0.01)
    _record(eng)
    targets = np.array([0.15, 0.7, 2.0])
    ln_z, heat = _subset_estimates(eng, targets)
    quad_rungs, quad_targets = demo.quadrature(temps), demo.quadrature(targets)
    _check("ln_z", ln_z, quad_rungs[0] - quad_rungs[0, 0])
    _check("heat_capacity", heat, quad_targets[2] / targets ** 2)


# -------------------------------------------------------------------------------------------------------- 8. the example


def test_ladder_free_energy_demo(capsys):
    out = _load_example("demo_ladder_free_energy").main()
    text = capsys.readouterr().out
    print(text)
    assert "quadrature" in text and len(text.strip().splitlines()) == 1 + out["temps"].size
    _check("demo ln_z", out["ln_z"], out["exact_ln_z"])
    _check("demo heat_capacity", out["heat_capacity"], out["exact_heat_capacity"])
