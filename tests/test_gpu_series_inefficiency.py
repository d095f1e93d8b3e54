"""Statistical inefficiencies of the recorded series on the GPU (csrc/me_series.hip) against the long-double reference of
tests/series_reference.py.  Every figure is printed before it is asserted (run with -s); profiles/mbar_inefficiency.txt holds
the values measured on the MI355X.

The stop lags are demanded exactly: tests/test_series_reference_cpu.py shows that no C(t) the walks of these inputs meet is
closer to 0 than 3.6e-4."""
import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import statistics
import mbar_uncertainty_reference as u
import series_reference as sref

pytestmark = pytest.mark.gpu
F_BOUND = 1e-8          # the project's bound for float64 quantities that pass through iterated arithmetic
# Largest errors against the long-double reference over the five shapes of test 1 as measured on the MI355X
# (profiles/mbar_inefficiency.txt): of an acf entry (absolute) and of g, mean and var (relative).  The tests assert ten times
# these, capped at 1e-8.
MEASURED_ACF_ERROR = 2.7e-16
MEASURED_REL_ERROR = 4.9e-14        # (of a mean: the means of these zero-mean series are sums that nearly cancel)
BOUND_ACF = min(10 * MEASURED_ACF_ERROR, F_BOUND)
BOUND_REL = min(10 * MEASURED_REL_ERROR, F_BOUND)
FLOAT_KEYS = ("g", "tau", "mean", "var", "acf")
KEYS = FLOAT_KEYS + ("stop_lag", "chains_used")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _bitwise(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same(a, b):
    """Two result dictionaries, bit for bit."""
    assert a.keys() == b.keys()
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].shape == b[key].shape and _bitwise(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


def _errors(got, want):
    """``(acf error, relative error)`` of the (groups,)-shaped entries of ``got`` against the reference dictionary ``want``;
    asserts what has to be exact: stop lags, chains used and where the acf is NaN."""
    assert np.array_equal(got["stop_lag"], want["stop_lag"]), (got["stop_lag"], want["stop_lag"])
    assert np.array_equal(got["chains_used"], want["chains_used"])
    ref_acf = np.asarray(want["acf"], dtype=np.longdouble)
    assert np.array_equal(np.isnan(got["acf"]), np.isnan(ref_acf.astype(np.float64)))
    seen = ~np.isnan(got["acf"])
    acf = float(np.max(np.abs(got["acf"].astype(np.longdouble)[seen] - ref_acf[seen]))) if seen.any() else 0.0
    rel = 0.0
    for key in ("g", "mean", "var"):
        w = np.asarray(want[key], dtype=np.longdouble)
        ok = ~np.isnan(w.astype(np.float64))
        assert np.array_equal(np.isnan(got[key]), ~ok), key
        if ok.any():
            rel = max(rel, float(np.max(np.abs(got[key].astype(np.longdouble)[ok] - w[ok]) / np.abs(w[ok]))))
    return acf, rel


# ---- 1. the host form against the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sref.SHAPES, ids=lambda s: "R%d-K%d-M%d" % s)
def test_host_form_against_the_reference(shape):
    r, k, m = shape
    x = sref.shape_series(r, k, m)
    got = statistics.series_inefficiency(x, group_chains=m)
    assert got["g"].shape == (1, k) and got["acf"].shape == (1, k, r - 1) and got["n_records"] == r
    assert got["stop_lag"].dtype == np.int32 and got["chains_used"].dtype == np.int64
    want = sref.grouped_inefficiency(x, m)
    acf, rel = _errors({key: got[key][0] for key in KEYS}, want)
    print("(R, K, M) = %s: stop lags %s; largest acf error %.3e (bound %.1e), largest relative error of g, mean, var %.3e "
          "(bound %.1e)" % (shape, list(got["stop_lag"][0]), acf, BOUND_ACF, rel, BOUND_REL))
    assert np.all(got["chains_used"] == m) and _bitwise(got["tau"], (got["g"] - 1.0) / 2.0)
    assert acf <= BOUND_ACF and rel <= BOUND_REL


def test_host_form_refuses_bad_arguments():
    x = sref.shape_series(18, 3, 192)
    for kwargs in ({"group_chains": 96}, {"group_chains": 128}, {"group_chains": 0}, {"mintime": -1}, {"max_lag": 0}, {"max_lag": 17}):
        with pytest.raises(ValueError):
            statistics.series_inefficiency(x, **kwargs)
    with pytest.raises(ValueError):
        statistics.series_inefficiency(x[:2])
    one = statistics.series_inefficiency(x)         # None: one group of all 576 series
    assert one["g"].shape == (1, 1) and one["chains_used"][0, 0] == 576


# ---- 2. the engine's stores ---------------------------------------------------------------------------------------------
STORE = (40, 4, 128, 3)       # R, K, M, Q


def _store_engine(energies, columns, k, which=None):
    records, n = energies.shape
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=n, seed=5, dtype="f64",
                              temperatures=u.CAL_TEMPS[:k] if k == 4 else None)
    eng.record_energies(records)
    eng.set_energy_samples(energies)
    if columns is not None:
        eng.record_observables(list(range(columns.shape[1])) if which is None else which)
        eng.set_energy_samples(energies)
        eng.set_observable_samples(columns)
    return eng


@pytest.fixture(scope="module")
def store():
    """``(engine, data (R, 1 + Q, K M))``: AR(1) series of a generator of their own in every column; column 0 is the energy."""
    r, k, m, q = STORE
    data = np.stack([sref.shape_series(r, k, m, seed=sref.SEED + 1 + j) for j in range(1 + q)], axis=1)
    return _store_engine(data[:, 0].copy(), data[:, 1:].copy(), k), data


def _by_column(data, m, **kwargs):
    return [statistics.series_inefficiency(data[:, j].copy(), group_chains=m, **kwargs) for j in range(data.shape[1])]


def test_engine_stores_equal_the_host_form_bit_for_bit(store):
    eng, data = store
    r, k, m, q = STORE
    got = eng.recorded_inefficiency()
    assert got["names"] == ("energy",) + eng.recorded_observables and len(got["names"]) == 1 + q
    assert got["g"].shape == (1 + q, k) and got["acf"].shape == (1 + q, k, r - 1) and got["n_records"] == r
    for j, want in enumerate(_by_column(data, m)):
        for key in KEYS:
            assert _bitwise(got[key][j], want[key][0]), (j, key)
    assert np.all(np.isfinite(got["g"])) and np.all(got["g"] >= 1.0)


def test_engine_without_a_ladder_is_one_group():
    x = sref.shape_series(20, 1, 256)
    eng = _store_engine(x, None, 1)
    assert eng.temperatures is None
    got = eng.recorded_inefficiency()
    assert got["names"] == ("energy",) and got["g"].shape == (1, 1) and got["acf"].shape == (1, 1, 19)
    want = statistics.series_inefficiency(x)
    for key in KEYS:
        assert _bitwise(got[key], want[key]), key
    assert got["chains_used"][0, 0] == 256
    # too few records, no store
    eng.set_energy_samples(x[:2])
    with pytest.raises(Exception, match="3 records"):
        eng.recorded_inefficiency()
    eng.record_energies(0)
    with pytest.raises(Exception, match="no recorded energy samples"):
        eng.recorded_inefficiency()


def test_engine_refuses_bad_lags(store):
    eng = store[0]
    for kwargs in ({"mintime": -1}, {"max_lag": 0}, {"max_lag": 39}, {"max_lag": 2.5}):
        with pytest.raises(ValueError):
            eng.recorded_inefficiency(**kwargs)


# ---- 3. non-finite and degenerate input ---------------------------------------------------------------------------------
def test_non_finite_and_degenerate_input(store):
    eng, data = store
    r, k, m, q = STORE
    clean = eng.recorded_inefficiency()
    bad = data.copy()
    bad[7, 0, 1 * m + 5] = np.nan            # the energy, rung 1, chain 5
    bad[0, 3, 3 * m + 100] = np.inf          # column 3, rung 3, chain 100
    bad[:, 2, 2 * m:3 * m] = np.nan          # column 2, rung 2: every chain
    bad[3, 2, 2 * m + 9] = -np.inf
    bad[:, 1] = 2.5                          # column 1: constant
    other = _store_engine(bad[:, 0].copy(), bad[:, 1:].copy(), k)
    got = other.recorded_inefficiency()
    touched = {(0, 1): 1 * m + 5, (3, 3): 3 * m + 100}
    for (j, rung), chain in touched.items():
        assert got["chains_used"][j, rung] == m - 1
        keep = [c for c in range(rung * m, (rung + 1) * m) if c != chain]
        want = sref.grouped_inefficiency(data[:, j][:, keep], m - 1)
        acf, rel = _errors({key: got[key][j, rung:rung + 1] for key in KEYS}, want)
        print("column %d rung %d without chain %d: acf error %.3e, relative error %.3e" % (j, rung, chain, acf, rel))
        assert acf <= BOUND_ACF and rel <= BOUND_REL
    # a rung without a used chain, a column without variance
    assert got["chains_used"][2, 2] == 0 and got["stop_lag"][2, 2] == 0
    assert all(np.isnan(got[key][2, 2]).all() for key in FLOAT_KEYS)
    assert np.all(got["var"][1] == 0.0) and np.all(got["mean"][1] == 2.5) and np.all(np.isnan(got["g"][1]))
    assert np.all(got["chains_used"][1] == m) and np.all(got["stop_lag"][1] == 0) and np.all(np.isnan(got["acf"][1]))
    # every other (column, rung) is unchanged bit for bit
    for j in range(1 + q):
        for rung in range(k):
            if j == 1 or (j, rung) in touched or (j, rung) == (2, 2):
                continue
            for key in KEYS:
                assert _bitwise(got[key][j, rung], clean[key][j, rung]), (j, rung, key)


# ---- 4. order and reproducibility ---------------------------------------------------------------------------------------
def test_reproducible_prefix_and_offset():
    r, k, m = sref.SHAPES[-1]
    x = sref.shape_series(r, k, m)
    full = statistics.series_inefficiency(x, group_chains=m)
    _same(full, statistics.series_inefficiency(x, group_chains=m))
    # max_lag = 70: the bitwise prefix; the walks that went further are clipped to 71
    short = statistics.series_inefficiency(x, group_chains=m, max_lag=70)
    assert short["acf"].shape == (1, k, 71) and _bitwise(short["acf"], full["acf"][:, :, :71])
    assert np.array_equal(short["stop_lag"], np.minimum(full["stop_lag"], 71)) and list(short["stop_lag"][0]) == [12, 18, 39, 71, 71]
    early = full["stop_lag"] <= 70
    assert _bitwise(short["g"][early], full["g"][early]) and np.all(short["g"][~early] < full["g"][~early])
    for key in ("mean", "var", "chains_used"):
        assert _bitwise(short[key], full[key])
    # A common offset of 1e6.  The values are first rounded to multiples of 2^-30, so that adding 1e6 (< 2^20) is exact in float64
    # and the comparison sees the arithmetic of the kernels alone (the two-pass centring), not the rounding of the test's input.
    xq = np.round(x * 2.0 ** 30) / 2.0 ** 30
    assert np.array_equal((xq + 1e6) - 1e6, xq)
    base, moved = statistics.series_inefficiency(xq, group_chains=m), statistics.series_inefficiency(xq + 1e6, group_chains=m)
    acf = float(np.nanmax(np.abs(moved["acf"] - base["acf"])))
    rel = float(np.max(np.abs(moved["g"] - base["g"]) / base["g"]))
    print("offset 1e6: acf moves by %.3e (bound %.1e), g by %.3e relative (bound %.1e)" % (acf, BOUND_ACF, rel, BOUND_REL))
    assert np.array_equal(moved["stop_lag"], base["stop_lag"]) and np.array_equal(np.isnan(moved["acf"]), np.isnan(base["acf"]))
    assert acf <= BOUND_ACF and rel <= BOUND_REL
    assert np.max(np.abs(moved["mean"] - 1e6 - base["mean"])) <= 1e6 * 2.0 ** -52


# ---- 5. "recorded" in the uncertainty methods ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder():
    """An engine with the first calibration replica's energies (Gamma(2, T) on CAL_TEMPS, correlated) and two recorded columns:
    one more correlated than the energy, one less."""
    e = sref.calibration_energies()[0]
    r, n = e.shape
    k = u.CAL_TEMPS.size
    cols = np.stack([sref.ar1(np.random.default_rng(41), [0.95] * k, r, n // k).reshape(r, n),
                     sref.ar1(np.random.default_rng(42), [0.2] * k, r, n // k).reshape(r, n)], axis=1)
    eng = _store_engine(e, cols, k)
    return eng, eng.ladder_free_energies(method="newton")["f"], cols


def test_recorded_in_the_uncertainty_methods(ladder):
    eng, f, _ = ladder
    g = eng.recorded_inefficiency()["g"]
    assert np.all(np.isfinite(g)) and g[1].max() > g[0].max() > g[2].max()
    targets = u.CAL_TARGETS
    # free energies: the largest energy g over the rungs
    by_hand = float(np.max(g[0]))
    _same(eng.ladder_free_energy_uncertainties(f, targets, inefficiency="recorded"),
          eng.ladder_free_energy_uncertainties(f, targets, inefficiency=by_hand))
    _same(eng.ladder_free_energy_uncertainties(f, targets), eng.ladder_free_energy_uncertainties(f, targets, inefficiency=1.0))
    one, rec = eng.ladder_free_energy_uncertainties(f), eng.ladder_free_energy_uncertainties(f, inefficiency="recorded")
    assert np.allclose(rec["d_f"], one["d_f"] * np.sqrt(by_hand), rtol=1e-14, atol=0)
    # observables: per column the larger of the energy's and the column's
    per_column = np.array([max(np.max(g[0]), np.max(g[1 + q])) for q in range(2)])
    assert per_column[0] == g[1].max() and per_column[1] == g[0].max()
    _same(eng.observable_uncertainties(targets, f, inefficiency="recorded"),
          eng.observable_uncertainties(targets, f, inefficiency=per_column))
    _same(eng.observable_uncertainties(targets, f), eng.observable_uncertainties(targets, f, inefficiency=1.0))
    # profiles: along the energy the energy's g, along a column the larger of the two
    for which, edges, value in (("energy", np.linspace(0.0, 6.0, 13), by_hand), (0, np.linspace(-3.0, 3.0, 13), per_column[0]),
                                (eng.recorded_observables[1], np.linspace(-3.0, 3.0, 13), per_column[1])):
        _same(eng.free_energy_profile_uncertainties(which, edges, targets, f, inefficiency="recorded"),
              eng.free_energy_profile_uncertainties(which, edges, targets, f, inefficiency=float(value)))
        _same(eng.free_energy_profile_uncertainties(which, edges, targets, f),
              eng.free_energy_profile_uncertainties(which, edges, targets, f, inefficiency=1.0))
    for call in (lambda s: eng.ladder_free_energy_uncertainties(f, targets, inefficiency=s),
                 lambda s: eng.observable_uncertainties(targets, f, inefficiency=s),
                 lambda s: eng.free_energy_profile_uncertainties("energy", np.linspace(0.0, 6.0, 13), targets, f, inefficiency=s)):
        with pytest.raises(ValueError, match="recorded"):
            call("auto")


def test_recorded_refuses_a_series_without_inefficiency(ladder):
    eng, f, cols = ladder
    flat = cols.copy()
    flat[:, 1] = 1.0                         # column 1 has no variance: its g is NaN
    eng.set_observable_samples(flat)
    try:
        assert np.all(np.isnan(eng.recorded_inefficiency()["g"][2]))
        with pytest.raises(ValueError, match="recorded"):
            eng.observable_uncertainties(u.CAL_TARGETS, f, inefficiency="recorded")
        with pytest.raises(ValueError, match="recorded"):
            eng.free_energy_profile_uncertainties(1, np.linspace(0.0, 2.0, 5), u.CAL_TARGETS, f, inefficiency="recorded")
        # what does not need that column still works
        eng.ladder_free_energy_uncertainties(f, inefficiency="recorded")
        eng.free_energy_profile_uncertainties(0, np.linspace(-3.0, 3.0, 13), u.CAL_TARGETS, f, inefficiency="recorded")
    finally:
        eng.set_observable_samples(cols)


# ---- 6. the calibration on the device -----------------------------------------------------------------------------------
def test_calibration_on_the_device():
    """The 64 replicas of tests/test_series_reference_cpu.py through an engine: error bars too small by sqrt(g) with
    inefficiency = 1, honest (slightly conservative: the largest g over the rungs) with "recorded"."""
    replicas = sref.calibration_energies()
    eng = _store_engine(replicas[0], None, u.CAL_TEMPS.size)
    f_all, sig_1, sig_g = [], [], []
    for e in replicas:
        eng.set_energy_samples(e)
        f = eng.ladder_free_energies(method="newton")["f"]
        f_all.append(f)
        sig_1.append(eng.ladder_free_energy_uncertainties(f)["d_f"])
        sig_g.append(eng.ladder_free_energy_uncertainties(f, inefficiency="recorded")["d_f"])
    z_1, z_g = sref.calibration_z(f_all, sig_1), sref.calibration_z(f_all, sig_g)
    print("pooled RMS z of f[1:]: %.3f with inefficiency 1, %.3f with \"recorded\"" % (z_1, z_g))
    assert z_1 > 1.5
    assert 0.7 <= z_g <= 1.2


# ---- 7. a real run ------------------------------------------------------------------------------------------------------
def _run(sweeps_between):
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=4 * 256, seed=11, dtype="f64",
                              temperatures=u.CAL_TEMPS)
    eng.step_all(500)
    eng.record_energies(64)
    eng.record_observables(["real_0", "real_0_sq"])
    for _ in range(64):
        eng.step_all(sweeps_between)
        eng.record_energy()
    return eng.recorded_inefficiency()


def test_the_example_runs(capsys):
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    try:
        demo = importlib.import_module("demo_recorded_inefficiency")
    finally:
        sys.path.pop(0)
    out = demo.main(chains_per_rung=512, burn_in=200, n_records=48)
    text = capsys.readouterr().out
    print(text)
    g = out["inefficiency"]["g"][0]
    assert "stop lag" in text and "d_f (recorded)" in text
    assert np.all(np.isfinite(g)) and np.all(g >= 1.0)
    assert np.allclose(out["d_f_recorded"], out["d_f"] * np.sqrt(g.max()), rtol=1e-12, atol=0)


def test_a_real_run():
    dense, sparse = _run(1), _run(20)
    for name, out in (("1 sweep", dense), ("20 sweeps", sparse)):
        print("records %s apart: g of %s per rung\n%s" % (name, out["names"], np.round(out["g"], 2)))
        assert out["names"] == ("energy", "real_0", "real_0_sq") and out["n_records"] == 64
        assert np.all(np.isfinite(out["g"])) and np.all(out["g"] >= 1.0) and np.all(out["chains_used"] == 256)
    assert np.all(dense["g"][0] > sparse["g"][0])
