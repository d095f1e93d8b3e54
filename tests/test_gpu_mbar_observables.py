"""Recorded observables and their MBAR reweighting on the GPU (csrc/me_mbar_obs.hip) against the host's restatement of a
record, the long-double reference of tests/mbar_observables_reference.py and exact results.  Every figure is printed before
it is asserted (run with -s); profiles/mbar_observables.txt holds the values measured on the MI355X.

Sample counts.  An engine's store holds records x n_chains samples and a ladder engine's n_chains is a multiple of 64 K
(every rung is a run of whole 64-chain tiles), so the ragged count 2048 * 3 + 5 = 11 * 13 * 43 cannot be a store: it goes through
the engine-less form (the same kernels, bit for bit: test 3), and the stores take the ragged counts 512 x 33 = 8 * 2048 + 512
(K = 8; four records to a tile) and 2112 x 6 = 6 * 2048 + 384 (K = 33; a record ends inside a thread's stride).  For the same
reason the ladder engines of test 1 have 512 chains; the ragged 192 is for the engines that need no ladder."""
import ctypes

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_reference as ref
import mbar_observables_reference as oref

pytestmark = pytest.mark.gpu
LADDER8 = oref.LADDER8
F_BOUND = 1e-8          # the project's bound for float64 quantities that pass through iterated arithmetic
# Largest relative errors of mean / var / cov_energy (and of neff_fraction) against the long-double reference over the cases
# of test 2 as measured on the MI355X (profiles/mbar_observables.txt); the tests assert ten times these, capped at 1e-8.
MEASURED_MEAN_ERROR = 2.03e-16
MEASURED_VAR_ERROR = 4.00e-16
MEASURED_COV_ERROR = 7.02e-16
MEASURED_NEFF_ERROR = 4.88e-16
BOUND = {"mean": min(10 * MEASURED_MEAN_ERROR, F_BOUND), "var": min(10 * MEASURED_VAR_ERROR, F_BOUND),
         "cov_energy": min(10 * MEASURED_COV_ERROR, F_BOUND), "neff_fraction": min(10 * MEASURED_NEFF_ERROR, F_BOUND)}
RAGGED = 2048 * 3 + 5
LARGE = 2048 * 2048 + 5         # more tiles than blocks: a block walks more than one tile


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


# ------------------------------------------------------------------------------------------------------ 1. the records


def _engine(kind, dtype):
    kw = dict(seed=5, dtype=dtype)
    if kind == "4,0":
        return me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1, -0.2, 0.3, 0.4], None, n_chains=192, temp=1.0, **kw)
    if kind == "16,0":          # tile-major state
        return me.MetropolisEngine(me.IsoQuadratic(1.0), None, list(0.05 * np.arange(1, 17)), None, n_chains=192, temp=1.0, **kw)
    if kind == "2,1":
        return me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.3, 0.2], [0.4 + 0.1j], n_chains=192, temp=0.7, **kw)
    if kind == "landau":        # three ledger rows
        return me.MetropolisEngine(me.LandauToy(1.0, -1.0, 0.5, terms=True), None, [0.3, 0.2], [0.4 + 0.1j], n_chains=192, temp=0.7,
                                   **kw)
    assert kind == "runtime"    # the runtime-dimension kernel set: component-major whatever D
    return me.MetropolisEngine(me.IsoQuadratic(1.0), None, list(0.01 * np.arange(1, 101)), None, n_chains=128, temp=1.0,
                               cov_mode="fixed", **kw)


def _restated(eng):
    return oref.catalogue_values(eng._get(_capi.FIELD_PARAMS), eng._get(_capi.FIELD_ENERGY), eng.num_real_params,
                                 eng.num_complex_params)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["4,0", "16,0", "2,1", "landau", "runtime"])
def test_records_are_the_hosts_restatement(kind, dtype):
    eng = _engine(kind, dtype)
    names = eng.observable_names()
    nr, nc = eng.num_real_params, eng.num_complex_params
    assert names == oref.catalogue_names(nr, nc, eng.energy_term_names)
    if kind == "landau":
        assert len(eng.energy_term_names) > 1
    # up to 16 columns: the ends of every range of the catalogue, one duplicate, in an order of their own
    d, nobs = nr + 2 * nc, 2 * nr + nc
    pick = sorted({0, d - 1, d, d + nr - 1, d + nr + nc - 1, d + nobs - 1, d + nobs, len(names) - 1, nr, d + nr}
                  & set(range(len(names))))[::-1]
    pick = (pick + [pick[0]] + list(range(1, len(names), 7)))[:16]
    eng.record_energies(3)
    eng.record_observables([names[q] if j % 2 else q for j, q in enumerate(pick)])
    assert eng.recorded_observables == tuple(names[q] for q in pick)
    is_abs_z = np.array([d + nr <= q < d + nr + nc for q in pick])
    rows, energies = [], []
    for r in range(3):
        eng.step_all(4)
        eng.record_energy()
        rows.append(_restated(eng)[pick])
        ledger = eng._get(_capi.FIELD_ENERGY).astype(np.float32 if dtype == "f32" else np.float64)
        total = ledger[:, 0].copy()
        for t in range(1, ledger.shape[1]):      # the energy record: the ledger rows added in row order in the device dtype
            total = total + ledger[:, t]
        energies.append(total.astype(np.float64))
        got = eng.observable_samples()
        assert got.shape == (r + 1, len(pick), eng.n_chains) and got.dtype == np.float64
        assert eng.n_energy_records == r + 1
        want = rows[-1]
        assert _bitwise(got[-1][~is_abs_z], want[~is_abs_z])            # bit for bit
        if is_abs_z.any():
            ulps = np.abs(got[-1][is_abs_z] - want[is_abs_z]) / np.spacing(want[is_abs_z])
            print(kind, dtype, "record", r, "|z|: largest distance from np.hypot in ulp:", ulps.max())
            assert ulps.max() <= 2
    assert _bitwise(eng.observable_samples()[:, ~is_abs_z], np.array(rows)[:, ~is_abs_z])     # rows keep their order
    assert np.array_equal(eng.energy_samples(), np.array(energies))                           # the energy row as before
    assert len(np.unique(eng.observable_samples()[0, 0])) > 1                                 # the chains have moved
    with pytest.raises(_capi.MetropolisLibraryError, match="full"):
        eng.record_energy()                                   # full (ME_ERR_STATE): neither store moves
    assert eng.n_energy_records == 3 and eng.observable_samples().shape[0] == 3


def test_enable_reenable_free_and_a_new_ladder_reset_both_counts():
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1, 0.2], [0.3j], n_chains=8 * 64, seed=5, dtype="f64",
                              temperatures=LADDER8)
    eng.record_energies(4)
    eng.record_energy()
    assert eng.n_energy_records == 1 and eng.recorded_observables == ()
    eng.record_observables(["abs_complex_0", "real_1"])       # enabling forgets the energy record too
    assert eng.n_energy_records == 0 and eng.observable_samples().shape == (0, 2, eng.n_chains)
    eng.record_energy()
    eng.record_energy()
    assert eng.n_energy_records == 2 and eng.observable_samples().shape[0] == 2
    eng.record_observables(["real_0"])                        # re-enabling: other columns, both counts 0
    assert eng.n_energy_records == 0 and eng.recorded_observables == ("real_0",)
    eng.record_energy()
    eng.set_temperatures(LADDER8 * 1.5)                       # a new ladder empties both, the stores stay
    assert eng.n_energy_records == 0 and eng.observable_samples().shape == (0, 1, eng.n_chains)
    eng.record_energy()
    assert eng.n_energy_records == 1 and eng.observable_samples().shape[0] == 1
    eng.record_observables(None)                              # freeing keeps the energy records
    assert eng.recorded_observables == () and eng.n_energy_records == 1
    with pytest.raises(ValueError):
        eng.observable_samples()
    eng.record_energy()                                       # ... and the energy store goes on alone
    assert eng.n_energy_records == 2
    eng.record_observables(["real_0"])
    eng.record_energies(2)                                    # a new energy store forgets the observable store
    assert eng.recorded_observables == ()


def test_set_get_round_trip_preserves_nan_and_inf_bit_patterns():
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=8 * 64, seed=5, dtype="f64", temperatures=LADDER8)
    eng.record_energies(4)
    eng.record_observables(["real_0", "abs_real_0", "energy_total"])
    assert np.array_equal(eng.observable_samples(), np.zeros((0, 3, eng.n_chains)))
    rng = np.random.default_rng(2)
    energies = rng.standard_normal((3, eng.n_chains))
    a = rng.standard_normal((3, 3, eng.n_chains))
    bits = a.view(np.uint64)
    bits[0, 1, 5] = 0x7FF8000000000123          # a quiet NaN with a payload
    bits[1, 2, 7] = 0xFFF0000000000000          # -inf
    bits[2, 0, 9] = 0x7FF0000000000000          # +inf
    bits[2, 2, 11] = 0x8000000000000000         # -0.0
    with pytest.raises(ValueError):
        eng.set_observable_samples(a)                          # the energy store has 0 records
    eng.set_energy_samples(energies)
    assert np.array_equal(_u64(eng.observable_samples()), np.zeros((3, 3, eng.n_chains), dtype=np.uint64))   # zero-filled
    eng.set_observable_samples(a)
    assert np.array_equal(_u64(eng.observable_samples()), bits)
    with pytest.raises(ValueError):
        eng.set_observable_samples(a[:2])
    with pytest.raises(ValueError):
        eng.set_observable_samples(a[:, :2])
    eng.record_energy()                                        # appends after the rows that were set
    assert eng.n_energy_records == 4 and np.array_equal(_u64(eng.observable_samples()[:3]), bits)


def test_error_cases():
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=128, temp=1.0)
    with pytest.raises(ValueError, match="energy store"):
        eng.record_observables(["real_0"])                     # no energy store
    eng.record_energies(2)
    with pytest.raises(ValueError):
        eng.record_observables(["real_0"] * 17)
    with pytest.raises(ValueError, match="unknown observable"):
        eng.record_observables(["real_1"])
    with pytest.raises(ValueError):
        eng.record_observables([len(eng.observable_names())])
    with pytest.raises(ValueError):
        eng.reweight_observables([1.0])                        # no observable store
    eng.record_observables(["real_0"])
    eng.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
        eng.reweight_observables([1.0], f=[0.0])               # no ladder
    idx = (ctypes.c_int32 * 1)(99)
    assert eng._lib.me_observable_samples_enable(eng._handle, idx, 1) == _capi.ME_ERR_INVALID
    assert eng._lib.me_observable_samples_enable(eng._handle, idx, 17) == _capi.ME_ERR_INVALID
    ledgers = me.MetropolisEngine(me.LandauToy(), None, [0.0, 0.0], [0j], n_chains=128, reference_energy_ledgers=True)
    with pytest.raises(NotImplementedError, match="LEDGERS"):
        ledgers.record_observables(["real_0"])


# ------------------------------------------------------------------------- 2. the kernels against the long-double reference


def _ladder(k):
    return 0.5 * (1.3 ** 7) ** (np.arange(k) / (k - 1.0))


def _columns(e, q, rng):
    """``q`` columns for the energies ``e``: column 0 is a copy of E, the others a_j + b_j E + noise with a_j, b_j > 0, so that
    neither their mean nor their covariance with E is a small difference (a relative error means something)."""
    cols = [e.copy()]
    for j in range(1, q):
        cols.append((j + 1.0) + 0.25 * (1 + j % 3) * e + (0.5 + 0.1 * j) * rng.standard_normal(e.size) * np.sqrt(e))
    return np.stack(cols)


def _flat_problem(k, n, q, seed=17):
    """Engine-less inputs: ``n`` samples, rung i % k, Gamma energies of the D = 16 quadratic form."""
    temps = _ladder(k)
    rng = np.random.default_rng(seed)
    rungs = (np.arange(n) % k).astype(np.int32)
    e = rng.gamma(8.0, temps[rungs])
    return temps, e, rungs, _columns(e, q, rng)


def _store_problem(k, m, records, q, seed=19):
    """The same as an engine's stores: ``(engine, temps, energies (records, k m), rungs, columns (records, q, k m))``."""
    temps = _ladder(k)
    rng = np.random.default_rng(seed)
    e = np.stack([np.concatenate([rng.gamma(8.0, t, size=m) for t in temps]) for _ in range(records)])
    cols = _columns(e.ravel(), q, rng).reshape(q, records, k * m).transpose(1, 0, 2).copy()
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, [0.1j] * 4, n_chains=k * m, seed=5, dtype="f64",
                              temperatures=temps)
    eng.record_energies(records)
    eng.record_observables(list(range(q)))
    eng.set_energy_samples(e)
    eng.set_observable_samples(cols)
    return eng, temps, e, np.tile(np.repeat(np.arange(k), m), records), cols


def _targets(temps, n):
    """``n`` target temperatures: both ends of the ladder first, then rungs and points between rungs."""
    k = temps.size
    pool = [temps[0], temps[-1], 0.57, temps[k // 2], 0.8, temps[1], 1.5, temps[3 * k // 4], 2.6]
    return np.array([0.9]) if n == 1 else np.array(pool[:n])


def _relative_errors(label, got, want):
    """Largest relative error of every result against the long-double ``want`` (printed: profiles/mbar_observables.txt)."""
    rel = {}
    for key, w in zip(("mean", "var", "cov_energy", "neff_fraction"), want):
        scale = np.where(w != 0, np.abs(w), 1.0)
        rel[key] = float(np.max(np.abs(got[key].astype(np.longdouble) - w) / scale))
    print("%s: largest relative error against long double: %s" % (label, rel))
    return rel


def _assert_errors(rel):
    for key, bound in BOUND.items():
        assert rel[key] <= bound, (key, rel[key], bound)


def _check_energy_column(got, energy_rw):
    """Column 0 is a copy of E: its mean and variance are the energy's of me_mbar_reweight, its covariance with E is its
    variance, all within the bound of this test.  neff_fraction is compared WITHIN THE BOUND, not bit for bit: this unit is
    compiled without floating-point contraction (so that a column's rounding cannot depend on its place in a pass), the
    energy kernels with the compiler's default."""
    for name, a, b, bound in (("mean", got["mean"][:, 0], energy_rw["energy_mean"], BOUND["mean"]),
                              ("var", got["var"][:, 0], energy_rw["energy_var"], BOUND["var"]),
                              ("cov = var", got["cov_energy"][:, 0], got["var"][:, 0], BOUND["cov_energy"]),
                              ("neff", got["neff_fraction"], energy_rw["neff_fraction"], BOUND["neff_fraction"])):
        err = float(np.max(np.abs(a - b) / np.abs(b)))
        print("  energy column, %s: largest relative difference %.3e" % (name, err))
        assert err <= bound, name
    assert np.array_equal(got["dmean_dT"], got["cov_energy"] / (got["temps"] ** 2)[:, None])


@pytest.mark.parametrize("k, q, n_targets", [(8, 5, 9), (33, 16, 4)])
def test_ragged_tile_matches_the_long_double_reference(k, q, n_targets):
    temps, e, rungs, cols = _flat_problem(k, RAGGED, q)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, n_targets)
    got = statistics.mbar_reweight_observables(e, rungs, temps, f, targets, cols)
    assert got["mean"].shape == (n_targets, q) and got["neff_fraction"].shape == (n_targets,) and got["names"] == tuple(range(q))
    want = oref.reweight_observables(e, rungs, temps, f, targets, cols, dtype=np.longdouble)
    _assert_errors(_relative_errors("engine-less n=%d K=%d Q=%d T=%d" % (RAGGED, k, q, n_targets), got, want))
    _check_energy_column(got, statistics.mbar_reweight(e, rungs, temps, f, targets))


@pytest.mark.parametrize("k, m, records, q, n_targets", [(8, 64, 33, 16, 5), (33, 64, 6, 1, 1)])
def test_stores_match_the_long_double_reference(k, m, records, q, n_targets):
    eng, temps, e, rungs, cols = _store_problem(k, m, records, q)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, n_targets)
    got = eng.reweight_observables(targets, f)
    assert got["names"] == tuple(eng.observable_names()[:q])
    flat = cols.transpose(1, 0, 2).reshape(q, -1)
    want = oref.reweight_observables(e, rungs, temps, f, targets, flat, dtype=np.longdouble)
    _assert_errors(_relative_errors("store %dx%d K=%d Q=%d T=%d" % (records, k * m, k, q, n_targets), got, want))
    _check_energy_column(got, eng.reweight(targets, f))


def test_a_block_that_walks_several_tiles_matches_the_long_double_reference():
    """2048 * 2048 + 5 samples: 2049 tiles on 2048 blocks, through the engine-less form (about 100 MB with Q = 2)."""
    temps, e, rungs, cols = _flat_problem(8, LARGE, 2)
    f = statistics.mbar_free_energies(e, rungs, temps, tol=1e-8)["f"]
    targets = np.array([1.1])
    got = statistics.mbar_reweight_observables(e, rungs, temps, f, targets, cols)
    want = oref.reweight_observables(e, rungs, temps, f, targets, cols, dtype=np.longdouble)
    _assert_errors(_relative_errors("engine-less n=%d K=8 Q=2 T=1" % LARGE, got, want))
    _check_energy_column(got, statistics.mbar_reweight(e, rungs, temps, f, targets))


# ------------------------------------------------------------------------------ 3. chunk independence and reproducibility


def test_results_do_not_depend_on_the_chunks_and_are_reproducible():
    eng, temps, e, rungs, cols = _store_problem(8, 64, 33, 16)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, 9)
    whole = eng.reweight_observables(targets, f)
    again = eng.reweight_observables(targets, f)
    flat = cols.transpose(1, 0, 2).reshape(16, -1)
    less = statistics.mbar_reweight_observables(e, rungs, temps, f, targets, flat)
    for key in ("mean", "var", "cov_energy", "dmean_dT", "neff_fraction"):
        assert _bitwise(whole[key], again[key]), key            # two calls
        assert _bitwise(whole[key], less[key]), key             # engine form and engine-less form
    for q, t in ((0, 0), (3, 3), (4, 4), (7, 8), (15, 8), (9, 5), (13, 2)):
        one = statistics.mbar_reweight_observables(e, rungs, temps, f, [targets[t]], flat[q])
        for key in ("mean", "var", "cov_energy"):
            assert _bitwise(one[key][0, 0], whole[key][t, q]), (key, q, t)     # alone = among 16 x 9
        assert _bitwise(one["neff_fraction"][0], whole["neff_fraction"][t])
    # ... and through the engine: a store of that one column
    eng.record_observables([11])
    eng.set_energy_samples(e)
    eng.set_observable_samples(cols[:, 11:12])
    one = eng.reweight_observables([targets[6]], f)
    for key in ("mean", "var", "cov_energy"):
        assert _bitwise(one[key][0, 0], whole[key][6, 11]), key


# --------------------------------------------------------------------------------------- 4. unused and non-finite samples


def test_samples_with_non_finite_energies_are_not_used():
    """Implemented: WITHIN THE BOUND of test 2, not bit for bit -- removing samples moves the others to other lanes and
    tiles, which changes the order of the sums."""
    temps, e, rungs, cols = _flat_problem(8, RAGGED, 5, seed=23)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    dirty, dirty_cols = e.copy(), cols.copy()
    dirty[[3, 64, 2047, 2048, 4100, RAGGED - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    dirty_cols[:, [3, 64, 4100]] = np.nan                     # of unused samples: never seen
    dirty_cols[1, 2047] = np.inf
    keep = np.isfinite(dirty)
    targets = _targets(temps, 4)
    a = statistics.mbar_reweight_observables(dirty, rungs, temps, f, targets, dirty_cols)
    b = statistics.mbar_reweight_observables(dirty[keep], rungs[keep], temps, f, targets, dirty_cols[:, keep])
    for key in ("mean", "var", "cov_energy", "neff_fraction"):
        err = float(np.max(np.abs(a[key] - b[key]) / np.abs(b[key])))
        print("planted against removed, %s: largest relative difference %.3e" % (key, err))
        assert np.all(np.isfinite(a[key])) and err <= BOUND[key], key
    want = oref.reweight_observables(dirty, rungs, temps, f, targets, dirty_cols, dtype=np.longdouble)
    _assert_errors(_relative_errors("engine-less n=%d K=8 Q=5 T=4, 6 unused samples" % RAGGED, a, want))


@pytest.mark.parametrize("q", [4, 5])
def test_a_non_finite_observable_stays_in_its_column(q):
    temps, e, rungs, cols = _flat_problem(8, RAGGED, q, seed=29)
    f = statistics.mbar_free_energies(e, rungs, temps)["f"]
    targets = _targets(temps, 5)
    clean = statistics.mbar_reweight_observables(e, rungs, temps, f, targets, cols)
    for value in (np.nan, np.inf):
        bad = cols.copy()
        bad[2, 1234] = value                                  # a used sample
        got = statistics.mbar_reweight_observables(e, rungs, temps, f, targets, bad)
        others = [j for j in range(q) if j != 2]
        for key in ("mean", "var", "cov_energy"):
            assert not np.any(np.isfinite(got[key][:, 2])), (key, value)
            assert _bitwise(got[key][:, others], clean[key][:, others]), (key, value)
        assert _bitwise(got["neff_fraction"], clean["neff_fraction"])


# ------------------------------------------------------------------------------------------------------ 5. exact physics


def test_exact_moments_of_the_quadratic_energy():
    """Exact samples of E = |x|^2 in 4 real dimensions on LADDER8, 16 independent subsets of 8 x 1024: the means of x_0,
    |x_0|, x_0^2 and d<x_0^2>/dT at three temperatures between rungs, twelve comparisons, each within 5 standard errors.
    tests/test_mbar_observables_cpu.py shows that the reference meets all twelve on these very inputs."""
    results = []
    for e, rungs, cols in oref.iso_quadratic_subsets():
        out = statistics.mbar_free_energies(e, rungs, LADDER8)
        assert out["converged"]
        rw = statistics.mbar_reweight_observables(e, rungs, LADDER8, out["f"], oref.PHYSICS_TARGETS, cols)
        assert np.array_equal(rw["dmean_dT"], rw["cov_energy"] / (oref.PHYSICS_TARGETS ** 2)[:, None])
        results.append((rw["mean"], rw["cov_energy"]))
    n = 0
    for name, (est, exact) in oref.physics_estimates(results).items():
        ok, m, se = ref.within_5_se(est, exact)
        print(name, "mean", m, "exact", exact, "se", se, "deviation / se", np.abs(m - exact) / se)
        assert np.all(ok), name
        n += ok.size
    assert n == 12


# --------------------------------------------------------------------------------------------------------- 6. end to end


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ladder_engine_end_to_end(dtype):
    """A (2, 1) quadratic ladder: MBAR at the rungs' own temperatures against the plain per-rung means of the records.  The
    records of a slot are correlated in time, the slots of a rung are independent: the standard error of a plain mean is the
    spread over the M slots of their time averages."""
    k, m, records = 8, 256, 32
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0, 0.0], [0j], n_chains=k * m, seed=47, dtype=dtype,
                              temperatures=LADDER8)
    for _ in range(200):
        eng.step_all(5)
        eng.replica_exchange()
    which = ["abs_real_0", "abs_complex_0", "real_1_sq", "real_0", "im_0", "energy_total"]
    eng.record_energies(records)
    eng.record_observables(which)
    for _ in range(records):
        eng.step_all(5)
        eng.replica_exchange()
        eng.record_energy()
    out = eng.reweight_observables(LADDER8)
    assert out["names"] == tuple(which) == eng.recorded_observables
    assert np.all((out["neff_fraction"] > 0) & (out["neff_fraction"] <= 1)) and np.all(out["var"] >= 0)
    samples = eng.observable_samples().reshape(records, len(which), k, m)
    assert np.array_equal(samples[:, 5].reshape(records, -1), eng.energy_samples())       # one ledger row: the energy itself
    per_slot = samples.mean(axis=0)                              # (Q, K, M) time averages
    plain = per_slot.mean(axis=2).T                              # (K, Q)
    se = (per_slot.std(axis=2, ddof=1) / np.sqrt(m)).T
    dev = np.abs(out["mean"] - plain) / se
    print(dtype, "MBAR at the rungs\n", out["mean"], "\nplain means\n", plain, "\nstandard errors\n", se, "\ndeviation / se\n", dev)
    assert np.all(dev <= 5.0)
