"""MBAR reweighting to perturbed energies on the GPU (csrc/me_mbar_perturbed.hip) against the long-double reference of
tests/mbar_perturbed_reference.py, against the temperature reweighting it must contain, and against closed forms.  Every
figure is printed before it is asserted (run with -s); profiles/mbar_perturbed.txt holds the values measured on the MI355X.

The inputs are those of tests/test_gpu_mbar_observables.py (its _ladder, _columns, _flat_problem, _store_problem and _targets,
restated here); the couplings are pref.case_couplings: 0.05 (-1)^(p + q) / (q + 1), 0 where (p + 2 q) % 3 == 0, so that every
target skips columns.  Every relative error is taken where the long-double reference's neff_fraction is >= 0.1 (asserted: a
collapsed weight set would make a relative error meaningless; the least at the ragged count is 0.167)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_observables_reference as oref
import mbar_perturbed_reference as pref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LADDER8 = oref.LADDER8
F_BOUND = 1e-8          # the project's bound for float64 quantities that pass through iterated arithmetic
# Largest relative errors (ln_z: absolute over max(|ln_z|, 1)) against the long-double reference over the first four cases of
# test 3 as measured on the MI355X (profiles/mbar_perturbed.txt); the tests assert ten times these, capped at 1e-8.
MEASURED_LN_Z_ERROR = 5.58e-16
MEASURED_HAMILTONIAN_MEAN_ERROR = 2.33e-16
MEASURED_HAMILTONIAN_VAR_ERROR = 3.72e-16
MEASURED_MEAN_ERROR = 2.34e-16
MEASURED_VAR_ERROR = 4.59e-16
MEASURED_COV_ERROR = 5.19e-16
MEASURED_NEFF_ERROR = 5.20e-16
BOUND = {key: min(10 * measured, F_BOUND) for key, measured in (
    ("ln_z", MEASURED_LN_Z_ERROR), ("hamiltonian_mean", MEASURED_HAMILTONIAN_MEAN_ERROR),
    ("hamiltonian_var", MEASURED_HAMILTONIAN_VAR_ERROR), ("mean", MEASURED_MEAN_ERROR), ("var", MEASURED_VAR_ERROR),
    ("cov_hamiltonian", MEASURED_COV_ERROR), ("neff_fraction", MEASURED_NEFF_ERROR))}
RAGGED = 2048 * 3 + 5
LARGE = 2048 * 2048 + 5         # more tiles than blocks: a block walks more than one tile


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


# ---- the inputs of tests/test_gpu_mbar_observables.py, restated


def _ladder(k):
    return 0.5 * (1.3 ** 7) ** (np.arange(k) / (k - 1.0))


def _columns(e, q, rng):
    """``q`` columns for the energies ``e``: column 0 is a copy of E, the others a_j + b_j E + noise with a_j, b_j > 0."""
    cols = [e.copy()]
    for j in range(1, q):
        cols.append((j + 1.0) + 0.25 * (1 + j % 3) * e + (0.5 + 0.1 * j) * rng.standard_normal(e.size) * np.sqrt(e))
    return np.stack(cols)


@functools.lru_cache(maxsize=None)
def _flat_problem(k, n, q, seed=17):
    """Engine-less inputs: ``n`` samples, rung i % k, Gamma energies of the D = 16 quadratic form; with their solved f.  Shared:
    nobody writes into them."""
    temps = _ladder(k)
    rng = np.random.default_rng(seed)
    rungs = (np.arange(n) % k).astype(np.int32)
    e = rng.gamma(8.0, temps[rungs])
    cols = _columns(e, q, rng)
    f = statistics.mbar_free_energies(e, rungs, temps, tol=1e-8 if n == LARGE else 1e-10)["f"]
    for a in (temps, e, rungs, cols, f):
        a.flags.writeable = False
    return temps, e, rungs, cols, f


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


def _relative(got, want, key):
    want = np.asarray(want, dtype=np.longdouble)
    scale = np.maximum(np.abs(want), 1.0) if key == "ln_z" else np.where(want != 0, np.abs(want), 1.0)
    return float(np.max(np.abs(np.asarray(got).astype(np.longdouble) - want) / scale))


def _assert_errors(label, got, want, keys=pref.KEYS):
    """Largest relative error of every key against the long-double ``want`` (printed: profiles/mbar_perturbed.txt)."""
    assert np.min(want["neff_fraction"]) >= 0.1, np.min(want["neff_fraction"])
    rel = {key: _relative(got[key], want[key], key) for key in keys}
    print("%s: least neff_fraction %.3f; largest relative error against long double: %s"
          % (label, float(np.min(want["neff_fraction"])), rel))
    for key in keys:
        assert rel[key] <= BOUND[key], (key, rel[key], BOUND[key])
    return rel


# ------------------------------------------------------------------------------------- 3. the long-double reference


@pytest.mark.parametrize("k, q, n_targets", [(8, 5, 9), (33, 16, 4)])
def test_ragged_tile_matches_the_long_double_reference(k, q, n_targets):
    temps, e, rungs, cols, f = _flat_problem(k, RAGGED, q)
    targets, lam = _targets(temps, n_targets), pref.case_couplings(n_targets, q)
    got = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, lam, cols)
    assert got["mean"].shape == got["cov_hamiltonian"].shape == (n_targets, q) and got["names"] == tuple(range(q))
    assert got["ln_z"].shape == got["hamiltonian_var"].shape == got["neff_fraction"].shape == (n_targets,)
    assert np.array_equal(got["couplings"], lam) and np.array_equal(got["temps"], targets)
    want = pref.reweight_perturbed(e, rungs, temps, f, targets, lam, cols, dtype=np.longdouble)
    _assert_errors("engine-less n=%d K=%d Q=%d P=%d" % (RAGGED, k, q, n_targets), got, want)
    assert np.array_equal(got["heat_capacity"], got["hamiltonian_var"] / targets ** 2)
    assert np.array_equal(got["dmean_dT"], got["cov_hamiltonian"] / (targets ** 2)[:, None])
    assert np.allclose(got["perturbation_mean"], (lam * got["mean"]).sum(axis=1), rtol=1e-14, atol=0)
    assert np.allclose(got["hamiltonian_mean"] - got["perturbation_mean"], got["mean"][:, 0], rtol=1e-12)   # column 0 is E


@pytest.mark.parametrize("k, m, records, q, n_targets", [(8, 64, 33, 16, 5), (33, 64, 6, 1, 1)])
def test_stores_match_the_long_double_reference(k, m, records, q, n_targets):
    eng, temps, e, rungs, cols = _store_problem(k, m, records, q)
    f = eng.ladder_free_energies()["f"]
    targets, lam = _targets(temps, n_targets), pref.case_couplings(n_targets, q)
    got = eng.reweight_perturbed(targets, lam, f)
    assert got["names"] == tuple(eng.observable_names()[:q])
    flat = cols.transpose(1, 0, 2).reshape(q, -1)
    want = pref.reweight_perturbed(e, rungs, temps, f, targets, lam, flat, dtype=np.longdouble)
    _assert_errors("store %dx%d K=%d Q=%d P=%d" % (records, k * m, k, q, n_targets), got, want)


def test_a_block_that_walks_several_tiles_matches_the_long_double_reference():
    """2048 * 2048 + 5 samples: 2049 tiles on 2048 blocks, through the engine-less form (about 100 MB with Q = 2)."""
    temps, e, rungs, cols, f = _flat_problem(8, LARGE, 2)
    targets, lam = np.array([1.1]), pref.case_couplings(1, 2)
    got = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, lam, cols)
    want = pref.reweight_perturbed(e, rungs, temps, f, targets, lam, cols, dtype=np.longdouble)
    _assert_errors("engine-less n=%d K=8 Q=2 P=1" % LARGE, got, want)


# ------------------------------------------------------------------------------------------------ 4. zero couplings


def test_zero_couplings_are_the_temperature_reweighting():
    eng, temps, e, rungs, cols = _store_problem(8, 64, 33, 16)
    f = eng.ladder_free_energies()["f"]
    targets = _targets(temps, 9)
    got = eng.reweight_perturbed(targets, np.zeros((9, 16)), f)
    obs, energy = eng.reweight_observables(targets, f), eng.reweight(targets, f)
    for key, other in (("mean", "mean"), ("var", "var"), ("cov_hamiltonian", "cov_energy"), ("dmean_dT", "dmean_dT"),
                       ("neff_fraction", "neff_fraction")):
        assert _bitwise(got[key], obs[other]), key
    assert np.all(got["perturbation_mean"] == 0)
    for key, other in (("ln_z", "ln_z"), ("hamiltonian_mean", "energy_mean"), ("hamiltonian_var", "energy_var")):
        err = _relative(got[key], energy[other], key)
        print("zero couplings, %s against reweight's %s: largest relative difference %.3e" % (key, other, err))
        assert err <= BOUND[key], key
    one = eng.reweight_perturbed(targets, {}, f)                  # an empty dictionary: the same
    assert all(_bitwise(one[key], got[key]) for key in pref.KEYS)


# ------------------------------------------------------------------------ 5. a coupling to the energy is a temperature


@pytest.mark.parametrize("lam", [0.25, -0.2])
def test_a_coupling_to_the_energy_column_is_a_temperature(lam):
    temps, e, rungs, cols, f = _flat_problem(8, RAGGED, 5)
    targets = np.array([0.7, 1.0, 1.5, 2.2])                  # T / (1 + lambda) stays inside the ladder, 0.5 ... 3.14
    got = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, {0: lam}, cols)
    assert np.min(got["neff_fraction"]) >= 0.1
    energy = statistics.mbar_reweight(e, rungs, temps, f, targets / (1 + lam))
    obs = statistics.mbar_reweight_observables(e, rungs, temps, f, targets / (1 + lam), cols)
    for name, a, b, key in (("ln_z", got["ln_z"], energy["ln_z"], "ln_z"),
                            ("mean", got["mean"][:, 1:], obs["mean"][:, 1:], "mean"),
                            ("var", got["var"][:, 1:], obs["var"][:, 1:], "var"),
                            ("hamiltonian_mean", got["hamiltonian_mean"], (1 + lam) * energy["energy_mean"], "hamiltonian_mean")):
        err = _relative(a, b, key)
        print("lambda = %g on the energy column against T / (1 + lambda), %s: largest relative difference %.3e" % (lam, name, err))
        assert err <= BOUND[key], name


# -------------------------------------------------------------------------------- 6. independence and reproducibility


def test_targets_do_not_depend_on_each_other_and_are_reproducible():
    eng, temps, e, rungs, cols = _store_problem(8, 64, 33, 16)
    f = eng.ladder_free_energies()["f"]
    targets, lam = _targets(temps, 9), pref.case_couplings(9, 16)
    whole = eng.reweight_perturbed(targets, lam, f)
    again = eng.reweight_perturbed(targets, lam, f)
    less = statistics.mbar_reweight_perturbed(eng.energy_samples(), rungs, temps, f, targets, lam,
                                              eng.observable_samples().transpose(1, 0, 2).reshape(16, -1))
    order = np.array([4, 8, 0, 3, 7, 1, 6, 2, 5])
    moved = eng.reweight_perturbed(targets[order], lam[order], f)
    for key in pref.KEYS + ("dmean_dT", "heat_capacity", "perturbation_mean"):
        assert _bitwise(whole[key], again[key]), key            # two calls
        assert _bitwise(whole[key], less[key]), key             # engine form and engine-less form
        assert _bitwise(whole[key][order], moved[key]), key     # any position
    for t in (0, 3, 4, 8):
        one = eng.reweight_perturbed([targets[t]], lam[t:t + 1], f)
        for key in pref.KEYS:
            assert _bitwise(one[key][0], whole[key][t]), (key, t)         # alone = among 9


def test_columns_nobody_couples_to_never_enter_the_bias():
    """Q = 16, columns 8 .. 15 uncoupled and NaN in some used samples: ln_z, the moments of H and columns 0 .. 7 are bit for
    bit what the first 8 columns alone give."""
    temps, e, rungs, cols, f = _flat_problem(33, RAGGED, 16)
    targets, lam = _targets(temps, 4), pref.case_couplings(4, 16)
    lam[:, 8:] = 0.0
    dirty = cols.copy()
    dirty[8:, 1234] = np.nan
    dirty[11, [0, 2047, 2048, RAGGED - 1]] = [np.nan, np.inf, -np.inf, np.nan]
    got = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, lam, dirty)
    first = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, lam[:, :8], cols[:8])
    for key in ("ln_z", "hamiltonian_mean", "hamiltonian_var", "neff_fraction", "perturbation_mean"):
        assert np.all(np.isfinite(got[key])) and _bitwise(got[key], first[key]), key
    for key in ("mean", "var", "cov_hamiltonian"):
        assert _bitwise(got[key][:, :8], first[key]), key
        assert not np.any(np.isfinite(got[key][:, 8:])), key


# ------------------------------------------------------------------------------------------- 7. non-finite values


def test_samples_with_non_finite_energies_are_not_used():
    """Within the bounds of test 3, not bit for bit: removing samples moves the others to other lanes and tiles."""
    temps, e, rungs, cols, f = _flat_problem(8, RAGGED, 5, seed=23)
    dirty, dirty_cols = e.copy(), cols.copy()
    dirty[[3, 64, 2047, 2048, 4100, RAGGED - 1]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    dirty_cols[:, [3, 64, 4100]] = np.nan                     # of unused samples, coupled columns among them: never seen
    keep = np.isfinite(dirty)
    targets, lam = _targets(temps, 4), pref.case_couplings(4, 5)
    a = statistics.mbar_reweight_perturbed(dirty, rungs, temps, f, targets, lam, dirty_cols)
    b = statistics.mbar_reweight_perturbed(dirty[keep], rungs[keep], temps, f, targets, lam, dirty_cols[:, keep])
    for key in pref.KEYS:
        err = _relative(a[key], b[key], key)
        print("planted against removed, %s: largest relative difference %.3e" % (key, err))
        assert np.all(np.isfinite(a[key])) and err <= BOUND[key], key
    want = pref.reweight_perturbed(dirty, rungs, temps, f, targets, lam, dirty_cols, dtype=np.longdouble)
    _assert_errors("engine-less n=%d K=8 Q=5 P=4, 6 unused samples" % RAGGED, a, want)


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_value_of_a_coupled_column_stays_in_its_targets(value):
    temps, e, rungs, cols, f = _flat_problem(8, RAGGED, 5, seed=29)
    targets, lam = _targets(temps, 9), pref.case_couplings(9, 5)
    clean = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, lam, cols)
    bad = cols.copy()
    bad[2, 1234] = value                                      # a used sample
    got = statistics.mbar_reweight_perturbed(e, rungs, temps, f, targets, lam, bad)
    coupled = lam[:, 2] != 0
    assert coupled.sum() == 6 and coupled[:4].any() and (~coupled[:4]).any()      # both kinds inside one chunk of 4 targets
    others = [q for q in range(5) if q != 2]
    for key in pref.KEYS:
        assert not np.any(np.isfinite(got[key][coupled])), (key, value)           # every output of a target that couples to it
    for key in ("ln_z", "hamiltonian_mean", "hamiltonian_var", "neff_fraction"):
        assert _bitwise(got[key][~coupled], clean[key][~coupled]), (key, value)   # every other target keeps its bits
    for key in ("mean", "var", "cov_hamiltonian"):
        assert _bitwise(got[key][~coupled][:, others], clean[key][~coupled][:, others]), (key, value)
        assert not np.any(np.isfinite(got[key][~coupled][:, 2])), (key, value)    # ... but for the column itself, as today


# --------------------------------------------------------------------------------------------------- 8. error cases


def test_error_cases_through_the_engine_and_the_c_abi():
    lib = _capi.load()
    nul = [None] * 7
    one = (ctypes.c_double * 1)(1.0)
    zero = (ctypes.c_double * 1)(0.0)
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=128, temp=1.0)
    eng.record_energies(2)
    with pytest.raises(ValueError, match="observable store"):
        eng.reweight_perturbed([1.0], {}, f=[0.0])             # no observable store
    eng.record_observables(["real_0", "real_0_sq"])
    eng.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder"):
        eng.reweight_perturbed([1.0], {"real_0": 0.1}, f=[0.0])
    assert lib.me_mbar_reweight_perturbed(None, zero, one, zero, 1, *nul) == _capi.ME_ERR_INVALID
    lad = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=8 * 64, seed=5, temperatures=LADDER8)
    f8 = (ctypes.c_double * 8)()
    lad.record_energies(2)
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, zero, 1, *nul) == _capi.ME_ERR_STATE       # no records
    assert "no recorded energy samples" in _capi.last_error(lad._handle)
    lad.record_energy()
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, zero, 1, *nul) == _capi.ME_ERR_STATE       # no observable store
    assert "no recorded observables" in _capi.last_error(lad._handle)
    lad.record_observables(["real_0", "real_0_sq"])
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples"):
        lad.reweight_perturbed([1.0], {"real_0": 0.1}, f=np.zeros(8))                                      # no records
    lad.record_energy()
    two = (ctypes.c_double * 2)(0.1, float("nan"))
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, two, 1, *nul) == _capi.ME_ERR_INVALID      # a non-finite coupling
    assert "couplings must be finite" in _capi.last_error(lad._handle)
    two[1] = float("inf")
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, two, 1, *nul) == _capi.ME_ERR_INVALID
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, None, 1, *nul) == _capi.ME_ERR_INVALID     # couplings == NULL
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, two, 0, *nul) == _capi.ME_ERR_INVALID      # no target
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, zero, two, 1, *nul) == _capi.ME_ERR_INVALID     # T = 0
    two[1] = 0.0
    assert lib.me_mbar_reweight_perturbed(lad._handle, f8, one, two, 1, *nul) == _capi.ME_OK               # every output NULL
    for bad in (np.zeros((1, 3)), np.zeros((2, 3)), np.zeros(3), {"real_1": 1.0}, {"real_0": 1.0, 0: 1.0}, {"real_0": np.nan}, [[np.inf, 0.0]]):
        with pytest.raises(ValueError):
            lad.reweight_perturbed([1.0], bad, f=np.zeros(8))
    # the engine-less form: no columns, a seventeenth column, a non-finite coupling
    e3, r3 = (ctypes.c_double * 2)(1.0, 2.0), (ctypes.c_int32 * 2)(0, 1)
    t2, f2 = (ctypes.c_double * 2)(1.0, 2.0), (ctypes.c_double * 2)()
    obs = (ctypes.c_double * 34)()
    lam = (ctypes.c_double * 17)()
    args = (0, e3, r3, 2, t2, 2, f2, one)
    assert lib.me_mbar_reweight_perturbed_samples(*args, lam, 1, obs, 0, *nul) == _capi.ME_ERR_INVALID
    assert lib.me_mbar_reweight_perturbed_samples(*args, lam, 1, obs, 17, *nul) == _capi.ME_ERR_INVALID
    assert lib.me_mbar_reweight_perturbed_samples(*args, lam, 1, None, 1, *nul) == _capi.ME_ERR_INVALID
    assert lib.me_mbar_reweight_perturbed_samples(*args, None, 1, obs, 1, *nul) == _capi.ME_ERR_INVALID
    lam[1] = float("nan")
    assert lib.me_mbar_reweight_perturbed_samples(*args, lam, 1, obs, 2, *nul) == _capi.ME_ERR_INVALID
    assert lib.me_mbar_reweight_perturbed_samples(*args, lam, 1, obs, 1, *nul) == _capi.ME_OK              # (lam[1] is not read)


# ------------------------------------------------------------------------------------------------ 9. device physics


def test_closed_forms_of_the_quadratic_energy_in_a_field_and_with_a_changed_stiffness():
    """tests/test_mbar_perturbed_cpu.py's targets and harness on the device's results: 16 subsets of exact samples of E =
    |x|^2, ln_z(T, lambda) - ln_z(T, 0), <x_0>, <x_0^2> and Var x_0 at eight (T, lambda), 32 values within 5 standard errors."""
    results = []
    for e, rungs, cols in oref.iso_quadratic_subsets():
        out = statistics.mbar_free_energies(e, rungs, LADDER8)
        assert out["converged"]
        results.append(statistics.mbar_reweight_perturbed(e, rungs, LADDER8, out["f"], pref.PHYSICS_TEMPS, pref.PHYSICS_COUPLINGS, cols))
    print("largest deviation in standard errors", pref.check_physics(results))


# ---------------------------------------------------------------------------------------------------- 10. end to end


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_ladder_engine_end_to_end(dtype):
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0, 0.0], None, n_chains=8 * 64, seed=47, dtype=dtype, temperatures=LADDER8)
    eng.record_energies(16)
    eng.record_observables(["real_0", "real_0_sq"])
    for _ in range(16):
        eng.step_all(5)
        eng.replica_exchange()
        eng.record_energy()
    out = eng.reweight_perturbed([0.6, 1.0, 2.2], {"real_0": -0.3, "real_0_sq": [0.0, 0.2, 0.4]})       # solves first
    assert out["names"] == ("real_0", "real_0_sq") and out["couplings"].tolist() == [[-0.3, 0.0], [-0.3, 0.2], [-0.3, 0.4]]
    for key in ("ln_z", "hamiltonian_mean", "hamiltonian_var", "heat_capacity", "perturbation_mean", "neff_fraction", "temps"):
        assert out[key].shape == (3,) and np.all(np.isfinite(out[key])), key
    for key in ("mean", "var", "cov_hamiltonian", "dmean_dT", "couplings"):
        assert out[key].shape == (3, 2) and np.all(np.isfinite(out[key])), key
    assert np.all((out["neff_fraction"] > 0) & (out["neff_fraction"] <= 1)) and np.all(out["var"] >= 0)
    assert np.all(out["hamiltonian_var"] > 0)
    same = eng.reweight_perturbed(1.0, {"real_0_sq": [0.0, 0.2]})                    # one temperature for both targets
    assert same["temps"].tolist() == [1.0, 1.0] and same["ln_z"][1] < same["ln_z"][0]


def test_field_reweighting_demo():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import demo_field_reweighting as demo
    finally:
        sys.path.pop(0)
    got = demo.main(**demo.QUICK)
    out, exact = got["result"], got["exact"]
    assert out["names"] == ("real_0",) and out["couplings"][:, 0].tolist() == (-demo.FIELDS).tolist()
    assert exact.shape == (3, 3) and all(np.all(np.isfinite(out[key])) for key in pref.KEYS)
    assert np.all((out["neff_fraction"] > 0) & (out["neff_fraction"] <= 1))
