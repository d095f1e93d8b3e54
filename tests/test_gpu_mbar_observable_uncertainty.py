"""Asymptotic error bars of reweighted observables on the GPU (csrc/me_mbar_cov.hip, the observable form: the Gram matrix of
the weight matrix with observable-weighted columns on the matrix cores) against the long-double restatement in
tests/mbar_observable_uncertainty_reference.py and against exact results.  Every figure is printed before it is asserted (run
with -s); profiles/mbar_observable_uncertainty.txt holds the values measured on the MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_observable_uncertainty_reference as ref
from test_gpu_mbar_observables import BOUND as REWEIGHT_BOUND
from test_gpu_mbar_uncertainty import TERM_ROUNDING, _gram_samples

pytestmark = pytest.mark.gpu
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
# (K, targets, Q): one 16 x 16 tile; C = 16 exactly; C = 59, padded row 80; C = 128, the full launch; C = 67; two chunks of 3
# and 1 targets, C = 115 on the first
CASES = [(8, 1, 1), (8, 2, 3), (8, 3, 16), (8, 8, 14), (33, 2, 16), (64, 4, 16)]
# Per-term rounding of a term W_ni W_nj of G in units of 2^-53.  TERM_ROUNDING (tests/test_gpu_mbar_uncertainty.py) covers
# the two exponentials (3 each), the product and one energy factor.  An observable factor (A_qn - S_q) / (mean_tq - S_q) is
# applied as w * (A - S) / norm: one subtraction, one multiplication and one division, each rounded once, 3 per factor, and
# a term may carry two such factors (the reference takes the device's own S_q and mean_tq, so the normaliser and the shift
# themselves add nothing).  As there, the rounding of the exponential's ARGUMENT is left to the N of the bound.
OBS_TERM_ROUNDING = TERM_ROUNDING + 2 * 3


def _gram_observables(energies, rungs, temps, f, targets, columns):
    """me_mbar_gram_observables_samples: (gram, column_counts, ln_z, mean, shifts, n_used)."""
    e = np.ascontiguousarray(energies, dtype=np.float64)
    r = np.ascontiguousarray(rungs, dtype=np.int32)
    t = np.ascontiguousarray(temps, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    a = np.ascontiguousarray(np.atleast_2d(columns), dtype=np.float64)
    q = a.shape[0]
    c = t.size + tg.size * (1 + q)
    gram, counts, ln_z, mean, shifts = np.zeros((c, c)), np.zeros(c), np.zeros(tg.size), np.zeros((tg.size, q)), np.zeros(q)
    n_used = ctypes.c_int64()
    _capi.check(_capi.load().me_mbar_gram_observables_samples(
        0, e.ctypes.data_as(DP), r.ctypes.data_as(IP), e.size, t.ctypes.data_as(DP), t.size, a.ctypes.data_as(DP), q,
        f.ctypes.data_as(DP), tg.ctypes.data_as(DP), tg.size, gram.ctypes.data_as(DP), counts.ctypes.data_as(DP),
        ln_z.ctypes.data_as(DP), mean.ctypes.data_as(DP), shifts.ctypes.data_as(DP), ctypes.byref(n_used)))
    return gram, counts, ln_z, mean, shifts, n_used.value


@functools.lru_cache(maxsize=None)
def _inputs(k):
    temps, energies, rungs = uref.synthetic(k)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-13)["f"]
    return temps, energies, rungs, f, ref.synthetic_columns(energies, 16)


@functools.lru_cache(maxsize=None)
def _case(k, n_targets, q):
    """Inputs, the device's Gram matrix and the long-double reference (normalised with the device's own means and shifts) of
    one case, computed once."""
    temps, energies, rungs, f, columns = _inputs(k)
    columns = columns[:q]
    targets = uref.targets_for(temps, n_targets)
    dev = _gram_observables(energies, rungs, temps, f, targets, columns)
    w, counts, ln_z, mean, shifts = ref.weight_matrix_observables(energies, rungs, temps, f, targets, columns, means=dev[3],
                                                                  shifts=dev[4])
    return dict(temps=temps, energies=energies, rungs=rungs, f=f, targets=targets, columns=columns, dev=dev, w=w, counts=counts,
                ln_z=ln_z, mean=mean, shifts=shifts, gram=ref.gram(w))


def _chunk_of(k, n_targets, q):
    chunk = np.full(k + n_targets * (1 + q), -1)
    chunk[k:] = (np.arange(n_targets * (1 + q)) // (1 + q)) // ((128 - k) // (1 + q))
    return chunk


def _computed(k, n_targets, q):
    """Mask of the entries of gram that are computed: everything but the blocks between targets of different chunks."""
    chunk = _chunk_of(k, n_targets, q)
    return (chunk[:, None] == chunk[None, :]) | (chunk[:, None] < 0) | (chunk[None, :] < 0)


def _plain(k, n_targets, q):
    """Indices of the ladder and state columns here, and of the same columns of me_mbar_gram_samples."""
    here = np.concatenate([np.arange(k), k + (1 + q) * np.arange(n_targets)])
    there = np.concatenate([np.arange(k), k + 2 * np.arange(n_targets)])
    return here, there


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    return np.array_equal(_u64(a), _u64(b))


# ------------------------------------------------------------------------------------ 1. G against the long-double G
@pytest.mark.parametrize("k,n_targets,q", CASES)
def test_gram_against_the_long_double_reference(k, n_targets, q):
    """Entrywise |G_dev - G_ref| <= (N + c) 2^-53 G_ref on the computed entries: every term of an entry is >= 0, so N 2^-53 is
    the worst case of ANY summation order, and c = OBS_TERM_ROUNDING the rounding of one term (see there).  The means are
    compared separately: with me_mbar_reweight_observables_samples bit for bit, with the long-double reference under the
    bound of tests/test_gpu_mbar_observables.py.  That bound is a RELATIVE error, and the columns it was set on are built so
    that their means are no small differences.  Column 1 here (c = 0, pure noise) has a mean that is the difference of two
    weighted sums thirty to a hundred and thirty times its size, so a relative error of its mean says nothing about the
    kernel; its error -- like every column's -- is measured against sum_n W_na |A_qn|, the size of the terms of the sum,
    which for a column of one sign IS |mean|.  The columns that follow the energy (c > 0) are held to the bound both ways.
    Measured on the MI355X for column 1: 2.50e-15 (K = 33) and 2.17e-15 (K = 64) of |mean| against the 2.03e-15 of the bound, 2.3e-17 and 6.1e-17 of sum W |A|;
    every other column is below 3.5e-16 either way (profiles/mbar_observable_uncertainty.txt)."""
    case = _case(k, n_targets, q)
    gram, counts, ln_z, mean, shifts, n_used = case["dev"]
    assert n_used == uref.N_GRAM and np.array_equal(counts, np.asarray(case["counts"], dtype=np.float64))
    mask = _computed(k, n_targets, q)
    assert np.all(np.isnan(gram[~mask])) and np.all(np.isfinite(gram[mask]))
    g_ref = case["gram"]
    err = np.abs(gram.astype(ref.LD) - g_ref)[mask] / g_ref[mask]
    bound = (uref.N_GRAM + OBS_TERM_ROUNDING) * 2.0 ** -53
    print("K = %d, %d targets, Q = %d: largest relative error of G %.3e (bound %.3e)" % (k, n_targets, q, float(err.max()), bound))
    rw = statistics.mbar_reweight_observables(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"],
                                              case["columns"])
    want = case["mean"]
    states = case["w"][:, k + (1 + q) * np.arange(n_targets)]                     # (every energy is finite: all samples)
    size = states.T @ np.abs(case["columns"]).astype(ref.LD).T                    # sum_n W_na |A_qn|, (T, Q)
    of_mean = (np.abs(mean.astype(ref.LD) - want) / np.abs(want)).max(axis=0).astype(np.float64)
    of_size = (np.abs(mean.astype(ref.LD) - want) / size).max(axis=0).astype(np.float64)
    follows_energy = np.arange(q) != 1                                            # (ref.synthetic_columns: c_1 = 0)
    print("    error of the means against long double per column, relative to |mean|:\n      %s\n    relative to sum W |A|:\n      %s"
          "\n    (bound %.3e)" % (of_mean, of_size, REWEIGHT_BOUND["mean"]))
    assert np.array_equal(shifts, ref.column_shifts(case["energies"], case["columns"]))
    assert np.array_equal(ln_z, statistics.mbar_reweight(case["energies"], case["rungs"], case["temps"], case["f"],
                                                         case["targets"])["ln_z"])
    assert float(err.max()) <= bound
    assert _bitwise(mean, rw["mean"])
    assert np.all(of_size <= REWEIGHT_BOUND["mean"]) and np.all(of_mean[follows_energy] <= REWEIGHT_BOUND["mean"])


# ------------------------------------------------------------------------------------------------------- 2. invariants
@pytest.mark.parametrize("k,n_targets,q", CASES)
def test_invariants(k, n_targets, q):
    case = _case(k, n_targets, q)
    gram, counts = case["dev"][:2]
    assert _bitwise(gram, gram.T)
    ladder = gram[:, :k] @ counts[:k]                     # (the target columns have count 0)
    print("K = %d, %d targets, Q = %d: largest |G N - 1| %.3e" % (k, n_targets, q, np.abs(ladder - 1).max()))
    assert np.abs(ladder - 1).max() <= 1e-12
    # the ladder block, ladder x state and state x state: me_mbar_gram_samples' entries, where both compute them
    plain = _gram_samples(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])[0]
    here, there = _plain(k, n_targets, q)
    a, b = gram[np.ix_(here, here)], plain[np.ix_(there, there)]
    both = np.isfinite(a) & np.isfinite(b)
    assert both[:k].all() and both[:, :k].all() and both.diagonal().all()
    assert np.array_equal(_u64(a)[both], _u64(b)[both])


@pytest.mark.parametrize("k,n_targets,column", [(8, 3, 0), (8, 3, 1), (8, 3, 15), (33, 2, 7)])
def test_a_column_alone_has_the_bits_it_has_among_sixteen(k, n_targets, column):
    case = _case(k, n_targets, 16)
    among = case["dev"][0]
    alone = _gram_observables(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], case["columns"][column])[0]
    plain16, _ = _plain(k, n_targets, 16)
    plain1, _ = _plain(k, n_targets, 1)
    for t in range(n_targets):
        c16, c1 = k + 17 * t + 1 + column, k + 2 * t + 1
        assert _bitwise(alone[c1, plain1], among[c16, plain16])          # against every ladder and state column
        assert _bitwise(alone[c1, c1], among[c16, c16])
    assert _bitwise(alone[np.ix_(plain1, plain1)], among[np.ix_(plain16, plain16)])


# ------------------------------------------------------------------------------------------- 3. non-finite energies
@pytest.mark.parametrize("k,n_targets,q", CASES)
def test_non_finite_energies_are_left_out(k, n_targets, q):
    """inf, -inf and nan at 1 % of the energies: everything equals the result on the arrays without those samples, bit for
    bit (the blocks between targets of different chunks are NaN in both)."""
    case = _case(k, n_targets, q)
    rng = np.random.default_rng(3)
    energies = case["energies"].copy()
    bad = rng.choice(energies.size, energies.size // 100, replace=False)
    energies[bad] = np.resize([np.inf, -np.inf, np.nan], bad.size)
    keep = np.isfinite(energies)
    columns = case["columns"].copy()
    columns[:, bad[::2]] = np.nan                          # of unused samples: never seen
    with_bad = _gram_observables(energies, case["rungs"], case["temps"], case["f"], case["targets"], columns)
    without = _gram_observables(energies[keep], case["rungs"][keep], case["temps"], case["f"], case["targets"], columns[:, keep])
    assert with_bad[5] == without[5] == int(keep.sum())
    mask = _computed(k, n_targets, q)
    assert np.all(np.isfinite(with_bad[0][mask])) and np.all(np.isnan(with_bad[0][~mask]))
    for a, b in zip(with_bad[:5], without[:5]):
        assert _bitwise(a, b)


# ------------------------------------------------------------------------------------------ 4. a non-finite observable
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_observable_stays_in_its_column(value):
    k, n_targets, q, column = 8, 3, 16, 5
    case = _case(k, n_targets, q)
    clean = case["dev"][0]
    columns = case["columns"].copy()
    columns[column, 1234] = value                          # a used sample
    got = _gram_observables(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], columns)[0]
    poisoned = np.zeros(clean.shape[0], dtype=bool)
    poisoned[k + (1 + q) * np.arange(n_targets) + 1 + column] = True
    touched = poisoned[:, None] | poisoned[None, :]
    assert np.all(np.isnan(got[touched]))
    assert np.array_equal(_u64(got)[~touched], _u64(clean)[~touched])
    args = (case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])
    want = statistics.mbar_observable_uncertainties(*args, case["columns"])
    out = statistics.mbar_observable_uncertainties(*args, columns)
    nan_cov = np.zeros((n_targets, q, q), dtype=bool)
    nan_cov[:, column, :] = nan_cov[:, :, column] = True
    assert np.array_equal(np.isnan(out["mean_cov"]), nan_cov)
    assert np.array_equal(np.isnan(out["d_mean"]), np.diagonal(nan_cov, axis1=1, axis2=2))
    assert not np.any(np.isfinite(out["mean"][:, column]))
    assert np.all(np.isfinite(want["d_mean"])) and np.all(np.isfinite(want["mean_cov"]))
    # the other columns: two float64 routes to Theta (with and without the poisoned columns): the rule of ref.covariances
    theta = ref.theta_svd(case["w"], case["counts"])
    _, scale = ref.covariances(theta, k, n_targets, q, case["dev"][3], case["dev"][4])
    bound = ref.route_bound(case["w"], case["counts"])
    err = (np.abs(out["mean_cov"] - want["mean_cov"]) / scale)[~nan_cov]
    others = [j for j in range(q) if j != column]
    err_d = np.abs(out["d_mean"] ** 2 - want["d_mean"] ** 2)[:, others] / np.diagonal(scale, axis1=1, axis2=2)[:, others]
    print("a %s in column %d: the other entries of mean_cov move by %.3e of their scale, d_mean^2 by %.3e (bound %.3e)"
          % (value, column, err.max(), err_d.max(), 4 * bound))
    assert err.max() <= 4 * bound and err_d.max() <= 4 * bound
    assert _bitwise(out["mean"][:, others], want["mean"][:, others]) and _bitwise(out["ln_z"], want["ln_z"])


# --------------------------------------------------------------------------------- 5. d_mean and mean_cov against the SVD route
def _largest_relative_difference(got, want):
    worst = 0.0
    for a, b in zip(got, want):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        nz = b != 0
        worst = max(worst, float((np.abs(a - b)[nz] / np.abs(b)[nz]).max()))
    return worst


@pytest.mark.parametrize("k,n_targets,q", [(8, 1, 1), (8, 2, 3), (8, 3, 16), (33, 2, 16)])
def test_uncertainties_against_the_reference(k, n_targets, q):
    """The yardstick is the reference's own spread: its Gram route in float64 against its SVD route on the long-double W.  The
    device may differ from the SVD route by ten times that (the rule of tests/test_gpu_mbar_uncertainty.py)."""
    case = _case(k, n_targets, q)
    mean, shifts = case["dev"][3], case["dev"][4]
    want = ref.sigmas(ref.theta_svd(case["w"], case["counts"]), k, n_targets, q, mean, shifts)
    own = ref.sigmas(ref.theta_gram(case["gram"], case["counts"]), k, n_targets, q, mean, shifts)
    out = statistics.mbar_observable_uncertainties(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"],
                                                   case["columns"])
    got = (out["d_mean"], out["mean_cov"])
    spread, err = _largest_relative_difference(own, want), _largest_relative_difference(got, want)
    print("K = %d, %d targets, Q = %d: reference Gram route against SVD route %.3e, device against SVD route %.3e"
          % (k, n_targets, q, spread, err))
    assert out["n_samples"] == uref.N_GRAM and out["names"] == tuple(range(q)) and _bitwise(out["mean"], mean)
    assert out["d_mean"].shape == (n_targets, q) and out["mean_cov"].shape == (n_targets, q, q)
    assert set(out) == {"temps", "names", "mean", "d_mean", "mean_cov", "ln_z", "d_ln_z", "n_samples"}
    assert err <= 10.0 * spread


# ------------------------------------------------------------------------------------------------------ 6. forms agree
def test_two_calls_agree_bit_for_bit():
    case = _case(33, 2, 16)
    again = _gram_observables(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], case["columns"])
    for a, b in zip(again[:5], case["dev"][:5]):
        assert _bitwise(a, b)


def _ladder_engine(records=8, observables=("real_0", "abs_real_0", "real_0_sq")):
    temps = np.array([0.6, 0.9, 1.4, 2.1])
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=4 * 64, seed=5, dtype="f64", temperatures=temps)
    eng.record_energies(records)
    if observables:
        eng.record_observables(list(observables))
    for _ in range(records):
        eng.step_all(10)
        eng.record_energy()
    return eng, temps


def test_engine_form_equals_the_engine_less_form():
    eng, temps = _ladder_engine()
    f = eng.ladder_free_energies()["f"]
    targets = np.array([0.7, 1.9])
    samples = eng.energy_samples()
    rungs = np.tile(np.arange(eng.n_chains) // 64, samples.shape[0])
    columns = eng.observable_samples().transpose(1, 0, 2).reshape(3, -1)
    a = eng.observable_uncertainties(targets, f)
    b = statistics.mbar_observable_uncertainties(samples, rungs, temps, f, targets, columns)
    assert a["names"] == ("real_0", "abs_real_0", "real_0_sq") and b["names"] == (0, 1, 2)
    assert np.all(np.isfinite(a["d_mean"])) and np.all(a["d_mean"] > 0)
    for key in ("temps", "mean", "d_mean", "mean_cov", "ln_z", "d_ln_z", "n_samples"):
        assert _bitwise(a[key], b[key]), key
    solved = eng.observable_uncertainties(targets)            # f = None solves first
    assert _bitwise(solved["mean"], eng.reweight_observables(targets)["mean"])
    c = 4 + targets.size * 4
    gram, counts = np.zeros((c, c)), np.zeros(c)
    eng._check(eng._lib.me_mbar_gram_observables(eng._handle, f.ctypes.data_as(DP), targets.ctypes.data_as(DP), targets.size,
                                                 gram.ctypes.data_as(DP), counts.ctypes.data_as(DP), None, None, None, None))
    less = _gram_observables(samples, rungs, temps, f, targets, columns)
    assert _bitwise(gram, less[0]) and np.array_equal(counts, less[1])


# ------------------------------------------------------------------------------------------ 7. calibration on the device
def test_calibration_on_the_device():
    """The subsets of tests/test_mbar_observable_uncertainty_cpu.py through the GPU; the same band for the nine RMS z-scores."""
    means, d_means = [], []
    for energies, rungs, cols in ref.calibration_subsets():
        f = statistics.mbar_free_energies(energies, rungs, ref.LADDER8, tol=1e-12)["f"]
        out = statistics.mbar_observable_uncertainties(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols)
        means.append(out["mean"]), d_means.append(out["d_mean"])
    four = statistics.mbar_observable_uncertainties(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols, inefficiency=4.0)
    assert np.array_equal(four["d_mean"], 2.0 * out["d_mean"]) and np.array_equal(four["mean_cov"], 4.0 * out["mean_cov"])
    assert np.array_equal(four["d_ln_z"], 2.0 * out["d_ln_z"])
    rms = ref.calibration_rms_z(means, d_means)
    print("rms z of the means on the device (targets x columns):\n%s" % rms)
    lo, hi = uref.CAL_RMS_Z
    assert np.all((rms >= lo) & (rms <= hi))


# ------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals():
    no_store, _ = _ladder_engine(records=1, observables=None)
    with pytest.raises(ValueError, match="no observable store"):
        no_store.observable_uncertainties([1.0], np.zeros(4))
    gram, counts, f4, t1 = np.zeros((9, 9)), np.zeros(9), np.zeros(4), np.ones(1)
    assert no_store._lib.me_mbar_gram_observables(no_store._handle, f4.ctypes.data_as(DP), t1.ctypes.data_as(DP), 1,
                                                  gram.ctypes.data_as(DP), counts.ctypes.data_as(DP), None, None, None,
                                                  None) == _capi.ME_ERR_STATE
    plain = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=256, seed=5, dtype="f64", temp=1.0)
    plain.record_energies(1)
    plain.record_observables(["real_0"])
    plain.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder") as no_ladder:
        plain.observable_uncertainties([1.0], f=[0.0])
    assert no_ladder.value.status == _capi.ME_ERR_STATE
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=256, seed=5, dtype="f64",
                              temperatures=[0.6, 0.9, 1.4, 2.1])
    eng.record_energies(1)
    eng.record_observables(["real_0"])
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples") as no_records:
        eng.observable_uncertainties([1.0], np.zeros(4))
    assert no_records.value.status == _capi.ME_ERR_STATE
    temps, energies, rungs = uref.synthetic(8, 2053)
    f, cols = np.zeros(8), np.ones((2, 2053))
    for bad in ([], [0.0], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            statistics.mbar_observable_uncertainties(energies, rungs, temps, f, bad, cols)
        with pytest.raises(ValueError):
            eng.observable_uncertainties(bad, np.zeros(4))
    for bad in (0.99, -2.0, np.nan, np.inf, [1.0, 0.5], [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError):
            statistics.mbar_observable_uncertainties(energies, rungs, temps, f, [1.0], cols, inefficiency=bad)
    for bad in (0.99, np.nan, [1.0, 1.0]):
        with pytest.raises(ValueError):
            eng.observable_uncertainties([1.0], np.zeros(4), inefficiency=bad)
    # no target and Q = 17 through the C ABI: ME_ERR_INVALID (ValueError)
    with pytest.raises(ValueError):
        _gram_observables(energies, rungs, temps, f, np.zeros(0), cols)
    with pytest.raises(ValueError):
        statistics.mbar_observable_uncertainties(energies, rungs, temps, f, [1.0], np.ones((17, 2053)))
    with pytest.raises(ValueError):
        _gram_observables(energies, rungs, temps, f, [1.0], np.ones((17, 2053)))
    # more than 64 rungs: the Python layer refuses (ValueError), the C ABI reports ME_ERR_UNSUPPORTED (NotImplementedError)
    temps65 = np.linspace(0.5, 3.0, 65)
    rungs65 = (np.arange(2053) % 65).astype(np.int32)
    with pytest.raises(ValueError):
        statistics.mbar_observable_uncertainties(energies, rungs65, temps65, np.zeros(65), [1.0], cols)
    with pytest.raises(NotImplementedError):
        _gram_observables(energies, rungs65, temps65, np.zeros(65), [1.0], cols)
