"""Asymptotic MBAR error bars on the GPU (csrc/me_mbar_cov.hip: the Gram matrix of the weight matrix on the matrix cores)
against the long-double restatement in tests/mbar_uncertainty_reference.py and against exact results.  Every figure is
printed before it is asserted (run with -s); profiles/mbar_uncertainty.txt holds the values measured on the MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as ref

pytestmark = pytest.mark.gpu
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
# (K, targets): one 16 x 16 tile; two tiles; C = 26 padded to 32; the 16- and 32-rung chunks with C = 39 padded to 48; two
# target chunks of 32 and 1 targets, C = 128 on the first
CASES = [(8, 0), (8, 1), (8, 9), (33, 3), (64, 33)]
# Per-term rounding of a term W_ni W_nj of G in units of 2^-53: exp_nonpos is within 1.5 ulp = 3 * 2^-53 of e^x
# (me_math64.h, tests/test_math64_cpu.py), twice for the two factors, plus 4 for the division by the mean and the products.
# This counts the error of the exponential's OUTPUT alone.  Its argument fma(-b, E, g) - d_n is itself rounded, a few
# 2^-53 times the magnitudes of b E, g and d_n (up to some tens here), which moves e^x by as many 2^-53 relative: c = 10 does
# NOT cover that.  The bound as a whole does, because N 2^-53 is the worst case of the summation and a sum of N = 6149
# non-negative terms added in any fixed order stays orders of magnitude below it.
TERM_ROUNDING = 2 * 3 + 4


def _gram_samples(energies, rungs, temps, f, targets):
    """me_mbar_gram_samples: (gram, column_counts, ln_z, mean_e, n_used)."""
    e = np.ascontiguousarray(energies, dtype=np.float64)
    r = np.ascontiguousarray(rungs, dtype=np.int32)
    t = np.ascontiguousarray(temps, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    c = t.size + 2 * tg.size
    gram, counts, ln_z, mean_e = np.zeros((c, c)), np.zeros(c), np.zeros(tg.size), np.zeros(tg.size)
    n_used = ctypes.c_int64()
    _capi.check(_capi.load().me_mbar_gram_samples(
        0, e.ctypes.data_as(DP), r.ctypes.data_as(IP), e.size, t.ctypes.data_as(DP), t.size, f.ctypes.data_as(DP),
        tg.ctypes.data_as(DP) if tg.size else None, tg.size, gram.ctypes.data_as(DP), counts.ctypes.data_as(DP),
        ln_z.ctypes.data_as(DP), mean_e.ctypes.data_as(DP), ctypes.byref(n_used)))
    return gram, counts, ln_z, mean_e, n_used.value


@functools.lru_cache(maxsize=None)
def _case(k, n_targets):
    """Inputs, the device's Gram matrix and the long-double reference of one case, computed once."""
    temps, energies, rungs = ref.synthetic(k)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-13)["f"]
    targets = ref.targets_for(temps, n_targets)
    dev = _gram_samples(energies, rungs, temps, f, targets)
    w, counts, ln_z, mean_e, shift = ref.weight_matrix(energies, rungs, temps, f, targets)
    return dict(temps=temps, energies=energies, rungs=rungs, f=f, targets=targets, dev=dev, w=w, counts=counts, ln_z=ln_z,
                mean_e=mean_e, shift=shift, gram=ref.gram(w))


def _computed(k, n_targets):
    """Mask of the entries of gram that are computed: everything but the blocks between targets of different chunks."""
    c = k + 2 * n_targets
    chunk = np.full(c, -1)
    chunk[k:] = (np.arange(2 * n_targets) // 2) // ((128 - k) // 2)
    return (chunk[:, None] == chunk[None, :]) | (chunk[:, None] < 0) | (chunk[None, :] < 0)


@pytest.mark.parametrize("k,n_targets", CASES)
def test_gram_against_the_long_double_reference(k, n_targets):
    """Entrywise |G_dev - G_ref| <= (N + c) 2^-53 G_ref: every term of an entry is >= 0, so N 2^-53 is the worst case of ANY
    summation order, and c = TERM_ROUNDING the rounding of one term's exponentials, division and products (see there for
    what it leaves to the N)."""
    case = _case(k, n_targets)
    gram, counts, _, _, n_used = case["dev"]
    assert n_used == ref.N_GRAM and np.array_equal(counts, np.asarray(case["counts"], dtype=np.float64))
    mask = _computed(k, n_targets)
    assert np.all(np.isnan(gram[~mask])) and np.all(np.isfinite(gram[mask]))
    g_ref = case["gram"]
    err = np.abs(gram.astype(ref.LD) - g_ref)[mask] / g_ref[mask]
    bound = (ref.N_GRAM + TERM_ROUNDING) * 2.0 ** -53
    print("K = %d, %d targets: largest relative error of G %.3e (bound %.3e)" % (k, n_targets, float(err.max()), bound))
    assert float(err.max()) <= bound


@pytest.mark.parametrize("k,n_targets", CASES)
def test_non_finite_samples_are_left_out(k, n_targets):
    """inf, -inf and nan at 1 % of the samples: everything equals the result on the array without them, bit for bit (the
    blocks between targets of different chunks are NaN in both)."""
    case = _case(k, n_targets)
    rng = np.random.default_rng(3)
    energies = case["energies"].copy()
    bad = rng.choice(energies.size, energies.size // 100, replace=False)
    energies[bad] = np.resize([np.inf, -np.inf, np.nan], bad.size)
    keep = np.isfinite(energies)
    with_bad = _gram_samples(energies, case["rungs"], case["temps"], case["f"], case["targets"])
    without = _gram_samples(energies[keep], case["rungs"][keep], case["temps"], case["f"], case["targets"])
    assert with_bad[4] == without[4] == int(keep.sum())
    for a, b in zip(with_bad[:4], without[:4]):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("k,n_targets", CASES)
def test_invariants(k, n_targets):
    case = _case(k, n_targets)
    gram, counts, ln_z, mean_e, _ = case["dev"]
    assert np.array_equal(gram, gram.T, equal_nan=True)
    ladder = gram[:, :k] @ counts[:k]                     # (the target columns have count 0)
    print("K = %d, %d targets: largest |G N - 1| %.3e" % (k, n_targets, np.abs(ladder - 1).max()))
    assert np.abs(ladder - 1).max() <= 1e-12
    if n_targets:
        rw = statistics.mbar_reweight(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])
        assert np.array_equal(ln_z, rw["ln_z"]) and np.array_equal(mean_e, rw["energy_mean"])


def _largest_relative_difference(got, want):
    worst = 0.0
    for a, b in zip(got, want):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        nz = b != 0
        if nz.any():
            worst = max(worst, float((np.abs(a - b)[nz] / np.abs(b)[nz]).max()))
    return worst


@pytest.mark.parametrize("k,n_targets", [(8, 0), (8, 1), (8, 9), (33, 3)])
def test_uncertainties_against_the_reference(k, n_targets):
    """The yardstick is the reference's own spread: its Gram route in float64 against its SVD route on the long-double W.  The
    device may differ from the SVD route by ten times that.  Measured on the MI355X: profiles/mbar_uncertainty.txt."""
    case = _case(k, n_targets)
    me64 = np.asarray(case["mean_e"], dtype=np.float64)
    want = ref.sigmas(ref.theta_svd(case["w"], case["counts"]), k, n_targets, me64, case["shift"])
    own = ref.sigmas(ref.theta_gram(case["gram"], case["counts"]), k, n_targets, me64, case["shift"])
    out = statistics.mbar_uncertainties(case["energies"], case["rungs"], case["temps"], case["f"],
                                        targets=case["targets"] if n_targets else None)
    got = (out["d_f"], out["d_f_matrix"]) + ((out["d_ln_z"], out["d_energy_mean"]) if n_targets else ((), ()))
    spread, err = _largest_relative_difference(own, want), _largest_relative_difference(got, want)
    print("K = %d, %d targets: reference Gram route against SVD route %.3e, device against SVD route %.3e" % (k, n_targets, spread, err))
    assert out["d_f"][0] == 0.0 and out["n_samples"] == ref.N_GRAM and out["theta"].shape == (k, k)
    assert err <= 10.0 * spread


def test_two_calls_agree_bit_for_bit():
    case = _case(33, 3)
    again = _gram_samples(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])
    assert np.array_equal(again[0], case["dev"][0], equal_nan=True)


def _ladder_engine(records=8):
    temps = np.array([0.6, 0.9, 1.4, 2.1])
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=4 * 64, seed=5, dtype="f64", temperatures=temps)
    eng.record_energies(records)
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
    a = eng.ladder_free_energy_uncertainties(f, targets=targets)
    b = statistics.mbar_uncertainties(samples, rungs, temps, f, targets=targets)
    assert set(a) == set(b) == {"theta", "d_f", "d_f_matrix", "n_samples", "temps", "ln_z", "d_ln_z", "energy_mean", "d_energy_mean"}
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    c = 4 + 2 * targets.size
    gram, counts = np.zeros((c, c)), np.zeros(c)
    eng._check(eng._lib.me_mbar_gram(eng._handle, f.ctypes.data_as(DP), targets.ctypes.data_as(DP), targets.size,
                                     gram.ctypes.data_as(DP), counts.ctypes.data_as(DP), None, None, None))
    assert np.array_equal(gram, _gram_samples(samples, rungs, temps, f, targets)[0])


def test_calibration_on_the_device():
    """The replicas of tests/test_mbar_uncertainty_cpu.py through the GPU; the same condition on the RMS z-scores."""
    exact_f, exact_lnz, exact_mean = ref.calibration_exact()
    rows = {name: [] for name in ("f", "d_f", "ln_z", "d_ln_z", "energy_mean", "d_energy_mean")}
    for energies, rungs in ref.calibration_replicas():
        f = statistics.mbar_free_energies(energies, rungs, ref.CAL_TEMPS, tol=1e-12)["f"]
        out = statistics.mbar_uncertainties(energies, rungs, ref.CAL_TEMPS, f, targets=ref.CAL_TARGETS)
        rows["f"].append(f[1:]), rows["d_f"].append(out["d_f"][1:])
        for name in ("ln_z", "d_ln_z", "energy_mean", "d_energy_mean"):
            rows[name].append(out[name])
    four = statistics.mbar_uncertainties(energies, rungs, ref.CAL_TEMPS, f, targets=ref.CAL_TARGETS, inefficiency=4.0)
    for name in ("d_f", "d_f_matrix", "d_ln_z", "d_energy_mean"):
        assert np.array_equal(four[name], 2.0 * out[name]), name
    lo, hi = ref.CAL_RMS_Z
    for name, rms in (("f", ref.rms_z(rows["f"], rows["d_f"], exact_f[1:])),
                      ("ln_z", ref.rms_z(rows["ln_z"], rows["d_ln_z"], exact_lnz, pooled=True)),
                      ("energy_mean", ref.rms_z(rows["energy_mean"], rows["d_energy_mean"], exact_mean, pooled=True))):
        print("rms z of %s on the device: %s" % (name, rms))
        assert np.all((rms >= lo) & (rms <= hi)), name


def test_refusals():
    plain = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=256, seed=5, dtype="f64", temp=1.0)
    plain.record_energies(1)
    plain.record_energy()
    statuses = []
    for call in (plain.ladder_free_energies, lambda: plain.ladder_free_energy_uncertainties(np.zeros(1))):
        with pytest.raises(_capi.MetropolisLibraryError) as no_ladder:
            call()
        statuses.append(no_ladder.value.status)
    assert statuses[0] == statuses[1]
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=256, seed=5, dtype="f64",
                              temperatures=[0.6, 0.9, 1.4, 2.1])
    statuses = []
    for call in (eng.ladder_free_energies, lambda: eng.ladder_free_energy_uncertainties(np.zeros(4))):
        with pytest.raises(_capi.MetropolisLibraryError) as no_records:
            call()
        statuses.append(no_records.value.status)
    assert statuses[0] == statuses[1]
    temps, energies, rungs = ref.synthetic(8, 2053)
    f = np.zeros(8)
    for bad in ([0.0], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            statistics.mbar_uncertainties(energies, rungs, temps, f, targets=bad)
        with pytest.raises(ValueError):
            eng.ladder_free_energy_uncertainties(np.zeros(4), targets=bad)
    for bad in (0.99, -2.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            statistics.mbar_uncertainties(energies, rungs, temps, f, inefficiency=bad)
        with pytest.raises(ValueError):
            eng.ladder_free_energy_uncertainties(np.zeros(4), inefficiency=bad)
    # more than 64 rungs: the Python layer refuses (ValueError), the C ABI reports ME_ERR_UNSUPPORTED (NotImplementedError)
    temps65 = np.linspace(0.5, 3.0, 65)
    rungs65 = (np.arange(2053) % 65).astype(np.int32)
    with pytest.raises(ValueError):
        statistics.mbar_uncertainties(energies, rungs65, temps65, np.zeros(65))
    with pytest.raises(NotImplementedError):
        _gram_samples(energies, rungs65, temps65, np.zeros(65), np.zeros(0))
