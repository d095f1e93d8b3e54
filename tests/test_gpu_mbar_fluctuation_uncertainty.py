"""Asymptotic error bars of reweighted variances, heat capacities and energy covariances on the GPU (csrc/me_mbar_cov.hip, the
fluctuation form: the Gram matrix of the weight matrix with second-moment columns formed in registers) against the long-double
restatement in tests/mbar_fluctuation_uncertainty_reference.py, against the two existing forms bit for bit, and against exact
results.  Every figure is printed before it is asserted (run with -s); profiles/mbar_fluctuation_uncertainty.txt holds the
values measured on the MI355X."""
import ctypes
import functools

import numpy as np
import pytest

import metropolisengine_amd as me
from metropolisengine_amd import _capi, statistics
import mbar_uncertainty_reference as uref
import mbar_fluctuation_uncertainty_reference as ref
from test_gpu_mbar_uncertainty import TERM_ROUNDING, _gram_samples
from test_gpu_mbar_observable_uncertainty import _gram_observables

pytestmark = pytest.mark.gpu
DP, IP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
# (K, targets, Q): C = 11, one tile, no observable LDS; C = 20; C = 59, padded row 80; C = 128 exactly, the full launch; C =
# 78; two chunks of 2 and 1 targets; one target per chunk, C = 115
CASES = [(8, 1, 0), (8, 2, 1), (8, 1, 16), (8, 8, 4), (33, 3, 4), (8, 3, 16), (64, 2, 16)]
# Per-term rounding of a term W_ni W_nj of G in units of 2^-53, by the rule at OBS_TERM_ROUNDING
# (tests/test_gpu_mbar_observable_uncertainty.py): TERM_ROUNDING covers the two exponentials, the product and one energy
# factor; to it come the roundings of the factors of the two columns of the term.  The longest fill expression here is
# w * ((a - S) * (es - shift)) / norm: two subtractions, the product of the two, the multiplication by w and the division, 5
# roundings per factor (E'^2 and A'^2 subtract once but are counted alike; E' and A' have 3), and a term may carry two such
# factors: 2 * 5 = 10.  The reference takes the device's own shifts and normalisers, so those add nothing.
FLUCT_TERM_ROUNDING = TERM_ROUNDING + 2 * 5
OUTPUTS = ("gram", "counts", "ln_z", "moments", "energy_shift", "shifts", "mean_e", "var_e", "mean", "var", "cov_energy")


def _gram_fluctuations(energies, rungs, temps, f, targets, columns=None):
    """me_mbar_gram_fluctuations_samples: a dictionary over OUTPUTS, and n_used."""
    e = np.ascontiguousarray(energies, dtype=np.float64)
    r = np.ascontiguousarray(rungs, dtype=np.int32)
    t = np.ascontiguousarray(temps, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    tg = np.ascontiguousarray(targets, dtype=np.float64)
    a = np.zeros((0, e.size)) if columns is None else np.ascontiguousarray(np.atleast_2d(columns), dtype=np.float64)
    q, n = a.shape[0], tg.size
    c = t.size + n * (3 + 3 * q)
    out = dict(gram=np.zeros((c, c)), counts=np.zeros(c), ln_z=np.zeros(n), moments=np.zeros((n, 2 + 3 * q)), energy_shift=np.zeros(1),
               shifts=np.zeros(q), mean_e=np.zeros(n), var_e=np.zeros(n), mean=np.zeros((n, q)), var=np.zeros((n, q)),
               cov_energy=np.zeros((n, q)))
    n_used = ctypes.c_int64()
    _capi.check(_capi.load().me_mbar_gram_fluctuations_samples(
        0, e.ctypes.data_as(DP), r.ctypes.data_as(IP), e.size, t.ctypes.data_as(DP), t.size, a.ctypes.data_as(DP) if q else None, q,
        f.ctypes.data_as(DP), tg.ctypes.data_as(DP), n, *(out[key].ctypes.data_as(DP) if out[key].size else None for key in OUTPUTS),
        ctypes.byref(n_used)))
    out["n_used"] = n_used.value
    return out


@functools.lru_cache(maxsize=None)
def _inputs(k):
    temps, energies, rungs = uref.synthetic(k)
    f = statistics.mbar_free_energies(energies, rungs, temps, tol=1e-13)["f"]
    return temps, energies, rungs, f, ref.synthetic_columns(energies, 16)


@functools.lru_cache(maxsize=None)
def _case(k, n_targets, q):
    """Inputs, the device's outputs and the long-double reference (normalised with the device's own moments and shifts) of one
    case, computed once."""
    temps, energies, rungs, f, columns = _inputs(k)
    columns = columns[:q]
    targets = uref.targets_for(temps, n_targets)
    dev = _gram_fluctuations(energies, rungs, temps, f, targets, columns if q else None)
    w, counts, ln_z, moments, _, _ = ref.weight_matrix_fluctuations(energies, rungs, temps, f, targets, columns if q else None,
                                                                   moments=dev["moments"], energy_shift=dev["energy_shift"][0],
                                                                   shifts=dev["shifts"])
    return dict(temps=temps, energies=energies, rungs=rungs, f=f, targets=targets, columns=columns, dev=dev, w=w, counts=counts,
                ln_z=ln_z, moments=moments, gram=ref.gram(w))


def _chunk_of(k, n_targets, q):
    per = 3 + 3 * q
    chunk = np.full(k + n_targets * per, -1)
    chunk[k:] = (np.arange(n_targets * per) // per) // ((128 - k) // per)
    return chunk


def _computed(k, n_targets, q):
    """Mask of the entries of gram that are computed: everything but the blocks between targets of different chunks."""
    chunk = _chunk_of(k, n_targets, q)
    return (chunk[:, None] == chunk[None, :]) | (chunk[:, None] < 0) | (chunk[None, :] < 0)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_u64(a), _u64(b))


def _same_bits_where_both(a, b):
    """The entries both forms compute (their chunks of targets differ) agree bit for bit; returns how many there are."""
    both = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(_u64(a)[both], _u64(b)[both])
    return both


# ------------------------------------------------------------------------------------ 1. G against the long-double G
@pytest.mark.parametrize("k,n_targets,q", CASES)
def test_gram_against_the_long_double_reference(k, n_targets, q):
    """Entrywise |G_dev - G_ref| <= (N + c) 2^-53 G_ref on the computed entries: every term of an entry is >= 0 (every factor is
    >= 1 by the shifts), so N 2^-53 is the worst case of ANY summation order, and c = FLUCT_TERM_ROUNDING the rounding of one
    term (see there).  The values come back bit for bit as the two reweighting functions give them, and the normalisers are
    those values recombined."""
    case = _case(k, n_targets, q)
    dev = case["dev"]
    gram = dev["gram"]
    assert dev["n_used"] == uref.N_GRAM and np.array_equal(dev["counts"], np.asarray(case["counts"], dtype=np.float64))
    mask = _computed(k, n_targets, q)
    assert np.all(np.isnan(gram[~mask])) and np.all(np.isfinite(gram[mask]))
    g_ref = case["gram"]
    err = np.abs(gram.astype(ref.LD) - g_ref)[mask] / g_ref[mask]
    bound = (uref.N_GRAM + FLUCT_TERM_ROUNDING) * 2.0 ** -53
    own = np.abs(dev["moments"].astype(ref.LD) - case["moments"]) / case["moments"]
    print("K = %d, %d targets, Q = %d: largest relative error of G %.3e (bound %.3e); the normalisers against long double %.3e"
          % (k, n_targets, q, float(err.max()), bound, float(own.max())))
    args = (case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])
    rw = statistics.mbar_reweight(*args)
    assert dev["energy_shift"][0] == case["energies"].min() - 1.0
    assert _bitwise(dev["ln_z"], rw["ln_z"]) and _bitwise(dev["mean_e"], rw["energy_mean"]) and _bitwise(dev["var_e"], rw["energy_var"])
    m_e = dev["mean_e"] - dev["energy_shift"][0]
    assert _bitwise(dev["moments"][:, 0], m_e)
    assert np.all(np.abs(dev["moments"][:, 1] - (dev["var_e"] + m_e * m_e)) <= 2.0 ** -52 * dev["moments"][:, 1])
    if q:
        ro = statistics.mbar_reweight_observables(*args, case["columns"])
        assert np.array_equal(dev["shifts"], ref.column_shifts(case["energies"], case["columns"]))
        for key in ("mean", "var", "cov_energy"):
            assert _bitwise(dev[key], ro[key]), key
        m_a = dev["mean"] - dev["shifts"][None, :]
        assert _bitwise(dev["moments"][:, 2::3], m_a)
        for got, want in ((dev["moments"][:, 3::3], dev["var"] + m_a * m_a), (dev["moments"][:, 4::3], dev["cov_energy"] + m_a * m_e[:, None])):
            assert np.all(np.abs(got - want) <= 2.0 ** -52 * got)
    assert float(case["w"].min()) >= 0.0
    assert float(err.max()) <= bound


# ------------------------------------------------------------------------------ 2. bitwise ties to the existing forms
@pytest.mark.parametrize("k,n_targets,q", CASES)
def test_bitwise_ties_to_the_existing_forms(k, n_targets, q):
    case = _case(k, n_targets, q)
    gram, counts = case["dev"]["gram"], case["dev"]["counts"]
    per, t = 3 + 3 * q, np.arange(n_targets)
    assert _bitwise(gram, gram.T)
    ladder = gram[:, :k] @ counts[:k]                     # (the target columns have count 0)
    print("K = %d, %d targets, Q = %d: largest |G N - 1| %.3e" % (k, n_targets, q, np.abs(ladder - 1).max()))
    assert np.abs(ladder - 1).max() <= 1e-12
    mask = _computed(k, n_targets, q)
    # ladder, state and E' columns: the energy form's ladder, state and energy columns
    plain = _gram_samples(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])[0]
    here = np.concatenate([np.arange(k), np.stack([k + per * t, k + per * t + 1], axis=1).ravel()])
    there = np.concatenate([np.arange(k), k + np.arange(2 * n_targets)])
    a, b = gram[np.ix_(here, here)], plain[np.ix_(there, there)]
    both = _same_bits_where_both(a, b)
    assert np.array_equal(both, mask[np.ix_(here, here)])               # (the energy form has all these targets in one chunk)
    if q == 0:
        return
    # ladder, state and A'_q columns: the observable form's
    obs = _gram_observables(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], case["columns"])[0]
    block = np.concatenate([[0], 3 + 3 * np.arange(q)])
    here = np.concatenate([np.arange(k), (k + per * t[:, None] + block[None, :]).ravel()])
    there = np.concatenate([np.arange(k), k + np.arange((1 + q) * n_targets)])
    a, b = gram[np.ix_(here, here)], obs[np.ix_(there, there)]
    both = _same_bits_where_both(a, b)
    assert np.array_equal(both, mask[np.ix_(here, here)])               # (the observable form's chunks hold all of these)


# ------------------------------------------------------------------ 3. a column alone and among sixteen; two calls
@pytest.mark.parametrize("k,n_targets,column", [(8, 3, 0), (8, 3, 1), (8, 3, 15), (64, 2, 7)])
def test_a_column_alone_has_the_bits_it_has_among_sixteen(k, n_targets, column):
    case = _case(k, n_targets, 16)
    among = case["dev"]
    alone = _gram_fluctuations(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], case["columns"][column])
    t = np.arange(n_targets)
    block1 = np.arange(6)                                                  # state, E', E'^2 and the column's three
    block16 = np.concatenate([np.arange(3), 3 + 3 * column + np.arange(3)])
    one = np.concatenate([np.arange(k), (k + 6 * t[:, None] + block1[None, :]).ravel()])
    sixteen = np.concatenate([np.arange(k), (k + 51 * t[:, None] + block16[None, :]).ravel()])
    a, b = alone["gram"][np.ix_(one, one)], among["gram"][np.ix_(sixteen, sixteen)]
    both = _same_bits_where_both(a, b)
    assert np.array_equal(both, _computed(k, n_targets, 16)[np.ix_(sixteen, sixteen)]) and np.all(np.isfinite(a))
    assert _bitwise(alone["moments"], among["moments"][:, np.concatenate([[0, 1], 2 + 3 * column + np.arange(3)])])
    for key in ("mean", "var", "cov_energy"):
        assert _bitwise(alone[key][:, 0], among[key][:, column]), key


def test_two_calls_agree_bit_for_bit():
    case = _case(33, 3, 4)
    again = _gram_fluctuations(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], case["columns"])
    for key in OUTPUTS:
        assert _bitwise(again[key], case["dev"][key]), key


# ------------------------------------------------------------------------------------------- 4. non-finite energies
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
    with_bad = _gram_fluctuations(energies, case["rungs"], case["temps"], case["f"], case["targets"], columns if q else None)
    without = _gram_fluctuations(energies[keep], case["rungs"][keep], case["temps"], case["f"], case["targets"],
                                 columns[:, keep] if q else None)
    assert with_bad["n_used"] == without["n_used"] == int(keep.sum())
    mask = _computed(k, n_targets, q)
    assert np.all(np.isfinite(with_bad["gram"][mask])) and np.all(np.isnan(with_bad["gram"][~mask]))
    for key in OUTPUTS:
        assert _bitwise(with_bad[key], without[key]), key


# ------------------------------------------------------------------------------------------ 5. a non-finite observable
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_observable_stays_in_its_columns(value):
    k, n_targets, q, column = 8, 3, 16, 5
    case = _case(k, n_targets, q)
    clean = case["dev"]
    columns = case["columns"].copy()
    columns[column, 1234] = value                          # a used sample
    got = _gram_fluctuations(case["energies"], case["rungs"], case["temps"], case["f"], case["targets"], columns)
    poisoned = np.zeros(clean["gram"].shape[0], dtype=bool)
    poisoned[(k + 51 * np.arange(n_targets)[:, None] + 3 + 3 * column + np.arange(3)[None, :]).ravel()] = True
    touched = poisoned[:, None] | poisoned[None, :]
    assert np.all(np.isnan(got["gram"][touched]))
    assert np.array_equal(_u64(got["gram"])[~touched], _u64(clean["gram"])[~touched])
    own = np.zeros(2 + 3 * q, dtype=bool)
    own[2 + 3 * column:5 + 3 * column] = True
    assert np.all(np.isnan(got["moments"][:, own])) and _bitwise(got["moments"][:, ~own], clean["moments"][:, ~own])
    args = (case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])
    want = statistics.mbar_fluctuation_uncertainties(*args, case["columns"])
    out = statistics.mbar_fluctuation_uncertainties(*args, columns)
    others = np.arange(q) != column
    for key in ("mean", "var", "cov_energy", "dmean_dT"):
        assert not np.any(np.isfinite(out[key][:, column])), key
        assert np.all(np.isnan(out["d_" + key][:, column])), key
        assert _bitwise(out[key][:, others], want[key][:, others]), key
        assert np.all(np.isfinite(want["d_" + key])) and np.all(np.isfinite(out["d_" + key][:, others])), key
    for key in ("energy_mean", "energy_var", "heat_capacity"):
        assert _bitwise(out[key], want[key]), key
    # the errors of everything else: two float64 routes to Theta (with and without the poisoned columns), the rule of
    # ref.variances
    _, scale = ref.variances(ref.theta_svd(case["w"], case["counts"]), k, n_targets, q, clean["moments"])
    bound = ref.route_bound(case["w"], case["counts"])
    for key in ref.KEYS:
        keep = (slice(None), others) if out[key].ndim == 2 else slice(None)
        err = (np.abs(out[key] ** 2 - want[key] ** 2) / scale[key])[keep]
        print("a %s in column %d: %s^2 elsewhere moves by %.3e of its scale (bound %.3e)" % (value, column, key, err.max(), 4 * bound))
        assert err.max() <= 4 * bound, key


# --------------------------------------------------------------------------------- 6. the sigmas against the SVD route
def _largest_relative_difference(got, want):
    worst = 0.0
    for a, b in zip(got, want):
        a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
        nz = b != 0
        if nz.any():
            worst = max(worst, float((np.abs(a - b)[nz] / np.abs(b)[nz]).max()))
    return worst


@pytest.mark.parametrize("k,n_targets,q", [(8, 1, 0), (8, 2, 1), (8, 1, 16), (33, 3, 4), (8, 3, 16)])
def test_uncertainties_against_the_reference(k, n_targets, q):
    """The yardstick is the reference's own spread: its Gram route in float64 against its SVD route on the long-double W.  The
    device may differ from the SVD route by ten times that (the rule of tests/test_gpu_mbar_uncertainty.py).  d_energy_mean and
    d_mean are also what the energy form and the observable form give, from other Theta matrices: the same rule."""
    case = _case(k, n_targets, q)
    moments = case["dev"]["moments"]
    want = ref.sigmas(ref.theta_svd(case["w"], case["counts"]), k, n_targets, q, moments)
    own = ref.sigmas(ref.theta_gram(case["gram"], case["counts"]), k, n_targets, q, moments)
    args = (case["energies"], case["rungs"], case["temps"], case["f"], case["targets"])
    out = statistics.mbar_fluctuation_uncertainties(*args, case["columns"] if q else None)
    spread = _largest_relative_difference([own[key] for key in ref.KEYS], [want[key] for key in ref.KEYS])
    err = _largest_relative_difference([out[key] for key in ref.KEYS], [want[key] for key in ref.KEYS])
    print("K = %d, %d targets, Q = %d: reference Gram route against SVD route %.3e, device against SVD route %.3e"
          % (k, n_targets, q, spread, err))
    plain = statistics.mbar_uncertainties(*args)
    cross = [_largest_relative_difference([out["d_energy_mean"]], [plain["d_energy_mean"]])]
    if q:
        obs = statistics.mbar_observable_uncertainties(*args, case["columns"])
        cross.append(_largest_relative_difference([out["d_mean"]], [obs["d_mean"]]))
    print("    d_energy_mean against the energy form%s: %s" % (", d_mean against the observable form" if q else "", cross))
    assert out["n_samples"] == uref.N_GRAM and out["names"] == tuple(range(q))
    assert set(out) == {"temps", "names", "n_samples", "energy_mean", "d_energy_mean", "energy_var", "d_energy_var", "heat_capacity",
                        "d_heat_capacity", "mean", "d_mean", "var", "d_var", "cov_energy", "d_cov_energy", "dmean_dT", "d_dmean_dT"}
    for key in ("energy_mean", "energy_var", "heat_capacity"):
        assert out[key].shape == out["d_" + key].shape == (n_targets,), key
        assert _bitwise(out[key], statistics.mbar_reweight(*args)[key]), key
    for key in ("mean", "var", "cov_energy", "dmean_dT"):
        assert out[key].shape == out["d_" + key].shape == (n_targets, q), key
        if q:
            assert _bitwise(out[key], statistics.mbar_reweight_observables(*args, case["columns"])[key]), key
    t_sq = case["targets"] ** 2
    assert np.array_equal(out["d_heat_capacity"], out["d_energy_var"] / t_sq)
    assert np.array_equal(out["d_dmean_dT"], out["d_cov_energy"] / t_sq[:, None])
    assert err <= 10.0 * spread
    assert max(cross) <= 10.0 * spread


# ------------------------------------------------------------------------------------------------------ 7. forms agree
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


@pytest.mark.parametrize("observables", [("real_0", "abs_real_0", "real_0_sq"), None])
def test_engine_form_equals_the_engine_less_form(observables):
    eng, temps = _ladder_engine(observables=observables)
    q = len(observables or ())
    f = eng.ladder_free_energies()["f"]
    targets = np.array([0.7, 1.9])
    samples = eng.energy_samples()
    rungs = np.tile(np.arange(eng.n_chains) // 64, samples.shape[0])
    columns = eng.observable_samples().transpose(1, 0, 2).reshape(q, -1) if q else None
    a = eng.fluctuation_uncertainties(targets, f)
    b = statistics.mbar_fluctuation_uncertainties(samples, rungs, temps, f, targets, columns)
    assert a["names"] == tuple(observables or ()) and b["names"] == tuple(range(q))
    four = eng.fluctuation_uncertainties(targets, f, inefficiency=4.0)
    for key in a:
        if key == "names":
            continue
        assert _bitwise(a[key], b[key]), key
        if key.startswith("d_"):
            assert np.asarray(a[key]).shape == ((2, q) if key[2:] in ("mean", "var", "cov_energy", "dmean_dT") else (2,)), key
            assert np.all(np.isfinite(a[key])) and np.all(a[key] > 0), key
            assert np.array_equal(four[key], 2.0 * a[key]), key
        else:
            assert _bitwise(four[key], a[key]), key
    solved = eng.fluctuation_uncertainties(targets)            # f = None solves first
    assert _bitwise(solved["heat_capacity"], eng.reweight(targets)["heat_capacity"])
    # "recorded": the largest g over the rungs, the energy and every recorded column (when every such series has one)
    g = eng.recorded_inefficiency()["g"][:1 + q]
    if np.all(np.isfinite(g)):
        recorded = eng.fluctuation_uncertainties(targets, f, inefficiency="recorded")
        by_hand = eng.fluctuation_uncertainties(targets, f, inefficiency=float(np.max(g)))
        assert all(_bitwise(recorded[key], by_hand[key]) for key in recorded if key != "names")
    else:
        with pytest.raises(ValueError, match="recorded"):
            eng.fluctuation_uncertainties(targets, f, inefficiency="recorded")
    if q:
        assert _bitwise(solved["var"], eng.reweight_observables(targets)["var"])
    c = 4 + targets.size * (3 + 3 * q)
    gram, counts = np.zeros((c, c)), np.zeros(c)
    eng._check(eng._lib.me_mbar_gram_fluctuations(eng._handle, f.ctypes.data_as(DP), targets.ctypes.data_as(DP), targets.size,
                                                  gram.ctypes.data_as(DP), counts.ctypes.data_as(DP), *([None] * 10)))
    less = _gram_fluctuations(samples, rungs, temps, f, targets, columns)
    assert _bitwise(gram, less["gram"]) and np.array_equal(counts, less["counts"])


# ------------------------------------------------------------------------------------------ 8. calibration on the device
def test_calibration_on_the_device():
    """The subsets of tests/test_mbar_fluctuation_uncertainty_cpu.py through the GPU; the same band for the 21 RMS z-scores of
    Var E, Var A_q and Cov(A_q, E) against the exact values (Cov(x_0, E) is exactly 0: that z is an absolute difference)."""
    estimates, errors = [], []
    for energies, rungs, cols in ref.calibration_subsets():
        f = statistics.mbar_free_energies(energies, rungs, ref.LADDER8, tol=1e-12)["f"]
        out = statistics.mbar_fluctuation_uncertainties(energies, rungs, ref.LADDER8, f, ref.PHYSICS_TARGETS, cols)
        estimates.append((out["energy_var"], out["var"], out["cov_energy"]))
        errors.append((out["d_energy_var"], out["d_var"], out["d_cov_energy"]))
    rms = ref.calibration_rms_z(estimates, errors)
    print("rms z on the device (targets x [Var E, Var x_0, Var |x_0|, Var x_0^2, Cov(x_0, E), Cov(|x_0|, E), Cov(x_0^2, E)]):\n%s"
          % rms)
    lo, hi = uref.CAL_RMS_Z
    assert rms.shape == (3, 7) and np.all((rms >= lo) & (rms <= hi))


# ------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    # an engine without an observable store works, with Q = 0
    no_store, _ = _ladder_engine(records=1, observables=None)
    out = no_store.fluctuation_uncertainties([1.0], np.zeros(4))
    assert out["names"] == () and out["d_heat_capacity"].shape == (1,) and out["d_var"].shape == (1, 0)
    assert np.isfinite(out["d_heat_capacity"][0]) and out["d_heat_capacity"][0] > 0
    gram, counts, f4, t1 = np.zeros((7, 7)), np.zeros(7), np.zeros(4), np.ones(1)
    none = [None] * 10
    assert no_store._lib.me_mbar_gram_fluctuations(no_store._handle, f4.ctypes.data_as(DP), t1.ctypes.data_as(DP), 1,
                                                   gram.ctypes.data_as(DP), counts.ctypes.data_as(DP), *none) == _capi.ME_OK
    assert no_store._lib.me_mbar_gram_fluctuations(no_store._handle, f4.ctypes.data_as(DP), t1.ctypes.data_as(DP), 0,
                                                   gram.ctypes.data_as(DP), counts.ctypes.data_as(DP), *none) == _capi.ME_ERR_INVALID
    plain = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=256, seed=5, dtype="f64", temp=1.0)
    plain.record_energies(1)
    plain.record_energy()
    with pytest.raises(_capi.MetropolisLibraryError, match="no temperature ladder") as no_ladder:
        plain.fluctuation_uncertainties([1.0], f=[0.0])
    assert no_ladder.value.status == _capi.ME_ERR_STATE
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1] * 4, None, n_chains=256, seed=5, dtype="f64",
                              temperatures=[0.6, 0.9, 1.4, 2.1])
    eng.record_energies(1)
    eng.record_observables(["real_0"])
    with pytest.raises(_capi.MetropolisLibraryError, match="no recorded energy samples") as no_records:
        eng.fluctuation_uncertainties([1.0], np.zeros(4))
    assert no_records.value.status == _capi.ME_ERR_STATE
    temps, energies, rungs = uref.synthetic(8, 2053)
    f, cols = np.zeros(8), np.ones((2, 2053))
    for bad in ([], [0.0], [-1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            statistics.mbar_fluctuation_uncertainties(energies, rungs, temps, f, bad, cols)
        with pytest.raises(ValueError):
            eng.fluctuation_uncertainties(bad, np.zeros(4))
    for bad in (0.99, -2.0, np.nan, np.inf, [1.0, 1.0], "measured"):
        with pytest.raises(ValueError):
            statistics.mbar_fluctuation_uncertainties(energies, rungs, temps, f, [1.0], cols, inefficiency=bad)
        with pytest.raises(ValueError):
            eng.fluctuation_uncertainties([1.0], np.zeros(4), inefficiency=bad)
    # no target and Q = 17 through the C ABI: ME_ERR_INVALID (ValueError)
    with pytest.raises(ValueError):
        _gram_fluctuations(energies, rungs, temps, f, np.zeros(0), cols)
    with pytest.raises(ValueError):
        statistics.mbar_fluctuation_uncertainties(energies, rungs, temps, f, [1.0], np.ones((17, 2053)))
    with pytest.raises(ValueError):
        _gram_fluctuations(energies, rungs, temps, f, [1.0], np.ones((17, 2053)))
    # more than 64 rungs: the Python layer refuses (ValueError), the C ABI reports ME_ERR_UNSUPPORTED (NotImplementedError)
    temps65 = np.linspace(0.5, 3.0, 65)
    rungs65 = (np.arange(2053) % 65).astype(np.int32)
    with pytest.raises(ValueError):
        statistics.mbar_fluctuation_uncertainties(energies, rungs65, temps65, np.zeros(65), [1.0], cols)
    with pytest.raises(NotImplementedError):
        _gram_fluctuations(energies, rungs65, temps65, np.zeros(65), [1.0], cols)
    with pytest.raises(NotImplementedError):
        _gram_fluctuations(energies, rungs65, temps65, np.zeros(65), [1.0])
