"""Timings of the MBAR solver and of the energy-sample record kernel (profiles/mbar_solve.txt).

    python tools/bench_mbar.py [--log2-chains 15] [--records 1024] [--rungs 8 16 32] [--reference-log2 20]
    python tools/bench_mbar.py --one-solve 16       (a single solve, for a kernel trace around it)
    python tools/bench_mbar.py --gram               (the Gram pass of the asymptotic error bars, profiles/mbar_uncertainty.txt)
    python tools/bench_mbar.py --observables        (reweighting of recorded observables: whole-call time beside the energy-only call)
    python tools/bench_mbar.py --perturbed --rungs 8 32
                                                    (reweighting to perturbed energies, every column coupled and one column
                                                     coupled, beside the observable reweighting, profiles/mbar_perturbed.txt)
    python tools/bench_mbar.py --observable-gram    (the Gram pass with observable columns beside me_mbar_gram at an equal
                                                     column count, profiles/mbar_observable_uncertainty.txt)
    python tools/bench_mbar.py --fluctuations --rungs 8 32
                                                    (the Gram pass with second-moment columns beside the observable form on the
                                                     same input, profiles/mbar_fluctuation_uncertainty.txt)
    python tools/bench_mbar.py --profile            (reweighted histograms along an observable beside the one-column observable
                                                     reweighting, profiles/mbar_profile.txt)
    python tools/bench_mbar.py --profile-uncertainty --rungs 8 32
                                                    (the error bars of those histograms beside the histograms themselves,
                                                     profiles/mbar_profile_uncertainty.txt)
    python tools/bench_mbar.py --surface            (joint histograms along two observables on 8 x 8, 16 x 16 and 33 x 33 bins
                                                     beside the 1-D histograms, profiles/mbar_surface.txt)
    python tools/bench_mbar.py --surface-uncertainty --rungs 8 32
                                                    (the error bars of those joint histograms beside the histograms themselves and
                                                     the host algebra with and without the cell covariance,
                                                     profiles/mbar_surface_uncertainty.txt)
    python tools/bench_mbar.py --newton             (the Newton solver beside the self-consistent one: one pass and the whole
                                                     solve, profiles/mbar_newton.txt)
    python tools/bench_mbar.py --inefficiency       (statistical inefficiencies of the recorded series with 0, 4 and 16 recorded
                                                     columns beside the host route, profiles/mbar_inefficiency.txt)

Per ladder size K: synthetic energies of a 16-dimensional quadratic form (E / T Gamma(8) distributed) on T_k = 0.5 r^k with
r chosen so that the ladder spans the same range for every K, injected with set_energy_samples; one warm-up solve, then a
timed solve to tol = 1e-10.  Milliseconds per iteration = wall time of the solve / iterations (the solve includes its
counting pass and one 16-byte read per batch of 16 iterations).  Beside it the numpy restatement's time per iteration.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metropolisengine_amd as me  # noqa: E402
import mbar_reference as ref  # noqa: E402

DIM = 16


def times_ms(call, repeats=3):
    """Milliseconds of ``repeats`` calls after one warm-up call (allocations, code objects)."""
    call()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return [1e3 * t for t in times]


def best(call, repeats=3):
    return min(times_ms(call, repeats))


def lane_patterns(n_chains):
    """The two inputs of the histogram timings as one bin index per chain (edges 0, 1, 2, ...; the value is the index + 0.5):
    every chain in bin 0 (a wavefront's 64 lanes share a slot) and consecutive chains in 64 DIFFERENT bins."""
    return np.zeros(n_chains, dtype=np.int64), np.arange(n_chains) % 64


def ladder(k):
    return 0.5 * (1.3 ** 7) ** (np.arange(k) / (k - 1.0))


def loaded_engine(k, log2_chains, records, seed=1):
    n = 1 << log2_chains
    temps = ladder(k)
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=n, seed=3, dtype="f64", temperatures=temps)
    eng.record_energies(records)
    rng = np.random.default_rng(seed)
    scale = np.repeat(temps, n // k)
    eng.set_energy_samples(rng.gamma(DIM / 2.0, 1.0, size=(records, n)) * scale[None, :])
    return eng, temps


def time_solve(k, log2_chains, records):
    eng, _ = loaded_engine(k, log2_chains, records)
    eng.ladder_free_energies(tol=1e-10, max_iter=16)            # warm-up: allocations, code objects
    t0 = time.perf_counter()
    out = eng.ladder_free_energies(tol=1e-10)
    wall = time.perf_counter() - t0
    n = records << log2_chains
    ms = 1e3 * wall / out["iterations"]
    exps = n * k * (1 if k <= 16 else 2)
    print("K = %2d: %d samples, %d iterations to residual %.2e (converged %s), %.3f ms per iteration, %.1f GB/s of samples, "
          "%.3e exponentials/s (%d per sample and rung)"
          % (k, n, out["iterations"], out["residual"], out["converged"], ms, 8e-9 * n / (1e-3 * ms), exps / (1e-3 * ms),
             1 if k <= 16 else 2), flush=True)
    t0 = time.perf_counter()
    eng.reweight(np.geomspace(0.5, 3.0, 8), out["f"])
    print("        reweighting to 8 temperatures: %.3f ms" % (1e3 * (time.perf_counter() - t0)), flush=True)


def time_gram(k, log2_chains, records, n_targets=8):
    """me_mbar_gram (csrc/me_mbar_cov.hip) without targets and with ``n_targets``, beside the solver's time per iteration on
    the same samples.  The call includes its counting pass, the reweighting of the targets and the copy of G to the host."""
    import ctypes
    eng, _ = loaded_engine(k, log2_chains, records)
    eng.ladder_free_energies(tol=1e-10, max_iter=16)
    t0 = time.perf_counter()
    out = eng.ladder_free_energies(tol=1e-10)
    per_iteration = 1e3 * (time.perf_counter() - t0) / out["iterations"]
    f, dp = out["f"], ctypes.POINTER(ctypes.c_double)
    line = "K = %2d: %d samples, solver %.3f ms per iteration;" % (k, records << log2_chains, per_iteration)
    for nt in (0, n_targets):
        targets = np.geomspace(0.5, 3.0, nt) if nt else np.zeros(0)
        c = k + 2 * nt
        gram, counts = np.zeros((c, c)), np.zeros(c)
        call = lambda: eng._check(eng._lib.me_mbar_gram(      # noqa: E731
            eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp) if nt else None, nt, gram.ctypes.data_as(dp),
            counts.ctypes.data_as(dp), None, None, None))
        call()                                                  # warm-up
        t0 = time.perf_counter()
        call()
        ms = 1e3 * (time.perf_counter() - t0)
        line += " Gram with %d targets (C = %d) %.3f ms = %.1f iterations;" % (nt, c, ms, ms / per_iteration)
    print(line, flush=True)


HBM_RATE = 6.3e12      # bytes per second a streaming kernel reaches on the MI355X (8 TB/s is the data-sheet figure)


def time_observables(k, log2_chains, records, n_targets=8, columns=(1, 4, 16)):
    """me_mbar_reweight_observables (csrc/me_mbar_obs.hip) for Q recorded columns at ``n_targets`` temperatures beside the
    energy-only me_mbar_reweight on the same samples in the same run.  Both calls include their counting pass and the upload
    of the table; the observables' call adds one pass that writes d_n and ceil(T / 4) ceil(Q / 4) passes of up to 4 targets x
    4 columns that each read (1 + q) 8 + 8 bytes per sample.  The time is the wall time of the WHOLE call (counting pass,
    table upload, allocation of d and of the partials, the d pass, two launches per pass, the copy back and the wait), so the
    rate printed from it is a lower bound for what k_mbar_reweight_obs itself reaches, not its share."""
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    targets = np.geomspace(0.5, 3.0, n_targets)

    energy_ms = best(lambda: eng.reweight(targets, f))
    print("K = %d, %d samples, %d targets: energy-only reweighting (me_mbar_reweight) %.3f ms" % (k, n, n_targets, energy_ms),
          flush=True)
    energies = eng.energy_samples()
    for q in columns:
        eng.record_observables([j % 4 for j in range(q)])       # (one real parameter: a catalogue of 4 entries, duplicates
        eng.set_energy_samples(energies)                        # allowed; the values are set below)
        scale = 1.0 + 0.125 * np.arange(q)
        eng.set_observable_samples(energies[:, None, :] * scale[None, :, None])
        ms = best(lambda: eng.reweight_observables(targets, f))
        passes = [(min(4, n_targets - t0), min(4, q - q0)) for t0 in range(0, n_targets, 4) for q0 in range(0, q, 4)]
        traffic = n * (16 + sum((1 + nq) * 8 + 8 for _, nq in passes))      # the d pass reads E and writes d
        print("    Q = %2d: %.3f ms = %.2f x energy-only; %d passes, %.2f GB of sample traffic: whole call >= %.0f GB/s = %.0f %% "
              "of the %.1f TB/s HBM rate (a lower bound for the passes)" % (q, ms, ms / energy_ms, len(passes), 1e-9 * traffic, 1e-9 * traffic / (1e-3 * ms),
                                      100 * traffic / (1e-3 * ms) / HBM_RATE, 1e-12 * HBM_RATE), flush=True)


def time_perturbed(k, log2_chains, records, n_targets=8, columns=(1, 4, 16)):
    """me_mbar_reweight_perturbed (csrc/me_mbar_perturbed.hip) for Q recorded columns at ``n_targets`` targets, with every column
    coupled and with one column coupled, beside me_mbar_reweight_observables on the same input in the same run (the yardstick:
    a kernel the perturbed unit does not touch).  Both times are wall times of the WHOLE call.  Per chunk of 4 targets the
    perturbed call adds one bias pass, which reads its coupled columns and writes 32 bytes per sample, and every pass of 4
    columns reads those 32 bytes on top of what k_mbar_reweight_obs reads."""
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    targets = np.geomspace(0.5, 3.0, n_targets)
    energies = eng.energy_samples()
    print("K = %d, %d samples, %d targets" % (k, n, n_targets), flush=True)
    for q in columns:
        eng.record_observables([j % 4 for j in range(q)])
        eng.set_energy_samples(energies)
        scale = 1.0 + 0.125 * np.arange(q)
        eng.set_observable_samples(energies[:, None, :] * scale[None, :, None])
        obs_ms = best(lambda: eng.reweight_observables(targets, f))
        line = "    Q = %2d: reweight_observables %.3f ms;" % (q, obs_ms)
        for label, coupled in (("every column coupled", q), ("one column coupled", 1)):
            lam = np.zeros((n_targets, q))
            lam[:, :coupled] = 0.02 / coupled
            ms = best(lambda: eng.reweight_perturbed(targets, lam, f))
            chunks, col_passes = -(-n_targets // 4), -(-q // 4)
            traffic = n * (16 + chunks * ((coupled * 8 + 32) + sum((1 + min(4, q - q0)) * 8 + 8 + 32 for q0 in range(0, q, 4))))
            line += " %s %.3f ms = %.2f x (%d bias + %d column passes, %.2f GB, whole call >= %.0f GB/s);" % (
                label, ms, ms / obs_ms, chunks, chunks * col_passes, 1e-9 * traffic, 1e-9 * traffic / (1e-3 * ms))
        print(line, flush=True)


def time_observable_gram(k, log2_chains, records, n_targets=8, columns=(1, 4, 16)):
    """me_mbar_gram_observables (csrc/me_mbar_cov.hip) for Q recorded columns at ``n_targets`` temperatures beside me_mbar_gram
    with as many targets as give the same number of target columns, (1 + Q) n_targets / 2, on the same samples in the same
    run.  Both are whole calls (counting pass, reweighting of the targets, the Gram launches of every chunk, the copy of G);
    the observable form's call also holds the reweighting of the observables that supplies its normalising means, which is
    timed alone beside it (me_mbar_reweight_observables, a whole call too).  Columns are counted per launch: every chunk of
    targets carries the K ladder columns."""
    import ctypes
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    dp = ctypes.POINTER(ctypes.c_double)
    targets = np.geomspace(0.5, 3.0, n_targets)
    energies = eng.energy_samples()

    def launched(per_target, nt):
        per_chunk = (128 - k) // per_target
        return [k + per_target * min(per_chunk, nt - t0) for t0 in range(0, nt, per_chunk)]

    print("K = %d, %d samples, %d targets" % (k, n, n_targets), flush=True)
    for q in columns:
        eng.record_observables([j % 4 for j in range(q)])       # (one real parameter: a catalogue of 4 entries, duplicates
        eng.set_energy_samples(energies)                        # allowed; the values are set below)
        scale = 1.0 + 0.125 * np.arange(q)
        eng.set_observable_samples(energies[:, None, :] * scale[None, :, None])
        c = k + n_targets * (1 + q)
        gram, counts = np.zeros((c, c)), np.zeros(c)
        obs = times_ms(lambda: eng._check(eng._lib.me_mbar_gram_observables(
            eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp), n_targets, gram.ctypes.data_as(dp), counts.ctypes.data_as(dp),
            None, None, None, None)))
        obs_ms, obs_max = min(obs), max(obs)
        rw_ms = best(lambda: eng.reweight_observables(targets, f))
        nt_e = max(1, (n_targets * (1 + q) + 1) // 2)
        targets_e = np.geomspace(0.5, 3.0, nt_e)
        ce = k + 2 * nt_e
        gram_e, counts_e = np.zeros((ce, ce)), np.zeros(ce)
        plain = times_ms(lambda: eng._check(eng._lib.me_mbar_gram(
            eng._handle, f.ctypes.data_as(dp), targets_e.ctypes.data_as(dp), nt_e, gram_e.ctypes.data_as(dp), counts_e.ctypes.data_as(dp),
            None, None, None)))
        e_ms, e_max = min(plain), max(plain)
        cols_o, cols_e = launched(1 + q, n_targets), launched(2, nt_e)
        print("    Q = %2d: me_mbar_gram_observables %.3f ms (slowest of 3: %.3f), launches of %s columns; of that the observables' "
              "reweighting alone %.3f ms; me_mbar_gram with %d targets %.3f ms (slowest of 3: %.3f), launches of %s columns; ratio "
              "of the times %.2f, of the launched columns %.2f, of their squares %.2f"
              % (q, obs_ms, obs_max, cols_o, rw_ms, nt_e, e_ms, e_max, cols_e, obs_ms / e_ms, sum(cols_o) / sum(cols_e),
                 sum(x * x for x in cols_o) / sum(x * x for x in cols_e)), flush=True)


def time_fluctuations(k, log2_chains, records, n_targets=8, columns=(0, 1, 4, 16)):
    """me_mbar_gram_fluctuations (csrc/me_mbar_cov.hip, the fluctuation form) for Q recorded columns at ``n_targets``
    temperatures beside me_mbar_gram_observables on the same samples, columns and targets in the same run (Q = 0: beside
    me_mbar_gram, the energy form, which has no observable form to compare with).  Whole calls (counting pass, the reweighting
    of the energies and of the observables that supplies the normalisers, the Gram launches of every chunk, the copy of G);
    the Python method, which adds the host algebra, is timed beside them.  Columns are counted per launch: every chunk of
    targets carries the K ladder columns."""
    import ctypes
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    dp = ctypes.POINTER(ctypes.c_double)
    targets = np.geomspace(0.5, 3.0, n_targets)
    energies = eng.energy_samples()

    def launched(per_target):
        per_chunk = (128 - k) // per_target
        return [k + per_target * min(per_chunk, n_targets - t0) for t0 in range(0, n_targets, per_chunk)]

    print("K = %d, %d samples, %d targets" % (k, n, n_targets), flush=True)
    for q in columns:
        eng.record_observables([j % 4 for j in range(q)] if q else None)
        eng.set_energy_samples(energies)
        if q:
            scale = 1.0 + 0.125 * np.arange(q)
            eng.set_observable_samples(energies[:, None, :] * scale[None, :, None])
        c = k + n_targets * (3 + 3 * q)
        gram, counts = np.zeros((c, c)), np.zeros(c)
        new = times_ms(lambda: eng._check(eng._lib.me_mbar_gram_fluctuations(
            eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp), n_targets, gram.ctypes.data_as(dp), counts.ctypes.data_as(dp),
            *([None] * 10))))
        whole = times_ms(lambda: eng.fluctuation_uncertainties(targets, f))
        per_old = 1 + q if q else 2
        co = k + n_targets * per_old
        gram_o, counts_o = np.zeros((co, co)), np.zeros(co)
        if q:
            old = times_ms(lambda: eng._check(eng._lib.me_mbar_gram_observables(
                eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp), n_targets, gram_o.ctypes.data_as(dp),
                counts_o.ctypes.data_as(dp), None, None, None, None)))
            old_whole = times_ms(lambda: eng.observable_uncertainties(targets, f))
        else:
            old = times_ms(lambda: eng._check(eng._lib.me_mbar_gram(
                eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp), n_targets, gram_o.ctypes.data_as(dp),
                counts_o.ctypes.data_as(dp), None, None, None)))
            old_whole = times_ms(lambda: eng.ladder_free_energy_uncertainties(f, targets))
        cols_n, cols_o = launched(3 + 3 * q), launched(per_old)
        print("    Q = %2d: me_mbar_gram_fluctuations %.3f ms (slowest of 3: %.3f), launches of %s columns, fluctuation_uncertainties "
              "%.3f ms; %s %.3f ms (slowest of 3: %.3f), launches of %s columns, %s %.3f ms; ratio of the C calls %.2f, of the "
              "launched columns %.2f, of their squares %.2f"
              % (q, min(new), max(new), cols_n, min(whole), "me_mbar_gram_observables" if q else "me_mbar_gram", min(old), max(old),
                 cols_o, "observable_uncertainties" if q else "ladder_free_energy_uncertainties", min(old_whole), min(new) / min(old),
                 sum(cols_n) / sum(cols_o), sum(x * x for x in cols_n) / sum(x * x for x in cols_o)), flush=True)


def time_profile(k, log2_chains, records, n_targets=8, bins=(64, 256)):
    """me_mbar_histogram (csrc/me_mbar_hist.hip) for one recorded column at ``n_targets`` temperatures, on two inputs: one
    whose values all fall in ONE bin (a wavefront's 64 lanes share a slot: one match round and a butterfly per temperature)
    and one where consecutive samples fall in 64 DIFFERENT bins (64 match rounds per item, every lane adds its own weight).
    Beside them, on the same samples in the same run, me_mbar_reweight_observables with that one column and the energy-only
    me_mbar_reweight.  All are whole calls (counting pass, table upload, allocations, every launch, the copy back and the
    wait); the histogram's call holds me_mbar_reweight's kernels (they supply ln_z and neff_fraction), the pass that writes
    d_n, and ceil(T / 4) passes that each read 24 bytes per sample."""
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    targets = np.geomspace(0.5, 3.0, n_targets)

    energy_ms = best(lambda: eng.reweight(targets, f))
    energies = eng.energy_samples()
    eng.record_observables([0])
    eng.set_energy_samples(energies)
    one_bin, many_bins = lane_patterns(eng.n_chains)
    inputs = (("every value in one bin", one_bin + 0.5), ("consecutive samples in 64 different bins", many_bins + 0.5))
    print("K = %d, %d samples, %d targets: energy-only reweighting (me_mbar_reweight) %.3f ms" % (k, n, n_targets, energy_ms),
          flush=True)
    for label, row in inputs:
        eng.set_observable_samples(np.broadcast_to(row[None, None, :], (records, 1, eng.n_chains)))
        obs_ms = best(lambda: eng.reweight_observables(targets, f))
        print("    %s: reweight_observables with this one column %.3f ms" % (label, obs_ms), flush=True)
        for b in bins:
            edges = np.linspace(0.0, float(b), b + 1)
            out = eng.free_energy_profile(0, edges, targets, f)
            assert int((out["counts"] > 0).sum()) == (1 if row.max() == row.min() else 64) and out["counts"].sum() == n
            ms = best(lambda: eng.free_energy_profile(0, edges, targets, f))
            print("        %3d bins: free_energy_profile %.3f ms = %.2f x the one-column observable reweighting, %.2f x energy-only; "
                  "%.3e exponentials/s over the whole call" % (b, ms, ms / obs_ms, ms / energy_ms, n * n_targets / (1e-3 * ms)),
                  flush=True)


def time_profile_uncertainty(k, log2_chains, records, n_targets=8, bins=(64, 256), forced_rows=0):
    """me_mbar_histogram_gram (csrc/me_mbar_hist_cov.hip) on the two inputs of :func:`time_profile`, beside me_mbar_histogram on
    the same samples in the same run.  Whole calls.  The new call holds the histogram's own kernels, ``n_targets ceil((K + 1) /
    R)`` passes of the slot Gram kernel (R rows of the weight matrix per pass: 16, 8 or 4 by the bin count) where the
    histogram takes ``ceil(n_targets / 4)``, and the Gram pass of the K ladder columns; ``sums`` is the same call without that
    last pass and without the host algebra (the C entry point with ladder_gram = NULL).  ``forced_rows``: the R of a library
    built with ``-DME_HIST_COV_ROWS=R`` (selected with METROPOLIS_HIP_LIB), for the pass counts that are printed."""
    import ctypes
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    targets = np.geomspace(0.5, 3.0, n_targets)
    dp = ctypes.POINTER(ctypes.c_double)

    energies = eng.energy_samples()
    eng.record_observables([0])
    eng.set_energy_samples(energies)
    one_bin, many_bins = lane_patterns(eng.n_chains)
    inputs = (("every value in one bin", one_bin + 0.5), ("consecutive samples in 64 different bins", many_bins + 0.5))
    print("K = %d, %d samples, %d targets" % (k, n, n_targets), flush=True)
    for label, row in inputs:
        eng.set_observable_samples(np.broadcast_to(row[None, None, :], (records, 1, eng.n_chains)))
        print("    %s" % label, flush=True)
        for b in bins:
            edges = np.linspace(0.0, float(b), b + 1)
            rows = forced_rows or gram_rows(b)
            out = eng.free_energy_profile_uncertainties(0, edges, targets, f)
            assert out["counts"].sum() == n and np.all(np.isfinite(out["d_mass"]))
            h = np.zeros((n_targets, k + 1, b + 3))
            sums = best(lambda: eng._check(eng._lib.me_mbar_histogram_gram(
                eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp), n_targets, 0, edges.ctypes.data_as(dp), b,
                h.ctypes.data_as(dp), None, None, None, None, None, None)))
            whole = best(lambda: eng.free_energy_profile_uncertainties(0, edges, targets, f))
            plain = best(lambda: eng.free_energy_profile(0, edges, targets, f))
            passes, plain_passes = n_targets * -(-(k + 1) // rows), -(-n_targets // 4)
            print("        %3d bins: free_energy_profile %.3f ms (%d passes); slot Gram sums %.3f ms (R = %d: %d more passes) = %.2f x, "
                  "%.3f ms per added pass; free_energy_profile_uncertainties %.3f ms = %.2f x"
                  % (b, plain, plain_passes, sums, rows, passes, sums / plain, (sums - plain) / passes, whole, whole / plain), flush=True)


def gram_rows(n_bins):
    """rule_rows of csrc/me_mbar_hist_cov.hip: the rows per pass, the widest of 16, 8, 4 whose LDS (slot_pass_lds of
    csrc/me_mbar_slots.h without counts) leaves four workgroups on a CU."""
    return next((r for r in (16, 8) if 4 * (8 * (n_bins + 1) + 32 * r * (n_bins + 3)) <= 160 * 1024), 4)


def surface_rows(n_cells):
    """rows_per_pass of csrc/me_mbar_hist2d.hip (joint_rule_rows of csrc/me_mbar_slots.h with counts, widest R = 4): the
    temperatures per pass, from the number of cells alone."""
    return 4 if n_cells <= 374 else 2 if n_cells <= 666 else 1


def time_surface(k, log2_chains, records, n_targets=8, grids=(8, 16, 33), bins=(64, 256), forced_rows=0):
    """me_mbar_histogram_joint (csrc/me_mbar_hist2d.hip) for two recorded columns at ``n_targets`` temperatures on square grids,
    beside me_mbar_histogram (64 and 256 bins) on the same samples in the same run, on the two kinds of input of
    :func:`time_profile`: every sample in ONE cell (a wavefront's 64 lanes share it) and consecutive samples in 64 DIFFERENT
    cells (an 8 x 8 block of the grid; 64 different bins for the 1-D call).  Whole calls (counting pass, table upload,
    allocations, every launch, the copy back and the wait); the joint call holds me_mbar_reweight's kernels, the pass that writes
    d_n and ceil(T / R) passes that each read 32 bytes per sample, R = 4, 2 or 1 by the number of cells.  ``forced_rows``: the R
    of a library built with ``-DME_HIST2D_ROWS=R`` (selected with METROPOLIS_HIP_LIB), for the pass counts that are printed."""
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    targets = np.geomspace(0.5, 3.0, n_targets)

    energies = eng.energy_samples()
    eng.record_observables([0, 1, 2])                           # columns: x, y, and the 1-D call's value
    eng.set_energy_samples(energies)
    one_bin, many_bins = lane_patterns(eng.n_chains)           # (the 64 bins as an 8 x 8 block of the grid)
    inputs = (("every sample in one cell", np.stack([one_bin + 0.5] * 3)),
              ("consecutive samples in 64 different cells", np.stack([many_bins // 8 + 0.5, many_bins % 8 + 0.5, many_bins + 0.5])))
    print("K = %d, %d samples, %d targets" % (k, n, n_targets), flush=True)
    for label, rows in inputs:
        eng.set_observable_samples(np.broadcast_to(rows[None, :, :], (records, 3, eng.n_chains)))
        print("    %s" % label, flush=True)
        filled = 1 if label.startswith("every") else 64
        plain = {}
        for b in bins:
            edges = np.linspace(0.0, float(b), b + 1)
            out = eng.free_energy_profile(2, edges, targets, f)
            assert int((out["counts"] > 0).sum()) == filled and out["counts"].sum() == n
            plain[b] = best(lambda: eng.free_energy_profile(2, edges, targets, f))
            print("        %3d bins: free_energy_profile %.3f ms (%d passes of 24 bytes per sample)" % (b, plain[b], -(-n_targets // 4)),
                  flush=True)
        for g in grids:
            edges = np.linspace(0.0, float(g), g + 1)
            out = eng.free_energy_surface(0, edges, 1, edges, targets, f)
            assert int((out["counts"] > 0).sum()) == filled and out["counts"].sum() == n
            assert np.max(np.abs(out["mass"].reshape(n_targets, -1).sum(axis=1) - 1.0)) <= 1e-13
            r = forced_rows or surface_rows((g + 3) * (g + 3))
            ms = best(lambda: eng.free_energy_surface(0, edges, 1, edges, targets, f))
            print("        %2d x %2d bins (%4d cells, R = %d: %d passes of 32 bytes per sample): free_energy_surface %.3f ms = %s"
                  % (g, g, (g + 3) * (g + 3), r, -(-n_targets // r), ms,
                     ", ".join("%.2f x the %d-bin profile" % (ms / plain[b], b) for b in bins)), flush=True)


def surface_gram_rows(n_cells):
    """rule_rows of csrc/me_mbar_hist2d_cov.hip (joint_rule_rows of csrc/me_mbar_slots.h without counts, widest R = 16): the
    rows per pass, the widest of 16, 8, 4, 2, 1 whose table, at most ``(32 R + 2) S`` bytes, leaves three workgroups within the
    160 KiB of a CU (16 up to 106 cells, 8 to 211, 4 to 420, 2 to 827)."""
    return next((r for r in (16, 8, 4, 2) if n_cells <= (160 * 1024 // 3) // (32 * r + 2)), 1)


def time_surface_uncertainty(k, log2_chains, records, n_targets=8, grids=(8, 16, 33), forced_rows=0, sums_only=False):
    """me_mbar_histogram_joint_gram (csrc/me_mbar_hist2d_cov.hip) on the two inputs of :func:`time_surface`, beside
    me_mbar_histogram_joint on the same samples in the same run.  Whole calls.  ``sums`` is the C entry point with ladder_gram =
    NULL: the joint histogram's own kernels and ``n_targets ceil((K + 1) / R)`` passes of the cell Gram kernel; the whole call adds
    the Gram pass of the K ladder columns and the host algebra, which is also timed alone with and without the cell covariance.
    ``forced_rows``: the R of a library built with ``-DME_HIST2D_COV_ROWS=R`` (selected with METROPOLIS_HIP_LIB), used wherever
    its table fits 64 KiB, for the pass counts that are printed.  ``sums_only``: the cell Gram sums alone (the forced-R runs)."""
    import ctypes
    from metropolisengine_amd import statistics
    eng, _ = loaded_engine(k, log2_chains, records)
    n = records << log2_chains
    f = eng.ladder_free_energies(tol=1e-8)["f"]
    targets = np.geomspace(0.5, 3.0, n_targets)
    dp = ctypes.POINTER(ctypes.c_double)

    energies = eng.energy_samples()
    eng.record_observables([0, 1])
    eng.set_energy_samples(energies)
    one_bin, many_bins = lane_patterns(eng.n_chains)           # (the 64 bins as an 8 x 8 block of the grid)
    inputs = (("every sample in one cell", np.stack([one_bin + 0.5] * 2)),
              ("consecutive samples in 64 different cells", np.stack([many_bins // 8 + 0.5, many_bins % 8 + 0.5])))
    print("K = %d, %d samples, %d targets" % (k, n, n_targets), flush=True)
    for label, rows in inputs:
        eng.set_observable_samples(np.broadcast_to(rows[None, :, :], (records, 2, eng.n_chains)))
        print("    %s" % label, flush=True)
        for g in grids:
            edges = np.linspace(0.0, float(g), g + 1)
            cells = (g + 3) * (g + 3)
            r = forced_rows if forced_rows and (32 * forced_rows + 2) * cells <= 64 * 1024 else surface_gram_rows(cells)
            out = eng.free_energy_surface_uncertainties(0, edges, 1, edges, targets, f, covariance=False)
            assert out["counts_slots"].sum() == n and np.all(np.isfinite(out["d_mass_slots"]))
            h = np.zeros((n_targets, k + 1, cells))
            sums = best(lambda: eng._check(eng._lib.me_mbar_histogram_joint_gram(
                eng._handle, f.ctypes.data_as(dp), targets.ctypes.data_as(dp), n_targets, 0, edges.ctypes.data_as(dp), g, 1,
                edges.ctypes.data_as(dp), g, h.ctypes.data_as(dp), None, None, None, None, None, None)))
            passes = n_targets * -(-(k + 1) // r)
            if sums_only:
                print("        %2d x %2d bins (%4d cells): cell Gram sums %.3f ms (R = %d: %d passes)" % (g, g, cells, sums, r, passes),
                      flush=True)
                continue
            plain = best(lambda: eng.free_energy_surface(0, edges, 1, edges, targets, f))
            whole = best(lambda: eng.free_energy_surface_uncertainties(0, edges, 1, edges, targets, f))
            lean = best(lambda: eng.free_energy_surface_uncertainties(0, edges, 1, edges, targets, f, covariance=False))
            plain_passes = -(-n_targets // surface_rows(cells))
            print("        %2d x %2d bins (%4d cells): free_energy_surface %.3f ms (%d passes); cell Gram sums %.3f ms (R = %d: %d more "
                  "passes) = %.2f x, %.3f ms per added pass; free_energy_surface_uncertainties %.3f ms = %.2f x, with covariance=False "
                  "%.3f ms" % (g, g, cells, plain, plain_passes, sums, r, passes, sums / plain, (sums - plain) / passes, whole,
                               whole / plain, lean), flush=True)
    # the host algebra alone on a full grid: random positive sums of the right shapes (every cell live)
    rng = np.random.default_rng(5)
    for g in () if sums_only else grids:
        edges = np.linspace(0.0, float(g), g + 1)
        cells = (g + 3) * (g + 3)
        mass = rng.random((n_targets, g + 3, g + 3)) + 0.1
        mass /= mass.reshape(n_targets, -1).sum(axis=1)[:, None, None]
        w = rng.random((4 * k, k)) / (4 * k)
        args = (targets, edges, edges, mass, np.ones((g + 3, g + 3), dtype=np.int64), np.ones(n_targets),
                rng.random((n_targets, k + 1, cells)) * 1e-3, w.T @ w, np.full(k, 4.0), n, 1.0)
        with_cov = best(lambda: statistics._surface_uncertainty_result(*args, True))
        without = best(lambda: statistics._surface_uncertainty_result(*args, False))
        print("    host algebra, %2d x %2d bins, %d targets, all %d cells live: %.3f ms with the cell covariance, %.3f ms without"
              % (g, g, n_targets, cells, with_cov, without), flush=True)


def time_newton(k, log2_chains, records, dim=DIM, ratio=None):
    """One pass and the whole solve of me_mbar_solve_newton (csrc/me_mbar_newton.hip) beside me_mbar_solve on the same samples
    in the same run.  A pass = (wall time of a solve limited to b passes - one limited to a passes) / (b - a) at a tolerance no
    iterate meets, which leaves the counting pass, the allocations and the read-backs out: for Newton the pass kernel, the sum
    of the block partials and the one-wavefront update (a = 3: Newton passes only), for the self-consistent solver
    k_mbar_weights and k_mbar_update.  Beside them me_mbar_gram without targets (k_mbar_gram over the K ladder columns), a
    WHOLE call: its counting pass, minimum pass, k_mbar_gram, the finish kernel and the copy of G; the pair "k_mbar_weights plus
    a ladder-only k_mbar_gram pass" is the self-consistent pass plus this call.  ``ratio``: T_k = 0.5 ratio^k instead of the
    ladder that spans 0.5 ... 0.5 1.3^7."""
    import ctypes
    n = 1 << log2_chains
    temps = ladder(k) if ratio is None else 0.5 * ratio ** np.arange(k)
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=n, seed=3, dtype="f64", temperatures=temps)
    eng.record_energies(records)
    rng = np.random.default_rng(1)
    eng.set_energy_samples(rng.gamma(dim / 2.0, 1.0, size=(records, n)) * np.repeat(temps, n // k)[None, :])

    def per_pass(method, a, b):
        few = best(lambda: eng.ladder_free_energies(tol=1e-300, max_iter=a, method=method))
        many = best(lambda: eng.ladder_free_energies(tol=1e-300, max_iter=b, method=method))
        return (many - few) / (b - a)

    newton_pass, plain_pass = per_pass("newton", 3, 19), per_pass("self-consistent", 1, 33)
    f = eng.ladder_free_energies(tol=1e-10, method="newton")["f"]
    dp = ctypes.POINTER(ctypes.c_double)
    gram, counts = np.zeros((k, k)), np.zeros(k)
    gram_call = best(lambda: eng._check(eng._lib.me_mbar_gram(eng._handle, f.ctypes.data_as(dp), None, 0, gram.ctypes.data_as(dp),
                                                               counts.ctypes.data_as(dp), None, None, None)))
    print("K = %2d, dim %d, T_k / T_k-1 = %.4f, %d samples: Newton pass %.3f ms; self-consistent pass %.3f ms; ladder-only "
          "me_mbar_gram call %.3f ms; Newton pass / (self-consistent pass + Gram call) = %.2f, / self-consistent pass = %.2f"
          % (k, dim, temps[1] / temps[0], records << log2_chains, newton_pass, plain_pass, gram_call,
             newton_pass / (plain_pass + gram_call), newton_pass / plain_pass), flush=True)
    line = "       whole solve to tol 1e-10:"
    for method in ("newton", "self-consistent"):
        out = eng.ladder_free_energies(tol=1e-10, method=method)
        ms = best(lambda: eng.ladder_free_energies(tol=1e-10, method=method), repeats=2)
        line += " %s %.2f ms, %d iterations, residual %.1e%s;" % (
            method, ms, out["iterations"], out["residual"],
            ", gradient %.1e, %d fallback passes" % (out["gradient"], out["fallback_steps"]) if method == "newton" else "")
        if method == "newton":
            newton_ms, f_newton = ms, out["f"]
        else:
            line += " self-consistent / Newton = %.2f; max |f - f_Newton| = %.1e" % (ms / newton_ms, np.max(np.abs(out["f"] - f_newton)))
    print(line, flush=True)


def time_inefficiency(k, log2_chains, records, columns=(0, 4, 16), phi=0.9):
    """me_recorded_inefficiency (csrc/me_series.hip) over the energy store and Q recorded columns: the whole call as users make
    it (the walks stop where the autocorrelation first turns non-positive, so only the first batches of 64 lags are computed)
    and with every lag up to records - 2 (mintime = records: no walk stops).  Every column is an AR(1) series with coefficient
    ``phi``.  For scale, the host route on ONE rung: energy_samples() and the pooled estimator in numpy."""
    n = 1 << log2_chains
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=n, seed=3, dtype="f64", temperatures=ladder(k))
    eng.record_energies(records)
    rng = np.random.default_rng(1)
    x = np.empty((records, n))
    x[0] = rng.standard_normal(n)
    for r in range(1, records):
        x[r] = phi * x[r - 1] + np.sqrt(1.0 - phi * phi) * rng.standard_normal(n)

    for q in columns:
        eng.record_observables([j % 4 for j in range(q)] if q else None)
        eng.set_energy_samples(x)
        if q:
            eng.set_observable_samples(np.repeat(x[:, None, :], q, axis=1) * (1.0 + 0.125 * np.arange(q))[None, :, None])
        out = eng.recorded_inefficiency()
        batches = int(out["stop_lag"].max()) // 64 + 1
        ms = best(eng.recorded_inefficiency)
        full_ms = best(lambda: eng.recorded_inefficiency(mintime=records), repeats=1)
        print("K = %d, %d chains x %d records, Q = %2d: g %.2f ... %.2f (exact %.2f), largest stop lag %d: %d batch(es) of 64 lags "
              "%.3f ms; all %d lags %.3f ms = %.3f ms per batch and column"
              % (k, n, records, q, out["g"].min(), out["g"].max(), (1 + phi) / (1 - phi), out["stop_lag"].max(), batches, ms,
                 records - 2, full_ms, full_ms / ((records - 2) // 64 + 1) / (1 + q)), flush=True)
    # the host route, one rung of the energy column
    m = n // k
    t0 = time.perf_counter()
    a = eng.energy_samples()[:, :m]
    copy_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    d = a - a.mean()
    p0 = np.sum(d * d)
    g, t = 1.0, 1
    while t < records - 1:
        c = np.sum(d[:records - t] * d[t:]) * records / (p0 * (records - t))
        if c <= 0.0 and t > 3:
            break
        g += 2.0 * c * (1.0 - t / records)
        t += 1
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    print("host route: energy_samples() %.1f ms (%d MB), then numpy on ONE rung of %d chains %.1f ms to stop lag %d (g = %.2f): "
          "%.0f ms for %d rungs" % (copy_ms, records * n * 8 >> 20, m, numpy_ms, t, g, copy_ms + k * numpy_ms, k), flush=True)


def time_reference(k, log2_samples):
    n = 1 << log2_samples
    temps = ladder(k)
    rng = np.random.default_rng(2)
    rungs = np.repeat(np.arange(k), n // k)
    e = rng.gamma(DIM / 2.0, 1.0, size=n) * temps[rungs]
    f = np.zeros(k)
    ref.iterate(e, rungs, temps, f)
    t0 = time.perf_counter()
    for _ in range(3):
        f, _ = ref.iterate(e, rungs, temps, f)
    ms = 1e3 * (time.perf_counter() - t0) / 3
    print("K = %2d: numpy reference, %d samples: %.1f ms per iteration; scaled to 2^25 samples: %.0f ms"
          % (k, n, ms, ms * (1 << 25) / n), flush=True)


def time_record(log2_chains=20, dtype="f32", calls=50):
    n = 1 << log2_chains
    eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.0] * DIM, None, temp=1.0, n_chains=n, seed=1, dtype=dtype)
    eng.record_energies(calls + 1)
    eng.record_energy()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        eng.record_energy()
    eng.sync()
    us = 1e6 * (time.perf_counter() - t0) / calls
    traffic = n * (8 + (4 if dtype == "f32" else 8))
    print("me_energy_samples_record, %d chains, %s, one ledger row: %.1f us per call back to back, %d bytes of traffic: %.0f GB/s"
          % (n, dtype, us, traffic, 1e-9 * traffic / (1e-6 * us)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-chains", type=int, default=15)
    ap.add_argument("--records", type=int, default=1024)
    ap.add_argument("--rungs", type=int, nargs="*", default=[8, 16, 32])
    ap.add_argument("--reference-log2", type=int, default=20)
    ap.add_argument("--one-solve", type=int, default=0)
    ap.add_argument("--gram", action="store_true")
    ap.add_argument("--observables", action="store_true")
    ap.add_argument("--perturbed", action="store_true")
    ap.add_argument("--observable-gram", action="store_true")
    ap.add_argument("--fluctuations", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-uncertainty", action="store_true")
    ap.add_argument("--surface", action="store_true")
    ap.add_argument("--surface-uncertainty", action="store_true")
    ap.add_argument("--sums-only", action="store_true", help="with --surface-uncertainty: time the cell Gram sums alone")
    ap.add_argument("--newton", action="store_true")
    ap.add_argument("--rows-per-pass", type=int, default=0, help="with --profile-uncertainty: the R of a -DME_HIST_COV_ROWS=R library; "
                    "with --surface: of a -DME_HIST2D_ROWS=R library; with --surface-uncertainty: of a -DME_HIST2D_COV_ROWS=R library")
    ap.add_argument("--grids", type=int, nargs="*", default=[8, 16, 33], help="with --surface and --surface-uncertainty: the bins per axis")
    ap.add_argument("--inefficiency", action="store_true")
    cli = ap.parse_args()
    if cli.inefficiency:
        time_inefficiency(8, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.newton:
        for k in (8, 32, 64):
            time_newton(k, cli.log2_chains, cli.records)
        time_newton(16, cli.log2_chains, max(1, cli.records // 32), dim=64, ratio=1.35)     # the poorly overlapping ladder
        sys.exit(0)
    if cli.surface_uncertainty:
        for k in cli.rungs:
            time_surface_uncertainty(k, cli.log2_chains, cli.records, grids=cli.grids, forced_rows=cli.rows_per_pass,
                                     sums_only=cli.sums_only)
        sys.exit(0)
    if cli.surface:
        time_surface(8, cli.log2_chains, cli.records, grids=cli.grids, forced_rows=cli.rows_per_pass)
        sys.exit(0)
    if cli.profile:
        time_profile(8, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.profile_uncertainty:
        for k in cli.rungs:
            time_profile_uncertainty(k, cli.log2_chains, cli.records, forced_rows=cli.rows_per_pass)
        sys.exit(0)
    if cli.fluctuations:
        for k in cli.rungs:
            time_fluctuations(k, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.perturbed:
        for k in cli.rungs:
            time_perturbed(k, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.observable_gram:
        for k in cli.rungs:
            time_observable_gram(k, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.observables:
        time_observables(8, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.gram:
        for k in cli.rungs:
            time_gram(k, cli.log2_chains, cli.records)
        sys.exit(0)
    if cli.one_solve:
        time_solve(cli.one_solve, cli.log2_chains, cli.records)
        sys.exit(0)
    for k in cli.rungs:
        time_solve(k, cli.log2_chains, cli.records)
    for k in cli.rungs:
        time_reference(k, cli.reference_log2)
    for dtype in ("f32", "f64"):
        time_record(dtype=dtype)
