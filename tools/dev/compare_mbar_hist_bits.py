"""Dev tool: the four histogram units (csrc/me_mbar_hist.hip, me_mbar_hist_cov.hip, me_mbar_hist2d.hip,
me_mbar_hist2d_cov.hip) of two builds of the library, bit for bit (profiles/mbar_slot_skeleton.txt, profiles/mbar_gram_driver.txt).

    python tools/dev/compare_mbar_hist_bits.py LIB_A.so LIB_B.so     (one fresh process per library, then the comparison)
    python tools/dev/compare_mbar_hist_bits.py --dump OUT.npz        (the library that METROPOLIS_HIP_LIB selects)

Engine-less entry points on the same seeded host arrays: K = 8 and 33 rungs (and K = 1, so that a single sample is a
problem); 1, 2047, 2049, 3 * 2048 + 5 and 2048 * 2048 + 5 samples (a count below K leaves a rung empty: the return code is
compared); a few non-finite energies; values below, above, on the first and on the last edge, infinite and NaN, all 64 lanes
in one slot, 64 distinct slots; 1, 64, 256 bins (masses), 64, 100, 256 bins with 5 temperatures (Gram sums: R = 16, 8, 4), grids
12 x 7, 20 x 20, 33 x 33 with 9 temperatures (R = 4, 2, 1) and, for the cell Gram sums, with 5 (R = 8, 2, 1) besides 4 x 12 and
6 x 9 (R = 16, 8: one grid on either side of a threshold).  An axis that IS the energy exists in the engine form only
(me_mbar_histogram_joint with column -1): 31 records of 512 chains, 7 of 2112, a ragged eighth tile.  Every output array of every call is
compared with np.array_equal on its bits."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
DP, IP, LP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
SIZES = (1, 2047, 2049, 3 * 2048 + 5, 2048 * 2048 + 5)
BINS_1D, BINS_GRAM, GRIDS = (1, 64, 256), (64, 100, 256), ((12, 7), (20, 20), (33, 33))
GRIDS_GRAM = ((4, 12), (6, 9))          # 105 and 108 cells: either side of the cell Gram sums' step from R = 16 to 8 at 106


def dp(a):
    return a.ctypes.data_as(DP)


def problem(k, n, seed):
    """Energies E / T Gamma(8) on a geometric ladder with the exact f_k = -8 ln T_k (up to a constant), rungs in turn."""
    rng = np.random.default_rng(seed)
    temps = 0.5 * (1.3 ** 7) ** (np.arange(k) / max(k - 1.0, 1.0))
    rungs = (np.arange(n) % k).astype(np.int32)
    energies = rng.gamma(8.0, 1.0, size=n) * temps[rungs]
    if n > 1000:
        energies[[5, 700, n - 3]] = np.nan, np.inf, -np.inf
    return temps, rungs, energies, -8.0 * np.log(temps / temps[0]), np.geomspace(0.55, 2.9, 9)


def value_patterns(n, top, rng):
    """Three value columns for edges linspace(0, top, .): spread over and beyond the edges with the corners, every value in one
    slot, 64 consecutive samples in 64 different slots (where there are that many)."""
    spread = rng.uniform(-0.1 * top, 1.1 * top, size=n)
    corners = [-np.inf, np.inf, np.nan, float(top), 0.0, -1e-300, np.nextafter(float(top), 0.0)]
    at = rng.choice(n, size=min(n, len(corners)), replace=False)
    spread[at] = corners[:at.size]
    i = np.arange(n)
    return {"spread": spread, "one slot": np.full(n, 0.5), "64 slots": (i % 64) * (top / 64.0) + top / 128.0}


def grid_patterns(n, bx, by, rng):
    """:func:`value_patterns` for the two axes of a grid, with 64 consecutive samples in 64 different CELLS."""
    xs, ys = value_patterns(n, bx, rng), value_patterns(n, by, rng)
    i = np.arange(n)
    per = min(by, 8)
    xs["64 slots"], ys["64 slots"] = (i % 64) // per + 0.5, (i % 64) % per + 0.5
    return xs, ys


def dump(path):
    import metropolisengine_amd as me
    from metropolisengine_amd import _capi
    lib, out = _capi.load(), {}

    def keep(label, rc, **arrays):
        out[label + " rc"] = np.array(rc)
        for name, a in arrays.items():
            out[label + " " + name] = a

    for k in (1, 8, 33):
        for n in SIZES if k > 1 else (1,):
            temps, rungs, energies, f, targets = problem(k, n, seed=1000 * k + n % 997)
            rng = np.random.default_rng(n + k)
            head = (0, dp(energies), rungs.ctypes.data_as(IP), n, dp(temps), k, dp(f))
            for b in sorted(set(BINS_1D + BINS_GRAM)):
                edges = np.linspace(0.0, float(b), b + 1)
                for pattern, values in value_patterns(n, b, rng).items():
                    label = "K=%d n=%d %d bins %s:" % (k, n, b, pattern)
                    if b in BINS_1D:
                        mass, counts, neff = np.zeros((9, b + 3)), np.zeros(b + 3, dtype=np.int64), np.zeros(9)
                        rc = lib.me_mbar_histogram_samples(*head, dp(targets), 9, dp(values), dp(edges), b, dp(mass),
                                                           counts.ctypes.data_as(LP), dp(neff))
                        keep(label + " masses", rc, mass=mass, counts=counts, neff_fraction=neff)
                    if b in BINS_GRAM:
                        h, ladder, cc = np.zeros((5, k + 1, b + 3)), np.zeros((k, k)), np.zeros(k)
                        mass, counts, neff = np.zeros((5, b + 3)), np.zeros(b + 3, dtype=np.int64), np.zeros(5)
                        n_used = ctypes.c_int64()
                        rc = lib.me_mbar_histogram_gram_samples(*head, dp(targets), 5, dp(values), dp(edges), b, dp(h), dp(ladder),
                                                                dp(cc), dp(mass), counts.ctypes.data_as(LP), dp(neff),
                                                                ctypes.byref(n_used))
                        keep(label + " gram", rc, slot_gram=h, ladder_gram=ladder, column_counts=cc, mass=mass, counts=counts,
                             neff_fraction=neff, n_used=np.array(n_used.value))
            for bx, by in GRIDS:
                ex, ey = np.linspace(0.0, float(bx), bx + 1), np.linspace(0.0, float(by), by + 1)
                xs, ys = grid_patterns(n, bx, by, rng)
                for pattern in xs:
                    mass, counts, neff = np.zeros((9, bx + 3, by + 3)), np.zeros((bx + 3, by + 3), dtype=np.int64), np.zeros(9)
                    rc = lib.me_mbar_histogram_joint_samples(*head, dp(targets), 9, dp(xs[pattern]), dp(ys[pattern]), dp(ex), bx,
                                                             dp(ey), by, dp(mass), counts.ctypes.data_as(LP), dp(neff))
                    keep("K=%d n=%d %d x %d bins %s: joint" % (k, n, bx, by, pattern), rc, mass=mass, counts=counts,
                         neff_fraction=neff)
            for bx, by in GRIDS + GRIDS_GRAM:
                ex, ey = np.linspace(0.0, float(bx), bx + 1), np.linspace(0.0, float(by), by + 1)
                xs, ys = grid_patterns(n, bx, by, rng)
                for pattern in xs:
                    h, ladder, cc = np.zeros((5, k + 1, (bx + 3) * (by + 3))), np.zeros((k, k)), np.zeros(k)
                    mass, counts, neff = np.zeros((5, bx + 3, by + 3)), np.zeros((bx + 3, by + 3), dtype=np.int64), np.zeros(5)
                    n_used = ctypes.c_int64()
                    rc = lib.me_mbar_histogram_joint_gram_samples(*head, dp(targets), 5, dp(xs[pattern]), dp(ys[pattern]), dp(ex),
                                                                  bx, dp(ey), by, dp(h), dp(ladder), dp(cc), dp(mass),
                                                                  counts.ctypes.data_as(LP), dp(neff), ctypes.byref(n_used))
                    keep("K=%d n=%d %d x %d bins %s: joint gram" % (k, n, bx, by, pattern), rc, cell_gram=h, ladder_gram=ladder,
                         column_counts=cc, mass=mass, counts=counts, neff_fraction=neff, n_used=np.array(n_used.value))
    # the engine form, for an axis that is the energy (column -1) in either position
    for k in (8, 33):
        m, records = 64, 31 if k == 8 else 7            # 15 872 and 14 784 samples: seven tiles and a ragged eighth
        temps, _, _, f, targets = problem(k, k, seed=0)
        rng = np.random.default_rng(k)
        e = rng.gamma(8.0, 1.0, size=(records, k * m)) * np.repeat(temps, m)[None, :]
        e[3, 5], e[records - 2, 100] = np.nan, np.inf
        eng = me.MetropolisEngine(me.IsoQuadratic(1.0), None, [0.1], None, n_chains=k * m, seed=5, dtype="f64", temperatures=temps)
        eng.record_energies(records)
        eng.record_observables([0, 0])
        eng.set_energy_samples(e)
        for bx, by in GRIDS:
            cols = np.stack([value_patterns(e.size, bx, rng)["spread"].reshape(e.shape),
                             value_patterns(e.size, by, rng)["spread"].reshape(e.shape)], axis=1)
            eng.set_observable_samples(cols)
            span = 12.0 * temps[-1]
            for cx, cy in ((-1, 1), (0, -1), (-1, -1), (0, 1)):
                ex = np.linspace(0.0, span if cx < 0 else float(bx), bx + 1)
                ey = np.linspace(0.0, span if cy < 0 else float(by), by + 1)
                mass, counts, neff = np.zeros((9, bx + 3, by + 3)), np.zeros((bx + 3, by + 3), dtype=np.int64), np.zeros(9)
                rc = lib.me_mbar_histogram_joint(eng._handle, dp(f), dp(targets), 9, cx, dp(ex), bx, cy, dp(ey), by, dp(mass),
                                                 counts.ctypes.data_as(LP), dp(neff))
                keep("engine K=%d %d x %d bins columns (%d, %d): joint" % (k, bx, by, cx, cy), rc, mass=mass, counts=counts,
                     neff_fraction=neff)
    np.savez(path, **out)
    ok = sum(1 for name in out if name.endswith(" rc") and out[name] == 0)
    print("%s: %d calls, %d returned 0, %d arrays" % (os.environ.get("METROPOLIS_HIP_LIB", "the built library"),
                                                     sum(1 for name in out if name.endswith(" rc")), ok, len(out)), flush=True)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files)
    different, filled = [], 0
    for name in a.files:
        x, y = a[name], b[name]
        same = x.shape == y.shape and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                     y.view(np.uint64) if y.dtype == np.float64 else y)
        filled += int(np.any(x != 0))
        if not same:
            different.append(name)
    fields = sorted({name.rsplit(" ", 1)[1] for name in a.files})
    print("%d arrays (%d not all zero) of the fields %s: %s" % (len(a.files), filled, ", ".join(fields),
                                                                "all EQUAL" if not different else "%d DIFFERENT" % len(different)))
    for name in different[:40]:
        print("    DIFFERENT: " + name)
    return 1 if different else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        dump(sys.argv[2])
        sys.exit(0)
    if len(sys.argv) != 3 or sys.argv[1].startswith("-"):
        sys.exit(__doc__.split("\n\n")[1])
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for idx, lib in enumerate(sys.argv[1:3]):
            paths.append(os.path.join(tmp, "%d.npz" % idx))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", paths[-1]], check=True, timeout=300,
                           env=dict(os.environ, METROPOLIS_HIP_LIB=os.path.abspath(lib)))
        sys.exit(compare(*paths))
