"""Every dense matrix-core product held to the per-chain forward-error bound of tests/dense_product_reference.py.

The probe reads a kernel's own product out of one ordinary step: crafted per-chain states, every ledger row set to a huge
finite value (so ``e_new - e <= 0`` accepts whatever the temperature and the uniform), and a width so small that
``x' = x`` bit for bit (energy leg) or ``x = 0`` with a power-of-two width (factor leg: ``x' = w L g`` exactly, and an
identity-shape engine with the same seed and chain ids yields ``g = x' / w`` -- every kernel draws g with the same
``Num<R>::normal_pair`` on the same Philox words in both shapes).  The reference is evaluated in long double on the state
read back.  Paths:

    dense64_f32   k_step_dense64_bf16x3<., 256> by default; METROPOLIS_DENSE64_THREADS=512 and
                  METROPOLIS_DENSE64_FP32_MFMA=1 (both read once per process) select the 512-thread instantiation and
                  k_step_dense64_mfma: the ``dense64_f32`` tests run again in one fresh child process each
    dense64_f64   k_step_dense64_f64
    generic16     the generic k_step with EnergyDense on the LDS-folded triangle, (16, 0), both types
    runtime       k_step_runtime_lds / tri_rows_mfma, both types, D = 97 (one row in the last 16-row block), 110 and 112
                  (D mod 4 != 0 clamps the B operand's k; 112 is a whole number of blocks)

Run with -s for the largest device ratio per path, type and class (DENSE_PRODUCT_GPU lines, in units of u)."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_product_reference as ref
import metropolisengine_amd as me
from metropolisengine_amd import _capi

pytestmark = pytest.mark.gpu

SEED = 3
if os.environ.get("METROPOLIS_DENSE64_FP32_MFMA", "")[:1] == "1":
    DENSE64_F32 = ("fp32_mfma", "fp32_mfma")                       # (label, gamma family)
elif os.environ.get("METROPOLIS_DENSE64_THREADS", "").strip() == "512":
    DENSE64_F32 = ("bf16x3_512", "bf16x3")
else:
    DENSE64_F32 = ("bf16x3_256", "bf16x3")

# path id -> (label, gamma family, dtype, D)
PATHS = {"dense64_f32": DENSE64_F32 + ("f32", 64), "dense64_f64": ("dense64_f64", "f64_mfma", "f64", 64)}
for _t in ("f32", "f64"):
    PATHS["generic16_" + _t] = ("generic16", "generic", _t, 16)
    for _d in (97, 110, 112):
        PATHS["runtime%d_%s" % (_d, _t)] = ("runtime", "runtime", _t, _d)
PATH_IDS = list(PATHS)
CHAIN_COUNTS = (1, 31, 33, 63, 65)          # beside the 197 of the class tests and the two-hot counts
N_CLASS = 197
BIG = {"f32": 1e30, "f64": 1e300}           # the ledger: every proposal goes downhill
TINY_WIDTH = {"f32": 2.0 ** -100, "f64": 2.0 ** -200}


def _engine(dtype, a, n, cov_mode="fixed"):
    d = a.shape[0]
    return me.MetropolisEngine(me.DenseQuadratic(a), None, [0.0] * d, None, temp=1.0, n_chains=n, seed=7, dtype=dtype,
                               sampling_width=0.1, cov_mode=cov_mode)


def _one_accepted_step(eng, x, width, dtype):
    n = x.shape[0]
    eng._set(_capi.FIELD_PARAMS, x)
    eng._set(_capi.FIELD_ENERGY, np.full((n, 1), BIG[dtype]))
    eng._set(_capi.FIELD_WIDTH, np.full((n, 1), width))
    eng.step_all()
    assert eng.accept_stats() == (n, n)
    return eng._get(_capi.FIELD_PARAMS), eng._get(_capi.FIELD_ENERGY).sum(axis=1)


def probe_energy(dtype, a, x):
    """(state read back, the kernel's x'^T (A x')) per chain."""
    x1, e = _one_accepted_step(_engine(dtype, a, x.shape[0]), x, TINY_WIDTH[dtype], dtype)
    assert np.array_equal(x1[x != 0], x[x != 0])
    return x1, e


def probe_factor(dtype, a, l, n):
    """(g, the kernel's L g) per chain."""
    d, w = a.shape[0], 2.0 ** -4
    zero = np.zeros((n, d))
    g = _one_accepted_step(_engine(dtype, a, n), zero, w, dtype)[0] / w
    shared = _engine(dtype, a, n, cov_mode="pooled")
    shared.set_shared_factor(l[np.tril_indices(d)])
    y = _one_accepted_step(shared, zero, w, dtype)[0] / w
    return g, y


def _report(path, name, ratio, bound, cap=None):
    label, _, dtype, d = PATHS[path]
    u = ref.UNIT_ROUNDOFF[dtype]
    print("\nDENSE_PRODUCT_GPU path=%s dtype=%s D=%d class=%s ratio=%.2f u gamma=%.0f u%s"
          % (label, dtype, d, name, ratio / u, bound / u, "" if cap is None else " cap=%.2f u" % (cap / u)))


@functools.lru_cache(maxsize=None)
def class_cap(name, d=64):
    """The calibrated cap of a class on its 197-chain inputs: a separation measured on a sample, also applied to the runs
    of the same class (and the same matrix) at fewer chains, where one or a few chains would make it a matter of luck."""
    return ref.calibrated_cap(*ref.make_case(name, d, SEED, "f32", N_CLASS))[0]


def check_energy(path, name, a, x, e=None, x1=None, cap=None):
    """gamma for every chain; where the kernel splits, the calibrated cap -- ``cap``, or computed on these inputs.
    Returns the kernel's energies."""
    label, family, dtype, d = PATHS[path]
    if e is None:
        x1, e = probe_energy(dtype, a, x)
    err = np.abs(np.asarray(e, dtype=ref.LD) - ref.quadratic_form_ld(a, x1))
    ratio = np.asarray(err / ref.abs_form(a, x1), dtype=np.float64)
    bound = ref.gamma(family, d, dtype)
    if family != "bf16x3":
        cap = None
    elif cap is None:
        cap = ref.calibrated_cap(a, x1)[0]
    _report(path, name, ratio.max(), bound, cap)
    assert np.all(ratio <= bound), (ratio.max(), bound)
    if cap is not None:
        assert ratio.max() <= cap, (ratio.max(), cap)
    return e


@pytest.mark.parametrize("name", ref.CLASSES)
@pytest.mark.parametrize("path", PATH_IDS)
def test_energy_on_every_class(path, name):
    _, _, dtype, d = PATHS[path]
    check_energy(path, name, *ref.make_case(name, d, SEED, dtype, N_CLASS))


@pytest.mark.parametrize("n", CHAIN_COUNTS)
@pytest.mark.parametrize("path", PATH_IDS)
def test_energy_at_every_lane_map(path, n):
    """Fewer chains than a tile, one short of and one past a 32- and a 64-chain tile: lanes that shadow the last chain."""
    _, _, dtype, d = PATHS[path]
    check_energy(path, "spd/n=%d" % n, *ref.make_case("spd", d, SEED, dtype, n),
                 cap=class_cap("spd") if path == "dense64_f32" else None)


@pytest.mark.parametrize("path", PATH_IDS)
def test_energy_scales_bitwise_with_a_power_of_two(path):
    _, _, dtype, d = PATHS[path]
    a, x = ref.make_case("pow2_scaled", d, SEED, dtype, N_CLASS)
    e = check_energy(path, "pow2_scaled/k=0", a, x)
    for k in (ref.POW2_SHIFT[dtype], -ref.POW2_SHIFT[dtype]):
        scaled = check_energy(path, "pow2_scaled/k=%d" % k, a * 2.0 ** k, x)
        assert np.array_equal(scaled, e * 2.0 ** k)


@pytest.mark.parametrize("path", PATH_IDS)
def test_energy_exact_two_hot(path):
    """Every retained product and partial sum is an integer: the kernel must return what integer arithmetic gives, bit for
    bit, for every pair of positions (a dropped, extra or misplaced product or fragment changes it)."""
    _, family, dtype, d = PATHS[path]
    split = family == "bf16x3"
    a, x, code = ref.two_hot_case(d, SEED, split)
    want, unfused, tie = ref.two_hot_expected(d, code, split)     # (the same two unless the kernel splits)
    assert not tie
    x1, e = probe_energy(dtype, a, x)
    assert np.all(x1 != 0) and np.max(np.abs(x1[x == 0])) < 1e-28
    check_energy(path, "exact_two_hot", a, x, e, x1)
    bad = np.flatnonzero((e != want) & (e != unfused))
    i, j = ref.two_hot_pairs(d)
    assert bad.size == 0, "%d of %d chains differ; first (i, j) = (%d, %d): %r != %r" % (
        bad.size, want.size, i[bad[0]], j[bad[0]], e[bad[0]], want[bad[0]])


@functools.lru_cache(maxsize=None)
def factor_case(d, dtype):
    """(A, L): L = chol of an SPD matrix without structure, rounded to the type."""
    a, _ = ref.make_case("spd", d, SEED, dtype, N_CLASS)
    b, _ = ref.make_case("asymmetric", d, SEED + 1, dtype, N_CLASS)
    l = np.linalg.cholesky(0.5 * np.linalg.inv(a) + 0.05 * b @ b.T / d)
    return a, l.astype(ref.NUMPY_DTYPE[dtype]).astype(np.float64)


@functools.lru_cache(maxsize=None)
def factor_cap():
    """The calibrated cap of the split L g on 197 vectors of float32 normals: a sample, applied at every chain count."""
    g = np.random.default_rng(SEED).standard_normal((N_CLASS, 64)).astype(np.float32).astype(np.float64)
    return ref.calibrated_cap(factor_case(64, "f32")[1], g, model=ref.split_bf16_product, ratio=ref.matvec_ratio,
                              defects=ref.FACTOR_DEFECTS)[0]


@pytest.mark.parametrize("n", CHAIN_COUNTS + (N_CLASS,))
@pytest.mark.parametrize("path", PATH_IDS)
def test_shared_factor_product(path, n):
    """x' = w L g read out exactly, at every lane map: componentwise against gamma_L |L| |g|."""
    label, family, dtype, d = PATHS[path]
    a, l = factor_case(d, dtype)
    g, y = probe_factor(dtype, a, l, n)
    assert np.all(np.isfinite(g)) and 0.5 < np.std(g) < 1.5          # (over all n x d components)
    err = np.abs(np.asarray(y, dtype=ref.LD) - ref.matvec_ld(l, g))
    ratio = np.asarray(err / ref.abs_matvec(l, g), dtype=np.float64)
    bound = ref.gamma(family, d, dtype, "factor")
    cap = factor_cap() if family == "bf16x3" else None
    _report(path, "L g/n=%d" % n, ratio.max(), bound, cap)
    assert np.all(ratio <= bound), (ratio.max(), bound)
    if cap is not None:
        assert ratio.max() <= cap, (ratio.max(), cap)


def test_energy_dense64_f32_persistent_grid_second_trip(monkeypatch):
    """Just more chains than CUs x 1024: some workgroups of the persistent grid take the ``base += stride`` second trip.
    The split-bf16 launchers cap their grid at CUs x 1024 chains by themselves; launch_step_dense64_mfma caps it only on
    request, so for that variant ME_GRID_BLOCKS (read when the engine is created) asks for 2 x CUs blocks of 512 threads.
    The states repeat a block of 1 024 distinct chains, so the reference and the cap are computed once on that block, and
    every repeat -- whichever workgroup and trip it lands on -- must return the block's energies bit for bit."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if DENSE64_F32[0] == "fp32_mfma":
        monkeypatch.setenv("ME_GRID_BLOCKS", str(2 * cus))
    n, block = cus * 1024 + 3 * 64 + 5, 1024
    a, xb = ref.make_case("spd", 64, SEED, "f32", block)
    x = np.tile(xb, ((n + block - 1) // block, 1))[:n]
    x1, e = probe_energy("f32", a, x)
    check_energy("dense64_f32", "spd/n=%d" % n, a, xb, e[:block], x1[:block])
    assert np.array_equal(e, np.tile(e[:block], (n + block - 1) // block)[:n])


# ---------------------------------------------------------------------------------------------------- the other variants
def _count_dense64_f32_cases():
    return len(ref.CLASSES) + len(CHAIN_COUNTS) + 1 + 1 + (len(CHAIN_COUNTS) + 1) + 1


@pytest.mark.parametrize("variant,env", [("threads512", {"METROPOLIS_DENSE64_THREADS": "512"}),
                                         ("fp32_mfma", {"METROPOLIS_DENSE64_FP32_MFMA": "1"})])
def test_dense64_f32_variant_in_child_process(variant, env):
    """The kernel choice is read once per process: every dense64_f32 case again in ONE fresh child test process."""
    base = {k: v for k, v in os.environ.items() if k not in ("METROPOLIS_DENSE64_THREADS", "METROPOLIS_DENSE64_FP32_MFMA")}
    try:
        res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k",
                              "dense64_f32 and not child_process", "-p", "no:cacheprovider"], env=dict(base, **env),
                             capture_output=True, text=True, timeout=600,
                             cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    except subprocess.TimeoutExpired:
        pytest.exit("the %s child process hung: nothing more is started on this device" % variant, returncode=1)
    print("\n" + "\n".join(line for line in res.stdout.splitlines() if line.startswith("DENSE_PRODUCT_GPU")))
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139):
        # the child died of a signal: nothing more is started on a device that may have faulted
        pytest.exit("the %s child process died with status %d:\n%s" % (variant, res.returncode, res.stderr[-2000:]), returncode=1)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    label = "bf16x3_512" if variant == "threads512" else "fp32_mfma"
    assert "path=%s " % label in res.stdout
    passed = re.search(r"(\d+) passed", res.stdout)
    assert passed and int(passed.group(1)) == _count_dense64_f32_cases(), res.stdout[-1000:]
