"""Every stage-1 kernel of the pooled-moment reduction (and k_pool_finish behind it) held to exact sums on integer states and
to the forward-error bound of tests/pooled_moments_reference.py on float states.

The probe: an engine with ``cov_mode="fixed"``, the crafted state written with ``_set(FIELD_PARAMS, x)`` and read back
(it must come back bit for bit, so the reference of x is the reference of the device state), then ``pooled_moments()``
twice.  Nothing steps: ``m[0] == n`` and the two trailing counters are 0.  Paths (``ref.conformance_cases``):

    gram32            k_pool_gram32<NR,NC> / k_pool_gram32_f64<NR,NC>: every prebuilt set with D + nr + nc <= 32; 1, 63, 65, 197
                      and 64 x 16 + 5 chains; (2, 7) and (16, 0) past 256 workgroups x 16 / 8 wavefronts (a wavefront's second
                      tile: the prefetched ``next[]``, the slab rewritten between the barriers)
    gram64            k_pool_gram64 / k_pool_gram64_f64: 1, 31, 65, 197 chains and 1 027 tiles (second trip)
    generic64         k_pool_reduce<R, 64>, component-major state of the runtime-dimension engines: (97, 0), (60, 25); (97, 0)
                      at 850 tiles on 847 blocks
    generic64_tiled   k_pool_reduce<R, 64> on the tile-major state of the on-demand (96, 0) kernel set
    generic32         k_pool_reduce<R, 32>: (160, 0) float64, (316, 0) float32, 197 and 33 chains (7 and 2 tiles of 32 chains
                      on 4 and 1 blocks: every block loops)
    generic16         k_pool_reduce<double, 16>: (312, 0), 197 and 17 chains

The float32 second-trip cases also run ``wide_integers``, whose tile sums fill float32's 24 bits: exact only if nothing is
carried in float32 from a wavefront's (a block's) first tile into its second.  Every case first asks the engine which first
stage it launches (``pooled_moments_geometry``): the kernel family, the chains per tile and the rows of partial sums must
be the ones the case is named for.

And, on ``integers`` only, the other doors to the same kernels: ``pooled_moments_by_rung()`` (a tile-major range offset
into the field; a component-major range through the strided gather), ``pooled_moments_begin()`` / ``_end()``, and the two
counters after a few steps.

Run with -s for the largest ratio of every case (POOLED_MOMENTS_GPU lines, in units of the dtype's u)."""
import numpy as np
import pytest

import metropolisengine_amd as me
import pooled_moments_reference as ref
from metropolisengine_amd import _capi

pytestmark = pytest.mark.gpu

SEED = 3
CASES = ref.conformance_cases()


def _engine(path, nr, nc, dtype, n, **kw):
    real0, cplx0 = ([0.0] * nr if nr else None), ([0j] * nc if nc else None)
    if path.startswith("generic") and path != "generic64_tiled":
        energy = me.DiagQuadratic((1.0,) * nr, (1.0,) * nc)        # beyond 96 degrees of freedom: the runtime-dimension set
    else:
        energy = me.IsoQuadratic(1.0)
    kw.setdefault("temp", 1.0)
    return me.MetropolisEngine(energy, None, real0, cplx0, n_chains=n, seed=7, dtype=dtype, sampling_width=0.1,
                               cov_mode="fixed", **kw)


def _load(eng, x):
    eng._set(_capi.FIELD_PARAMS, x)
    assert np.array_equal(eng._get(_capi.FIELD_PARAMS), x)         # every value is representable: the device holds x itself


def _first_differences(got, s, nr, nc):
    bad = np.flatnonzero(np.asarray(got) != s.astype(np.float64))
    names = {v.start: k for k, v in ref.layout(nr, nc).items() if v.stop > v.start}
    return "%d of %d entries differ; sections start at %r; first: %s" % (
        bad.size, s.size, names, ", ".join("[%d] %r != %d" % (k, got[k], s[k]) for k in bad[:6]))


def _check(path, nr, nc, dtype, n, name, got, s, a):
    u, limit = ref.UNIT_ROUNDOFF[dtype], ref.bound(dtype, n, ref.path_family(path, dtype))
    ratio = ref.error_ratio(got, s, a)
    print("\nPOOLED_MOMENTS_GPU path=%s dtype=%s nr=%d nc=%d n=%d class=%s ratio=%.3f u bound=%.1f u"
          % (path, dtype, nr, nc, n, name, ratio.max() / u, limit / u))
    assert got[0] == n and got[-2] == 0 and got[-1] == 0
    if name in ("integers", ref.WIDE):
        assert ref.is_exact(got, s), _first_differences(got, s, nr, nc)
    else:
        worst = int(np.argmax(ratio))
        assert np.all(ratio <= limit), "entry %d: ratio %.3f u, bound %.1f u" % (worst, ratio[worst] / u, limit / u)


@pytest.mark.parametrize("path,nr,nc,dtype,n,name", CASES, ids=["%s-%d-%d-%s-n%d-%s" % c for c in CASES])
def test_pooled_moments(path, nr, nc, dtype, n, name):
    tile = {"generic32": 32, "generic16": 16}.get(path, 64)
    assert ref.path_tile(path, nr, nc, dtype) == tile
    x = ref.make_state(name, nr, nc, n, SEED, dtype)
    s, a = ref.exact_moments(x, nr, nc)
    eng = _engine(path, nr, nc, dtype, n)
    # the engine's own account of what it launches: the case holds the kernel it is named for, at the geometry the
    # reference's second-trip sizes and planted defects assume
    assert eng.pooled_moments_geometry() == (path.startswith("gram"), tile, ref.partial_rows(path, nr, nc, n))
    _load(eng, x)
    got = eng.pooled_moments()
    again = eng.pooled_moments()
    _check(path, nr, nc, dtype, n, name, got, s, a)
    assert np.array_equal(got, again)                              # fixed summation order: bit for bit


# ---------------------------------------------------------------------------------------------------- the other doors
@pytest.mark.parametrize("nr,nc,dtype", [(16, 0, "f32"), (4, 0, "f64"), (2, 2, "f32")])
def test_every_rung_equals_the_sums_of_its_slice(nr, nc, dtype):
    """(16, 0): a tile-major range is the field offset by whole tiles; (4, 0), (2, 2): the rows of a component-major range
    are gathered into a field of their own first.  Three rungs of 128 chains."""
    rungs, m = 3, 128
    x = ref.make_state("integers", nr, nc, rungs * m, SEED, dtype)
    eng = _engine("gram32", nr, nc, dtype, rungs * m, temp=0, temperatures=[0.5, 1.0, 2.0])
    _load(eng, x)
    got = eng.pooled_moments_by_rung()
    assert got.shape == (rungs, ref.moments_size(nr, nc))
    for k in range(rungs):
        s, a = ref.exact_moments(x[k * m:(k + 1) * m], nr, nc)
        _check("gram32/rung%d" % k, nr, nc, dtype, m, "integers", got[k], s, a)
    assert np.array_equal(got, eng.pooled_moments_by_rung())
    s, a = ref.exact_moments(x, nr, nc)
    _check("gram32/ladder", nr, nc, dtype, rungs * m, "integers", eng.pooled_moments(), s, a)


def test_split_reduction_equals_the_plain_one():
    nr, nc, dtype, n = 2, 7, "f32", 64 * 16 + 5
    x = ref.make_state("integers", nr, nc, n, SEED, dtype)
    s, a = ref.exact_moments(x, nr, nc)
    eng = _engine("gram32", nr, nc, dtype, n)
    _load(eng, x)
    plain = eng.pooled_moments()
    eng.pooled_moments_begin()
    split = eng.pooled_moments_end()
    _check("gram32/begin_end", nr, nc, dtype, n, "integers", split, s, a)
    assert np.array_equal(split, plain)


def test_the_trailing_counters_are_the_acceptance_counters():
    nr, nc, dtype, n = 2, 1, "f64", 197
    eng = _engine("gram32", nr, nc, dtype, n)
    _load(eng, 0.01 * ref.make_state("integers", nr, nc, n, SEED, dtype))
    eng.step_all(3)
    accepted, proposed = eng.accept_stats()
    got = eng.pooled_moments()
    assert proposed == 3 * n and 0 < accepted < proposed
    assert (got[-2], got[-1]) == (float(accepted), float(proposed)) and got[0] == n
    s, a = ref.exact_moments(eng._get(_capi.FIELD_PARAMS), nr, nc)
    assert np.all(ref.error_ratio(got[:-2], s[:-2], a[:-2]) <= ref.bound(dtype, n))
