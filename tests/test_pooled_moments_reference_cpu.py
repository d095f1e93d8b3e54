"""CPU tests of tests/pooled_moments_reference.py: the layout, the exact reference, that honest arithmetic sits well inside
the bound and is exact on both integer classes at every size of the GPU conformance module, and -- above all -- that every
planted defect is caught by the class named for it (no GPU).

float32 accumulation across tiles is planted with the launch geometry: wavefront w of the 4 096 of k_pool_gram32 adds its
tiles w + 4 096 k up in float32, the wavefronts' sums are added in float64 (and, second variant, in float32 as well).
``test_fp32_across_tiles_is_caught_by_wide_integers_and_not_by_the_bound`` records why the bound is not what catches it.
Largest error / bound on ``offset``, (2, 1) float32:

    tiles     chains        trips    float32 per wavefront    float32 throughout    honest model
    1 027        65 669     1        0.0012                   0.10                  0.0012
    2 058       131 653     1        0.0010                   0.29                  0.0010
    4 113       263 173     2        0.0004                   0.30                  0.0004
    8 192       524 229     2        0.0003                   0.33                  0.0003
    16 384    1 048 517     4        0.0004                   0.30                  0.0004
    32 768    2 097 093     8        0.0003                   0.22                  0.0002

("throughout" adds the 4 096 wavefronts' sums one after the other in float32, the least favourable order.)  A trip adds
one float32 rounding to the at most 130 of a tile, so even in the worst case a wavefront needs more than 130 trips -- 34
million chains -- before the bound could be passed, and the measured errors, which average out, are nowhere near.
``wide_integers`` catches both variants at the first second-trip size, on every float32 path that has one."""
import functools

import numpy as np
import pytest

import pooled_moments_reference as ref

SEED = 3
CASES = ref.conformance_cases()
GROUPS = sorted({(path, nr, nc, dtype) for path, nr, nc, dtype, _, _ in CASES})


@functools.lru_cache(maxsize=4)
def _state_and_reference(name, nr, nc, n, dtype):
    x = ref.make_state(name, nr, nc, n, SEED, dtype)
    return (x,) + ref.exact_moments(x, nr, nc)


def _worst(got, s, a, dtype, n):
    return float(ref.error_ratio(got, s, a).max() / ref.bound(dtype, n))


def test_layout_is_the_public_one():
    from metropolisengine_amd import distributed
    for nr, nc in ((1, 0), (0, 1), (2, 7), (64, 0), (60, 25)):
        assert ref.moments_size(nr, nc) == distributed.moments_size(nr, nc)
    x = np.array([[1.0, -2.0, 3.0, 4.0], [-5.0, 6.0, -6.0, 8.0]])        # (2, 1): x0, x1, z = 3 + 4i, -6 + 8i
    s, a = ref.exact_moments(x, 2, 1)
    want = [2, -4, 4, -3, 12, 26, -32, 40, 33, -42, 45, -36, 40, -36, 80, 6, 8, 15, 26, 40, 0, 0]
    assert s.tolist() == want
    assert a.tolist() == [2, 6, 8, 9, 12, 26, 32, 40, 33, 42, 45, 44, 56, 60, 80, 6, 8, 15, 26, 40, 0, 0]
    lay = ref.layout(2, 1)
    assert s[lay["abs_complex"]].tolist() == [15] and s[lay["squares"]].tolist() == [26, 40]
    # the long-double branch agrees with the integer one
    sf, af = ref.exact_moments(x + 0.5, 2, 1)
    assert sf.dtype == ref.LD and float(sf[1]) == -3.0 and float(af[1]) == 6.0
    assert abs(float(sf[lay["abs_complex"]][0]) - (np.hypot(3.5, 4.5) + np.hypot(5.5, 8.5))) < 1e-14


def test_classes_are_what_they_say():
    for dtype in ("f32", "f64"):
        x = ref.make_state("integers", 2, 7, 1029, SEED, dtype)
        assert ref.is_integer_state(x) and np.all(x[:, :2] != 0) and np.max(np.abs(x)) == 8
        z2 = x[:, 2:9] ** 2 + x[:, 9:] ** 2
        assert set(np.unique(z2)) <= {k * k for k in range(1, 11)} and {25.0, 100.0, 1.0} <= set(np.unique(z2))
        for name in ("scaled", "offset"):
            x = ref.make_state(name, 2, 7, 1029, SEED, dtype)
            assert np.array_equal(x, x.astype(ref.NUMPY_DTYPE[dtype]).astype(np.float64))
            assert not ref.is_integer_state(x)
            assert np.all(np.abs(x) > 1e-15) and np.all(np.abs(x) < 1e4)
        assert np.all(x > 0)                                             # offset: one sign per entry
    assert ref.bound("f64", 197) == ref.gamma(199, 2.0 ** -53)
    assert abs(ref.bound("f32", 197) / 2.0 ** -24 - 130) < 0.01
    assert ref.bound("f32", 197, "fp32_mfma") == ref.bound("f32", 197) * ref.MFMA_WIDENING


@pytest.mark.parametrize("path,nr,nc,dtype", GROUPS, ids=["%s-%d-%d-%s" % g for g in GROUPS])
def test_honest_models_are_exact_on_integers_and_well_inside_the_bound(path, nr, nc, dtype):
    """Every case of the GPU module: the float32-tile models in both orders for float32 engines, the all-float64 model for
    float64 engines, at the path's own tile and with the path's own stride between a wavefront's tiles.  Largest fraction of
    the bound over all cases (printed per group and class under -s): float32 tiles sequential 0.050, pairwise 0.020;
    all-float64 0.43 at one chain (a single |z| against 3 u), 0.098 from 63 chains on."""
    tile = ref.path_tile(path, nr, nc, dtype)
    models = ("f64",) if dtype == "f64" else ("f32_sequential", "f32_pairwise")
    worst = {(name, model): 0.0 for name in ("scaled", "offset") for model in models}
    for _, _, _, _, n, name in [c for c in CASES if c[:4] == (path, nr, nc, dtype)]:
        x, s, a = _state_and_reference(name, nr, nc, n, dtype)
        step = ref.tiles_between_trips(path, nr, nc, dtype, n)
        for model in models:
            got = ref.model_moments(x, nr, nc, tile=tile, trip_step=step, **ref.MODELS[model])
            assert got[0] == n and got[-1] == 0 and got[-2] == 0
            if name in ("integers", ref.WIDE):
                assert ref.is_exact(got, s), (model, n, name)
            else:
                frac = _worst(got, s, a, dtype, n)
                worst[name, model] = max(worst[name, model], frac)
                assert frac <= (0.25 if n >= 63 else 0.5), (model, n, name, frac)
    for name in ("scaled", "offset"):
        print("\nPOOLED_MOMENTS_MODEL path=%s dtype=%s nr=%d nc=%d class=%s " % (path, dtype, nr, nc, name) +
              " ".join("%s=%.4f" % (model, worst[name, model]) for model in models) + " of the bound")


# ---------------------------------------------------------------------------------------------------- planted defects
def _caught_by_integers(nr, nc, dtype, n, tile=64, name="integers", **defect):
    x, s, _ = _state_and_reference(name, nr, nc, n, dtype)
    model_dtype = defect.pop("model_dtype", dtype)
    assert ref.is_exact(ref.model_moments(x, nr, nc, model_dtype, tile=defect.get("tile", tile)), s)
    return not ref.is_exact(ref.model_moments(x, nr, nc, model_dtype, **dict(dict(tile=tile), **defect)), s)


SECOND_TRIP_F32 = ref.gram32_second_trip_chains("f32")
SECOND_TRIP_F64 = ref.gram32_second_trip_chains("f64")


@pytest.mark.parametrize("nr,nc,dtype,n,tile", [
    (2, 7, "f32", 63, 64), (2, 7, "f32", 65, 64), (16, 0, "f64", 197, 64), (2, 1, "f32", 64 * 16 + 5, 64),
    (2, 7, "f32", SECOND_TRIP_F32, 64), (16, 0, "f64", SECOND_TRIP_F64, 64), (64, 0, "f32", 31, 64),
    (64, 0, "f64", ref.chains(1027), 64), (97, 0, "f64", ref.chains(850), 64), (316, 0, "f32", 33, 32), (312, 0, "f64", 17, 16)])
def test_a_dropped_last_chain_breaks_integers(nr, nc, dtype, n, tile):
    assert n % tile
    assert _caught_by_integers(nr, nc, dtype, n, tile, drop_last_of_ragged_tile=True)


@pytest.mark.parametrize("path,nr,nc,dtype,n", [
    ("gram32", 2, 7, "f32", SECOND_TRIP_F32), ("gram32", 16, 0, "f32", SECOND_TRIP_F32), ("gram32", 2, 7, "f64", SECOND_TRIP_F64),
    ("gram32", 16, 0, "f64", SECOND_TRIP_F64), ("gram64", 64, 0, "f32", ref.chains(1027)),
    ("gram64", 64, 0, "f64", ref.chains(1027))])
def test_a_stale_prefetch_breaks_integers(path, nr, nc, dtype, n):
    stale = ref.stale_prefetch_tiles(path, dtype, n)
    assert stale is not None and stale[0] < (n + 63) // 64
    assert ref.stale_prefetch_tiles(path, dtype, 64 * stale[0]) is None       # one tile fewer: no second trip
    assert _caught_by_integers(nr, nc, dtype, n, stale_prefetch=stale)


@pytest.mark.parametrize("nr,dtype,n", [(160, "f64", 197), (160, "f64", 33), (316, "f32", 197), (316, "f32", 33)])
def test_a_64_chain_tile_where_32_are_staged_breaks_integers(nr, dtype, n):
    assert ref.generic_tile(nr, 0, dtype) == 32
    kw, _ = ref.DEFECTS["tile64_where_32"]
    assert _caught_by_integers(nr, 0, dtype, n, **kw)


def test_the_tile_rule_selects_every_instantiation():
    dims = ((97, 0, "f64"), (250, 0, "f32"), (157, 0, "f64"), (158, 0, "f64"), (315, 0, "f32"), (316, 0, "f32"), (310, 0, "f64"),
            (311, 0, "f64"), (312, 0, "f64"))
    assert [ref.generic_tile(*c) for c in dims] == [64, 64, 64, 32, 64, 32, 32, 16, 16]
    assert ref.generic_rows(97, 0) == 847 and ref.generic_rows(312, 0) == 84 and ref.generic_rows(2, 7) == 1024


@pytest.mark.parametrize("nr,nc", [(16, 0), (0, 4), (4, 4), (2, 1), (2, 2), (2, 7), (64, 0), (97, 0)])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_layout_defects_break_integers(nr, nc, dtype):
    """A transposed block, the Re / Im rows of another parameter, a missing absolute value, the square of the next
    parameter: each on every set that has the rows in question, at 197 chains."""
    n, d = ref.N_CLASS, nr + 2 * nc
    assert d >= 4 and _caught_by_integers(nr, nc, dtype, n, transposed_block=True)
    if nc >= 2:
        assert _caught_by_integers(nr, nc, dtype, n, wrong_complex_pairing=True)
    if nr:
        assert _caught_by_integers(nr, nc, dtype, n, no_abs=True)
        assert _caught_by_integers(nr, nc, dtype, n, square_of_next_parameter=True)


def test_every_defect_is_accounted_for():
    assert {name for name, (_, by) in ref.DEFECTS.items() if by == "integers"} == {
        "drop_last_of_ragged_tile", "stale_prefetch", "tile64_where_32", "transposed_block", "wrong_complex_pairing", "no_abs",
        "square_of_next_parameter"}
    assert ref.DEFECTS["fp32_across_tiles"][1] == ref.WIDE and ref.DEFECTS["f32_sqrt_of_f32_squares"][1] is None


def test_wide_integers_is_what_it_says():
    for nr, nc in ((2, 7), (16, 0), (64, 0)):
        x = ref.make_state(ref.WIDE, nr, nc, 197, SEED, "f32")
        assert ref.is_integer_state(x) and np.array_equal(x, x.astype(np.float32).astype(np.float64))
        real, cplx = np.abs(x[:, :nr]), np.abs(x[:, nr:])
        assert real.min() >= 363 and real.max() <= 511 and cplx.max(initial=0) <= 408
        assert 64 * 363 ** 2 > 2 ** 23 and 64 * 511 ** 2 < 2 ** 24 and 511 ** 2 * ref.gram32_second_trip_chains("f32") < 2 ** 53
        _, a = ref.exact_moments(x[:64], nr, nc)
        assert a.max() < 2 ** 24 and a[ref.layout(nr, nc)["squares"]].min() > 2 ** 23   # one tile: exact in float32, in any order


FLOAT32_SECOND_TRIPS = [c[:5] for c in CASES if c[5] == ref.WIDE]


@pytest.mark.parametrize("path,nr,nc,dtype,n", FLOAT32_SECOND_TRIPS, ids=["%s-%d-%d-%s-n%d" % c for c in FLOAT32_SECOND_TRIPS])
def test_fp32_across_a_wavefronts_tiles_breaks_wide_integers(path, nr, nc, dtype, n):
    """Every float32 path with a second full tile per wavefront or block: float32 carried from the first tile into the second,
    the wavefronts' sums added in float64 -- and in float32 too -- returns other numbers than S on ``wide_integers``; on
    ``integers``, whose sums stay below 2^24, it does not."""
    assert (path, nr, nc, dtype) in {("gram32", 2, 7, "f32"), ("gram32", 16, 0, "f32"), ("gram64", 64, 0, "f32"), ("generic64", 97, 0, "f32")}
    kw, by = ref.DEFECTS["fp32_across_tiles"]
    step = ref.tiles_between_trips(path, nr, nc, dtype, n)
    assert by == ref.WIDE and (n + 63) // 64 >= step + 2                           # two wavefronts with a second FULL tile
    assert _caught_by_integers(nr, nc, dtype, n, name=ref.WIDE, trip_step=step, **kw)
    assert _caught_by_integers(nr, nc, dtype, n, name=ref.WIDE, trip_step=step, across=np.float32, **kw)
    assert not _caught_by_integers(nr, nc, dtype, n, trip_step=step, **kw)
    # one tile per wavefront: nothing is carried, and nothing is caught
    few = 64 * step
    assert not _caught_by_integers(nr, nc, dtype, few, name=ref.WIDE, trip_step=ref.tiles_between_trips(path, nr, nc, dtype, few), **kw)


def test_fp32_across_tiles_is_caught_by_wide_integers_and_not_by_the_bound():
    """See the module docstring: with the launch geometry of k_pool_gram32 the defect stays far inside the bound on
    ``offset`` at the GPU module's large sizes and at the power-of-two tile counts after them, in both variants, where the
    honest model is; a bound on sums cannot catch it at a chain count a test can afford."""
    nr, nc, dtype = 2, 1, "f32"
    kw, _ = ref.DEFECTS["fp32_across_tiles"]
    sizes = [ref.chains(1027), SECOND_TRIP_F64, SECOND_TRIP_F32] + [ref.chains(1 << k) for k in (13, 14, 15)]
    assert sizes[:3] == [65669, 131653, 263173]
    for n in sizes:
        x = ref.make_state("offset", nr, nc, n, SEED, dtype)
        s, a = ref.exact_moments(x, nr, nc)
        step = ref.tiles_between_trips("gram32", nr, nc, dtype, n)
        honest = _worst(ref.model_moments(x, nr, nc, dtype, trip_step=step), s, a, dtype, n)
        waves = _worst(ref.model_moments(x, nr, nc, dtype, trip_step=step, **kw), s, a, dtype, n)
        every = _worst(ref.model_moments(x, nr, nc, dtype, trip_step=step, across=np.float32, **kw), s, a, dtype, n)
        tiles = (n + 63) // 64
        print("\nfp32 across tiles: tiles=%d chains=%d trips=%d per-wavefront=%.4f throughout=%.4f honest=%.4f of the bound"
              % (tiles, n, -(-tiles // step), waves, every, honest))
        assert honest < 0.5 and waves < 0.5 and every < 0.5
    assert ref.K_TILE * ref.GRAM32_ROWS * ref.GRAM32_WAVES["f32"] * 64 > 34e6      # chains before a wavefront has 130 trips


@pytest.mark.parametrize("nr,nc", [(0, 4), (4, 4), (2, 1), (2, 7)])
def test_a_float32_root_of_float32_squares_is_not_told_apart(nr, nc):
    """|z_c| = sqrtf(re re + im im) errs by at most 3 u per term: inside the numerics class the bound describes and exact on
    Pythagorean pairs.  Recorded so that the conformance module is not taken for a test of it: on the sum |z_c| entries the
    defect reaches 0.007 - 0.026 of the bound over these sets and the two float classes, the honest model 0.003 - 0.026 on
    the same inputs (printed under -s)."""
    kw, by = ref.DEFECTS["f32_sqrt_of_f32_squares"]
    assert by is None and not _caught_by_integers(nr, nc, "f32", ref.N_CLASS, **kw)
    rows = ref.layout(nr, nc)["abs_complex"]
    for name in ("scaled", "offset"):
        x, s, a = _state_and_reference(name, nr, nc, ref.N_CLASS, "f32")
        honest = _worst(ref.model_moments(x, nr, nc, "f32")[rows], s[rows], a[rows], "f32", ref.N_CLASS)
        got = ref.model_moments(x, nr, nc, "f32", **kw)
        defect = _worst(got[rows], s[rows], a[rows], "f32", ref.N_CLASS)
        print("\nf32 sqrt of f32 squares: nr=%d nc=%d class=%s sum |z_c|: defect=%.4f honest=%.4f of the bound"
              % (nr, nc, name, defect, honest))
        assert _worst(got, s, a, "f32", ref.N_CLASS) <= 1.0
