"""tests/measure_reference.py checked against itself, no GPU: a numpy model of honest device code (float32 with the fused
multiply-add as a float64 product-sum rounded once, float64 through long double) stays within every derived bound and is
exact on both integer classes; every planted defect breaks exactness or exceeds the bound -- the table below says which."""
import numpy as np
import pytest

import cholesky_reference as cr
import measure_reference as mr

N = 41
SHAPES = [(1, 0), (4, 4), (2, 7), (0, 13), (20, 6), (33, 0)]
DTYPES = ("f32", "f64")
QUANTITIES = ("mean", "obs_mean", "cov")


def float_cases():
    return [(name, count) for name in ("scaled", "offset") for count in mr.SCALED_COUNTS]


def worst_ratios(got, ref, dtype):
    return {q: float(mr.ratio(got[q], ref[q][0], ref[q][1], mr.K[q], dtype).max()) for q in QUANTITIES}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nr,nc", SHAPES)
def test_honest_model_stays_within_every_bound(nr, nc, dtype):
    worst = dict.fromkeys(QUANTITIES, 0.0)
    cases = float_cases() + [(name, None) for name in mr.EXACT_COUNT]
    for index, (name, count) in enumerate(cases):
        inp = mr.make_inputs(name, N, nr, nc, dtype, count, seed=10 + index)
        r = worst_ratios(mr.model(inp, dtype), mr.reference(inp), dtype)
        assert all(v <= 1 for v in r.values()), (name, count, r)
        worst = {q: max(worst[q], r[q]) for q in QUANTITIES}
    print("(%d,%d) %s honest model, largest ratios: " % (nr, nc, dtype) + ", ".join("%s %.3f" % kv for kv in worst.items()))
    # the bounds are not slack by orders of magnitude either: honest code uses a fair share of them
    assert worst["mean"] > 0.1 and worst["cov"] > 0.1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nr,nc", SHAPES)
def test_integer_classes_are_exact_in_the_model(nr, nc, dtype):
    inp = mr.make_inputs("integers_rank_one", N, nr, nc, dtype, seed=3)
    got, ref = mr.model(inp, dtype), mr.reference(inp)
    for q in QUANTITIES:
        s = ref[q][0]
        assert np.all(s == np.rint(s)) and np.abs(s).max() < 2 ** 24, q
        assert mr.exact(got[q], s).all(), q
    assert np.count_nonzero(ref["cov"][0]) > 0.5 * ref["cov"][0].size or nr + nc == 1
    inp = mr.make_inputs("integers_keep", N, nr, nc, dtype, seed=4)
    got = mr.model(inp, dtype)
    assert np.array_equal(got["cov"] * 64, inp["cov"] * 63) and np.all(inp["cov"] != 0)
    assert mr.exact(got["cov"], mr.reference(inp)["cov"][0]).all()
    _, _, bad = cr.reference_factor(*mr.unpack_blocks(inp["cov"], nr, nc))
    assert not bad.any()


def test_the_classes_are_what_they_claim():
    nr, nc = 4, 4
    for dtype in DTYPES:
        t = cr.NUMPY_DTYPE[dtype]
        for name, count in float_cases() + [(name, None) for name in mr.EXACT_COUNT]:
            inp = mr.make_inputs(name, N, nr, nc, dtype, count, seed=1)
            for key in ("x", "mean", "obs_mean", "cov", "width"):
                assert np.array_equal(inp[key].astype(t).astype(np.float64), inp[key]), (name, key)     # dtype numbers
            assert inp["width"].shape == (N, 3) and inp["cov"].shape == (N, cr.packed_size(nr, nc))
            assert len(np.unique(inp["x"], axis=0)) == N                                               # another value per chain
    off = mr.make_inputs("offset", N, nr, nc, "f32", 52, seed=1)
    assert np.all(np.abs(off["mean"]) > 100 * np.abs(off["x"] - off["mean"]).max(axis=0))
    rank = mr.make_inputs("integers_rank_one", N, nr, nc, "f32", seed=1)
    assert np.all(rank["width"][:, 1] != rank["width"][:, 2]) and np.all(rank["width"] % 8 == 0)
    assert mr.width_rows_used(4, 4) == (1, 2) and mr.width_rows_used(4, 0) == (0, 0) and mr.width_rows_used(4, 4, split=False) == (0, 0)


# defect -> how it is caught: "exact" = an integer class no longer comes back bit for bit; "bound" = the covariance ratio of a
# float class exceeds 1.  (shapes: where the defect can show at all)
MIXED = [(4, 4), (2, 7), (20, 6)]
COMPLEX = MIXED + [(0, 13)]
CAUGHT_BY = {
    "delta_from_new_mean": ({"exact", "bound"}, SHAPES),
    "two_pass": ({"exact", "bound"}, SHAPES),
    "im_sign": ({"exact", "bound"}, COMPLEX),
    "re_im_swapped": ({"exact", "bound"}, COMPLEX),
    "real_width_on_hermitian": ({"exact", "bound"}, MIXED),
    "no_epsilon": ({"exact", "bound"}, SHAPES),
    "neighbour_chain_delta": ({"exact", "bound"}, SHAPES),
    "slot_shifted_at_batch": ({"exact", "bound"}, [(33, 0), (20, 6), (0, 13)]),
    "mean_keep_for_cov_keep": ({"exact", "bound"}, SHAPES),
}


def defect_findings(defect, nr, nc, dtype):
    """(an integer class is no longer exact, the largest covariance ratio over the float classes)."""
    broken = False
    for name in mr.EXACT_COUNT:
        inp = mr.make_inputs(name, N, nr, nc, dtype, seed=3)
        broken |= not mr.exact(mr.model(inp, dtype, defect)["cov"], mr.reference(inp)["cov"][0]).all()
    worst = 0.0
    for index, (name, count) in enumerate(float_cases()):
        inp = mr.make_inputs(name, N, nr, nc, dtype, count, seed=10 + index)
        s, a = mr.reference(inp)["cov"]
        worst = max(worst, float(mr.ratio(mr.model(inp, dtype, defect)["cov"], s, a, mr.K_COV, dtype).max()))
    return broken, worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", mr.DEFECTS)
def test_every_planted_defect_is_caught(defect, dtype):
    assert set(CAUGHT_BY) == set(mr.DEFECTS)
    how, shapes = CAUGHT_BY[defect]
    for nr, nc in shapes:
        broken, worst = defect_findings(defect, nr, nc, dtype)
        print("%s (%d,%d) %s: exactness %s, largest covariance ratio %.3g" % (defect, nr, nc, dtype, "BROKEN" if broken else "kept", worst))
        assert broken or worst > 1
        if "exact" in how:
            assert broken
        if "bound" in how:
            assert worst > 1
