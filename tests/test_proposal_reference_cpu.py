"""tests/proposal_reference.py checked against itself, no GPU: a numpy model of honest device code (float32 with the fused
multiply-add as a float64 product-sum rounded once, float64 through long double) is exact on the exact classes and stays
within every derived bound; every planted defect breaks an exact class AND exceeds the bound on a float class; on every
shape the device test uses, each packed slot is the live one of some chain of the one_per_row class.  Run with -s for the
fractions of the bounds that honest code reaches and the defects' excesses ("Proposal conformance")."""
import numpy as np
import pytest

import proposal_reference as pr

DTYPES = ("f32", "f64")
W0 = 2.0 ** -4
# (nr, nc) -> spelling: small shapes that reach every branch of a spelling (a chunk edge, nr mod 4 = 1 with a row tail, the
# 8-row complex batch with a tail, a Philox block that straddles the end of the real parameters)
MODEL_SHAPES = [((4, 4), "registers"), ((2, 7), "registers"), ((0, 12), "registers"), ((17, 0), "registers"),
                ((13, 0), "runtime"), ((9, 3), "runtime"), ((5, 12), "runtime"), ((0, 13), "runtime")]
# the shapes and chain counts of tests/test_gpu_proposal_conformance.py
DEVICE_SHAPES = [(4, 4), (2, 7), (0, 12), (13, 0), (16, 0), (17, 0), (14, 0), (24, 0), (33, 0), (64, 0), (1, 13), (0, 13), (20, 6),
                 (129, 0), (130, 0), (125, 4), (100, 12), (140, 0)]


def device_chains(nr, nc):
    return 3 * 64 + 7 if nr + 2 * nc > 135 else 2 * 64 + 7


def n_for(nr, nc):
    return max(nr, 2 * nc - 1) + 5


def normals(n, nr, nc, dtype, seed=5):
    return pr.to_dtype(np.random.default_rng([seed, nr, nc]).standard_normal((n, nr + 2 * nc)), dtype)


def float_inputs(name, n, nr, nc, dtype, g):
    gr, zre, zim = pr.split_normals(g, nr, nc, dtype)
    if name == "scaled":
        return pr.scaled_case(n, nr, nc, dtype, seed=11)
    return pr.cancelling_case(n, nr, nc, dtype, 12, gr, zre, zim)


def float_ratio(spelling, name, nr, nc, dtype, defect=None, group="all"):
    n = n_for(nr, nc)
    g = normals(n, nr, nc, dtype)
    gr, zre, zim = pr.split_normals(g, nr, nc, dtype)
    x, width, rows = float_inputs(name, n, nr, nc, dtype, g)
    w_r, w_c = pr.widths_used(width, nr, nc)
    got = pr.model_proposal(spelling, x, w_r, w_c, rows, g, nr, nc, dtype, group, defect)
    s, a = pr.proposal_reference(x, w_r, w_c, rows, gr, zre, zim, nr, nc, group)
    return pr.ratio(got, s, a, pr.k_proposal(spelling, nr, nc), dtype)


def one_per_row_equal(spelling, nr, nc, dtype, defect=None, group="all"):
    """Whether the model returns the expected values of the exact class, coordinate by coordinate."""
    n = n_for(nr, nc)
    g = normals(n, nr, nc, dtype)
    gr, zre, zim = pr.split_normals(g, nr, nc, dtype)
    ident = W0 * np.concatenate((gr, zre, zim), axis=1)          # what the identity-shape engine holds
    rows = pr.one_per_row(n, nr, nc)
    w = np.full(n, W0)
    w_r = 2 * w if defect == "real_width_on_complex" else w      # (the device test loads another width per group row as well)
    x = np.zeros((n, nr + 2 * nc))
    got = pr.model_proposal(spelling, x, w_r, w, rows, g, nr, nc, dtype, group, defect)
    want = pr.one_per_row_expected(rows, ident, nr, nc, group)
    if defect == "real_width_on_complex":
        want[:, :nr] *= 2
    return got == want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,spelling", MODEL_SHAPES)
def test_honest_model_is_exact_and_within_every_bound(shape, spelling, dtype):
    nr, nc = shape
    for group in ("all",) + (("real", "complex") if nr and nc else ()):
        assert one_per_row_equal(spelling, nr, nc, dtype, group=group).all()
        for name in ("scaled", "cancelling"):
            r = float_ratio(spelling, name, nr, nc, dtype, group=group)
            print("PROPOSAL_MODEL spelling=%s (%d,%d) %s %s group=%s: real %.3f Hermitian %.3f of the bound"
                  % (spelling, nr, nc, dtype, name, group, r[:, :nr].max(initial=0), r[:, nr:].max(initial=0)))
            assert r.max() < 1
            if group == "all":
                assert r.max() > 0.01               # the bound is not slack by orders of magnitude either


def test_the_classes_are_what_they_claim():
    nr, nc, n = 4, 4, 41
    assert pr.INV_SQRT2["f32"] != pr.INV_SQRT2["f64"] and abs(pr.INV_SQRT2["f64"] ** 2 - 0.5) < 1e-15
    rows = pr.one_per_row(n, nr, nc)
    lr, lre, lim = pr.unpack(rows, nr, nc)
    assert np.all((lr != 0).sum(axis=2) == 1)                                          # one live entry per real row
    assert np.all((lre != 0).sum(axis=2) + (lim != 0).sum(axis=2) == 1)                # ... and per Hermitian row
    assert np.all(np.abs(np.log2(np.abs(rows[rows != 0]))) <= 4) and (rows < 0).any() and (rows > 0).any()
    assert np.all(np.log2(np.abs(rows[rows != 0])) % 1 == 0)
    k = np.arange(5000)
    assert np.all(pr.slot_code(k) != pr.slot_code(k + 1))                              # consecutive slots differ
    for dtype in DTYPES:
        t = pr.NUMPY_DTYPE[dtype]
        g = normals(n, nr, nc, dtype)
        gr, zre, zim = pr.split_normals(g, nr, nc, dtype)
        for name in ("scaled", "cancelling"):
            x, width, rows = float_inputs(name, n, nr, nc, dtype, g)
            for v in (x, width, rows, zre, zim):
                assert np.array_equal(v.astype(t).astype(np.float64), v), name
            assert width.shape == (n, 3) and np.all(width[:, 1] != width[:, 2])
            assert len(np.unique(rows, axis=0)) == n
            s, a = pr.proposal_reference(x, *pr.widths_used(width, nr, nc), rows, gr, zre, zim, nr, nc)
            if name == "cancelling":
                assert np.all(np.abs(s) <= 4 * pr.UNIT_ROUNDOFF[dtype] * a)            # |S| << A in every row
            else:
                assert np.log10(width.max() / width.min()) > 4
    x, width, rows, g = pr.integers_case(n, nr, nc, seed=3)
    for v in (x, rows, g):
        assert np.all(v == np.rint(v)) and np.abs(v).max() < 2 ** 10
    assert np.all(np.log2(width) % 1 == 0) and np.all(width[:, 1] != width[:, 2])


@pytest.mark.parametrize("shape", [(4, 4), (2, 7)])
def test_integer_class_is_exact_in_the_real_rows(shape):
    nr, nc = shape
    n = 41
    x, width, rows, g = pr.integers_case(n, nr, nc, seed=3)
    w_r, w_c = pr.widths_used(width, nr, nc)
    zre, zim = (g[:, nr:nr + nc].astype(pr.LD) * pr.LD(pr.INV_SQRT2["f64"]), g[:, nr + nc:].astype(pr.LD) * pr.LD(pr.INV_SQRT2["f64"]))
    s, a = pr.proposal_reference(x, w_r, w_c, rows, g[:, :nr], zre, zim, nr, nc)
    got = pr.model_proposal("registers", x, w_r, w_c, rows, g, nr, nc, "f64")
    assert np.array_equal(got[:, :nr].astype(pr.LD), s[:, :nr]) and np.any(s[:, :nr] != x[:, :nr])
    assert pr.ratio(got, s, a, pr.k_proposal("registers", nr, nc, raw_normals=True), "f64").max() < 1
    if nr > 2:                                    # (tri(0, 1) IS tri(1, 0): two real rows have nothing to transpose)
        broken = pr.model_proposal("registers", x, w_r, w_c, rows, g, nr, nc, "f64", defect="transposed_real_slot")
        assert not np.array_equal(broken[:, :nr].astype(pr.LD), s[:, :nr])


# defect -> the shapes at which it can show at all (with the spelling it is planted in)
MIXED = [(4, 4), (2, 7)]
CAUGHT_AT = {
    "transposed_real_slot": [(4, 4), (17, 0)],
    "chunk_parity": [(17, 0), (2, 7)],                   # more packed entries than one chunk holds
    "re_im_swapped": MIXED + [(0, 12)],
    "conj_l": MIXED + [(0, 12)],
    "no_sqrt2_on_diagonal": MIXED + [(0, 12)],
    "real_width_on_complex": MIXED,
    "neighbour_chain_row": MIXED + [(17, 0), (0, 12)],
    "im_part_sign": [(9, 3), (5, 12), (0, 13)],
    "real_tail_drops_last_row": [(13, 0), (9, 3), (5, 12)],          # nr mod 4 = 1 and a row below the diagonal triangle
    "complex_batch_starts_late": [(5, 12), (0, 13)],                 # nc >= 9: a whole 8-row batch below the diagonal
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", pr.PROPOSAL_DEFECTS)
def test_every_planted_defect_is_caught(defect, dtype):
    assert set(CAUGHT_AT) == set(pr.PROPOSAL_DEFECTS)
    spelling = pr.PROPOSAL_DEFECTS[defect]
    for nr, nc in CAUGHT_AT[defect]:
        same = one_per_row_equal(spelling, nr, nc, dtype, defect)
        worst = max(float(float_ratio(spelling, name, nr, nc, dtype, defect).max()) for name in ("scaled", "cancelling"))
        print("PROPOSAL_DEFECT %s (%d,%d) %s: one_per_row differs in %d of %d values, largest float-class ratio %.3g"
              % (defect, nr, nc, dtype, int((~same).sum()), same.size, worst))
        assert not same.all()
        assert worst > 1


@pytest.mark.parametrize("nr,nc", DEVICE_SHAPES)
def test_one_per_row_reaches_every_slot_on_the_device_shapes(nr, nc):
    n = device_chains(nr, nc)
    need = max(nr, 2 * nc - 1)      # row i of the Hermitian block: the Im slot of column i - 1 is live in chain (i - 1) + (i + 1)
    assert n >= need
    assert pr.one_per_row_coverage(n, nr, nc).all() and pr.one_per_row_coverage(need, nr, nc).all()
    assert not pr.one_per_row_coverage(need - 1, nr, nc).all()                          # (and needs that many chains)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nr,nc", [(0, 3), (2, 2)])
def test_honest_magnitude_stage_is_within_its_bound(nr, nc, dtype):
    n = 61
    rng = np.random.default_rng([7, nr, nc])
    x = rng.standard_normal((n, nr + 2 * nc))
    x[::7, nr], x[::7, nr + nc] = 0.0, 0.0                          # |z_0| = 0: the direction (1, 0)
    x, w, kdiag, g = (pr.to_dtype(v, dtype) for v in (x, 2.0 ** rng.uniform(-2, 0, n), rng.uniform(0.5, 2, (n, nc)), rng.standard_normal((n, nc))))
    s, a, direction = pr.magphase_reference(x, w, kdiag, g, nr, nc)
    got = pr.model_magphase(x, w, kdiag, g, nr, nc, dtype)
    r = pr.ratio(got, np.tile(s, 2) * direction, np.tile(a, 2) * np.abs(direction), pr.K_MAGPHASE, dtype)
    print("MAGPHASE_MODEL (%d,%d) %s: %.3f of the bound" % (nr, nc, dtype, r.max()))
    assert 0.01 < r.max() < 1
    assert np.array_equal(got[::7, nc], np.zeros(len(got[::7]))) and np.all(got[::7, 0] != 0)
    wrong_row = pr.model_magphase(x, w, np.roll(kdiag, 1, axis=1), g, nr, nc, dtype)        # K of the neighbouring parameter
    assert pr.ratio(wrong_row, np.tile(s, 2) * direction, np.tile(a, 2) * np.abs(direction), pr.K_MAGPHASE, dtype).max() > 1


# ------------------------------------------------------------------------------------------------------ energies
ENERGY_CASES = [("iso", (16, 0), False), ("iso", (3, 0), False), ("iso", (2, 1), False), ("diag", (4, 4), False),
                ("diag", (33, 0), False), ("diag", (3, 0), False), ("iso", (101, 0), True), ("diag", (60, 25), True),
                ("landau", (2, 1), False), ("landau_terms", (2, 1), False), ("cylinder", (1, 3), False), ("cylinder", (2, 2), False)]


def energy_classes(kind):
    return pr.ENERGY_CLASSES if kind in ("landau", "landau_terms") else pr.ENERGY_CLASSES[:2]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,shape,runtime", ENERGY_CASES)
def test_honest_energy_model_is_exact_and_within_every_bound(kind, shape, runtime, dtype):
    nr, nc = shape
    n = 61
    for name in energy_classes(kind):
        x, cf = pr.energy_case(kind, name, n, nr, nc, dtype, seed=21)
        s, a = pr.energy_reference(kind, x, nr, nc, cf)
        got = pr.model_energy(kind, x, nr, nc, cf, dtype, runtime)
        if name == "integers":
            assert np.abs(a).max() < 2 ** 23 and np.all(2 * s == np.rint(2 * s))         # (the cylinder's tot^2 / 2: halves)
            assert np.array_equal(got.astype(pr.LD), s)
        else:
            r = pr.ratio(got, s, a, pr.k_energy(kind, nr, nc, runtime), dtype)
            print("ENERGY_MODEL %s (%d,%d) %s %s%s: %.3f of the bound" % (kind, nr, nc, dtype, name, " runtime" if runtime else "", r.max()))
            assert r.max() < 1
        if name == "cancelling":
            assert np.median((np.abs(s) / a).reshape(n, -1)[:, 0]) < 0.5                  # (row "field" of the term form)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("defect", pr.ENERGY_DEFECTS)
def test_every_planted_energy_defect_is_caught(defect, dtype):
    shapes = {"iso": (3, 0), "diag": (3, 0), "landau": (2, 1), "landau_terms": (2, 1)}
    for kind in pr.ENERGY_DEFECTS[defect]:
        nr, nc = shapes[kind]
        x, cf = pr.energy_case(kind, "integers", 61, nr, nc, dtype, seed=21)
        s, _ = pr.energy_reference(kind, x, nr, nc, cf)
        assert not np.array_equal(pr.model_energy(kind, x, nr, nc, cf, dtype, defect=defect).astype(pr.LD), s)
        x, cf = pr.energy_case(kind, "scaled", 61, nr, nc, dtype, seed=21)
        s, a = pr.energy_reference(kind, x, nr, nc, cf)
        worst = float(pr.ratio(pr.model_energy(kind, x, nr, nc, cf, dtype, defect=defect), s, a, pr.k_energy(kind, nr, nc), dtype).max())
        print("ENERGY_DEFECT %s %s %s: largest ratio %.3g" % (defect, kind, dtype, worst))
        assert worst > 1


def test_the_cylinder_factor_is_the_denominators_conditioning():
    x0 = pr.CYLINDER_X0_MAX
    assert x0 * x0 / (1 - x0 * x0) <= pr.CYLINDER_DENOMINATOR_FACTOR + 1e-12 < 4.27
    assert pr.k_energy("cylinder", 1, 3) == 14 and pr.k_energy("cylinder", 2, 2) == 13
