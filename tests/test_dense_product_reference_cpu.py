"""CPU checks of tests/dense_product_reference.py: the arithmetic model of the split-bf16 kernel and plain fma chains stay
inside the derived bound gamma on every input class, the planted defects of the model do not stay under the calibrated
cap, and the exact cases are exact.  No GPU; run with -s to see the ratios (in units of u)."""
import numpy as np
import pytest

import dense_product_reference as ref

N, SEED = 197, 3
U32, U64 = ref.UNIT_ROUNDOFF["f32"], ref.UNIT_ROUNDOFF["f64"]


def _tiny_noise(x, dtype, seed=1):
    """What one probe step leaves where x was zero: w g with w = 2^-100 (float32) or 2^-200 (float64)."""
    g = np.random.default_rng(seed).standard_normal(x.shape)
    w = 2.0 ** (-100 if dtype == "f32" else -200)
    return np.where(x == 0, np.asarray(w * g, dtype=ref.NUMPY_DTYPE[dtype]).astype(np.float64), x)


def test_split_pieces_are_exact_and_bounded_as_derived():
    rng = np.random.default_rng(0)
    v = np.concatenate((rng.standard_normal(20000) * np.exp(rng.uniform(-20, 20, 20000)),
                        ref._all_ones((1000,), rng, np.float32),
                        # 1.0000000 1111... : the supremum of |v2| / |v| and |v3| / |v|
                        np.float32(1) + np.float32(2.0 ** -7) - np.float32(2.0 ** -23) * rng.integers(1, 3, 100))).astype(np.float32)
    p1, p2, p3 = (p.astype(np.float64) for p in ref.bf16_pieces(v))
    assert np.array_equal(p1 + p2 + p3, v.astype(np.float64))
    assert np.all(np.abs(p2) < 2.0 ** -7 * np.abs(v)) and np.all(np.abs(p3) < 2.0 ** -15 * np.abs(v))
    assert np.max(np.abs(p2 / v)) > 0.98 * 2.0 ** -7        # the bound on the second piece is approached, so 2^-24 was not one
    neglected = np.abs(p2) * np.abs(p3) * 2 + np.abs(p3) * np.abs(p3)
    assert np.all(neglected <= ref.SPLIT_TERM * v.astype(np.float64) ** 2)


@pytest.mark.parametrize("name", ref.CLASSES + ("pow2_scaled",))
def test_models_stay_inside_gamma(name):
    a, x = ref.make_case(name, 64, SEED, "f32", N)
    r = ref.energy_ratio(ref.split_bf16_energy(a, x), a, x)
    r_chain = ref.energy_ratio(ref.fma_chain_energy(a, x, "f32"), a, x)
    print("\nDENSE_PRODUCT_CPU class=%s f32: split model %.2f u, fma chain %.2f u (gamma %.0f / %.0f u)"
          % (name, r / U32, r_chain / U32, ref.gamma("bf16x3", 64, "f32") / U32, ref.gamma("fp32_mfma", 64, "f32") / U32))
    assert r <= ref.gamma("bf16x3", 64, "f32")
    assert r_chain <= ref.gamma("fp32_mfma", 64, "f32")
    for d, family in ((64, "f64_mfma"), (16, "generic"), (97, "runtime")):
        a, x = ref.make_case(name, d, SEED, "f64", N)
        r64 = ref.energy_ratio(ref.fma_chain_energy(a, x, "f64"), a, x)
        print("DENSE_PRODUCT_CPU class=%s f64 D=%d: fma chain %.2f u (gamma %.0f u)" % (name, d, r64 / U64, ref.gamma(family, d, "f64") / U64))
        assert r64 <= ref.gamma(family, d, "f64")
    a, x = ref.make_case(name, 97, SEED, "f32", N)
    assert ref.energy_ratio(ref.fma_chain_energy(a, x, "f32"), a, x) <= ref.gamma("runtime", 97, "f32")


@pytest.mark.parametrize("name", ref.CLASSES)
def test_calibrated_cap_separates_the_model_from_its_mildest_defect(name):
    a, x = ref.make_case(name, 64, SEED, "f32", N)
    cap, r_ref, r_def, mildest = ref.calibrated_cap(a, x)
    print("\nDENSE_PRODUCT_CPU class=%s: r_ref %.2f u, mildest defect (%s) r_def %.1f u, quotient %.1f, cap %.2f u"
          % (name, r_ref / U32, mildest, r_def / U32, r_def / r_ref, cap / U32))
    if name in ("spd", "wide", "ones_mantissa"):
        assert r_def / r_ref >= 16
    if name in ("spd", "ones_mantissa"):
        for defect, kw in ref.DEFECTS.items():
            r = ref.energy_ratio(ref.split_bf16_energy(a, x, **kw), a, x)
            assert r > cap, (defect, r / U32, cap / U32)
    assert r_ref <= cap <= r_def


def test_factor_leg_model_inside_gamma_and_cap_separates():
    a, _ = ref.make_case("spd", 64, SEED, "f32", N)
    l = np.linalg.cholesky(a).astype(np.float32).astype(np.float64)
    g = np.random.default_rng(SEED).standard_normal((N, 64)).astype(np.float32).astype(np.float64)
    cap, r_ref, r_def, mildest = ref.calibrated_cap(l, g, model=ref.split_bf16_product, ratio=ref.matvec_ratio,
                                                    defects=ref.FACTOR_DEFECTS)
    print("\nDENSE_PRODUCT_CPU L g: r_ref %.2f u, mildest defect (%s) r_def %.1f u, quotient %.1f, cap %.2f u"
          % (r_ref / U32, mildest, r_def / U32, r_def / r_ref, cap / U32))
    assert r_ref <= ref.gamma("bf16x3", 64, "f32", "factor")
    assert r_def / r_ref >= 16
    for defect, kw in ref.FACTOR_DEFECTS.items():
        assert ref.matvec_ratio(ref.split_bf16_product(l, g, **kw), l, g) > cap, defect
    assert ref.matvec_ratio(ref.fma_chain_matvec(l, g, "f32"), l, g) <= ref.gamma("fp32_mfma", 64, "f32", "factor")


@pytest.mark.parametrize("sign", [1, -1])
def test_pow2_scaling_commutes_bitwise_without_under_or_overflow(sign):
    a, x = ref.make_case("pow2_scaled", 64, SEED, "f32", N)
    k = sign * ref.POW2_SHIFT["f32"]
    scaled = (a * 2.0 ** k).astype(np.float32)
    assert np.all(np.isfinite(scaled)) and np.array_equal(scaled.astype(np.float64), a * 2.0 ** k)
    # the smallest retained piece product stays a normal float32: nothing underflows on the way
    pieces_a, pieces_x = ref.bf16_pieces(scaled), ref.bf16_pieces(x)
    smallest = min(np.min(np.abs(p[p != 0])) for p in pieces_a) * min(np.min(np.abs(p[p != 0])) for p in pieces_x)
    assert smallest > np.finfo(np.float32).tiny
    e, e_scaled = ref.split_bf16_energy(a, x), ref.split_bf16_energy(scaled, x)
    assert np.all(np.isfinite(e_scaled)) and np.array_equal(e_scaled.astype(np.float64), e.astype(np.float64) * 2.0 ** k)
    a, x = ref.make_case("pow2_scaled", 64, SEED, "f64", N)
    k = sign * ref.POW2_SHIFT["f64"]
    e, e_scaled = ref.fma_chain_energy(a, x, "f64"), ref.fma_chain_energy(a * 2.0 ** k, x, "f64")
    assert np.all(np.isfinite(e_scaled)) and np.array_equal(e_scaled, e * 2.0 ** k)
    assert np.min(np.abs(a[a != 0])) * 2.0 ** k * np.min(np.abs(x)) ** 2 > 1e-250


def test_exact_two_hot_split_model_is_integer_arithmetic_and_every_defect_breaks_it():
    a, x, code = ref.two_hot_case(64, SEED, split=True)
    assert x.shape[0] == 2080
    want, unfused, tie = ref.two_hot_expected(64, code, split=True)
    assert not tie
    # fusing the last multiply-add or not moves E by an ulp at most; the smallest retained product is 2^-16 of a term
    assert np.all(np.abs(unfused - want) <= 2.0 ** -23 * want) and np.any(unfused != want)
    for defect, kw in ref.EXACT_DEFECTS.items():
        got = ref.split_bf16_energy(a, x, **kw).astype(np.float64)
        assert np.any((got != want) & (got != unfused)), defect
    assert np.array_equal(want, want.astype(np.float32).astype(np.float64)) and np.all(want > 0)
    # all three pieces of both operands are non-zero
    assert all(np.all(p[x != 0] != 0) for p in ref.bf16_pieces(x)) and all(np.all(p != 0) for p in ref.bf16_pieces(a))
    assert np.array_equal(ref.split_bf16_energy(a, x).astype(np.float64), want)
    noisy = _tiny_noise(x, "f32")          # the 1e-30 that a probe step leaves in the zero components is absorbed
    assert np.all(noisy != 0)
    assert np.array_equal(ref.split_bf16_energy(a, noisy).astype(np.float64), want)
    for defect, kw in ref.EXACT_DEFECTS.items():
        assert not np.array_equal(ref.split_bf16_energy(a, noisy, **kw).astype(np.float64), want), defect


@pytest.mark.parametrize("d,dtype", [(16, "f32"), (16, "f64"), (64, "f32"), (64, "f64"), (97, "f32"), (97, "f64")])
def test_exact_two_hot_small_integers(d, dtype):
    a, x, code = ref.two_hot_case(d, SEED, split=False)
    assert x.shape[0] == d * (d + 1) // 2
    want, _, _ = ref.two_hot_expected(d, code, split=False)
    assert np.all(want > 0) and np.array_equal(want, np.asarray(ref.quadratic_form_ld(a, x), dtype=np.float64))
    assert np.array_equal(ref.fma_chain_energy(a, _tiny_noise(x, dtype), dtype).astype(np.float64), want)
