"""tests/draw_reference.py checked on the host: against the oracle's draws, against the host build of me_math64.h, against a
C build of Num<float>::unit, and -- from the reference alone -- the tie caps tests/test_gpu_draw_conformance.py relies on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import draw_reference as dr
from oracle import philox
from test_math64_cpu import _build as build_math64, _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = dr.LD
SEED, OFFSET = 99, (1 << 33) + 17


@pytest.fixture(scope="module")
def stream():
    ids = dr.chain_ids(1 << 14, OFFSET)
    return ids, dr.words(SEED, ids, (1 << 32) + 5, 17)


def test_reference_normals_agree_with_the_oracle(stream):
    ids, w = stream
    g, _ = dr.coordinate_normals(w, 15, "f64")
    g_oracle, u_oracle = philox.step_draws(SEED, ids, (1 << 32) + 5, 15)
    assert np.abs(g - g_oracle.astype(LD)).max() <= 1e-13
    assert np.array_equal(dr.units(w[:, 16], "f64").astype(np.float64), u_oracle)      # the accept word is word W = 16
    # complex coordinates: 1/sqrt 2 on everything behind the real block
    gs, rs = dr.scale_complex(g, g, 5)
    assert np.array_equal(gs[:, :5], g[:, :5]) and np.abs(gs[:, 5:] * np.sqrt(LD(2)) - g[:, 5:]).max() < 1e-18
    # phases: -pi + 2 pi u
    assert np.abs(dr.phases(w[:, 3], "f64").astype(np.float64) - (-np.pi + 2 * np.pi * philox.unit_open(w[:, 3]))).max() < 1e-15


def test_host_math64_is_within_4_ulp_of_the_reference(stream, tmp_path):
    _, w = stream
    lib = build_math64(str(tmp_path), 1)                # the noisy-rsq build: the worse of the two host builds
    wa = np.ascontiguousarray(w[:, 0:16:2].ravel().astype(np.uint32))
    wb = np.ascontiguousarray(w[:, 1:16:2].ravel().astype(np.uint32))
    g0, g1 = np.empty(wa.size), np.empty(wa.size)
    lib.me_math64_normals(_ptr(wa), _ptr(wb), ctypes.c_long(wa.size), _ptr(g0), _ptr(g1))
    r0, r1, _ = dr.normal_pairs(wa, wb, "f64")
    assert dr.ulp_err(g0, r0).max() <= dr.FLOAT64_NORMAL_ULPS
    assert dr.ulp_err(g1, r1).max() <= dr.FLOAT64_NORMAL_ULPS


def test_float32_unit_model_matches_the_c_build(tmp_path):
    out = str(tmp_path / "libunit32.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "unit32_host.cpp"), "-o", out],
                   check=True)
    lib = ctypes.CDLL(out)
    rng = np.random.default_rng(8)
    edge = np.concatenate(([0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1], np.arange((1 << 32) - 129, 1 << 32)))
    w = np.concatenate((edge, rng.integers(0, 1 << 32, size=1_000_000))).astype(np.uint32)
    got = np.empty(w.size, dtype=np.float32)
    lib.me_unit_f32(_ptr(w), ctypes.c_long(w.size), _ptr(got))
    model = dr.unit_f32(w)
    assert model.dtype == np.float32 and np.array_equal(got, model)
    assert model.min() == np.float32(2.0 ** -33) and model.max() == 1.0     # (0, 1]: the float32 unit reaches 1
    assert np.array_equal(dr.units(w, "f32").astype(np.float32), model)


def test_the_bounds_reject_a_reference_with_two_words_swapped(stream):
    """The layout check of the GPU test is sharp: the exact normals of a stream whose words 2 and 3 changed places fail
    the float64 4-ulp bound and the float32 bound on (nearly) every chain, in both coordinates of the pair."""
    _, w = stream
    swapped = w.copy()
    swapped[:, [2, 3]] = w[:, [3, 2]]
    for dtype in ("f64", "f32"):
        g, rad = dr.coordinate_normals(w, 6, dtype)
        bad, _ = dr.coordinate_normals(swapped, 6, dtype)
        got = bad.astype(np.float64 if dtype == "f64" else np.float32)         # what a kernel with that fault would store
        if dtype == "f64":
            ok = dr.ulp_err(got, g) <= dr.FLOAT64_NORMAL_ULPS
        else:
            ok = np.abs(got.astype(LD) - g) <= dr.float32_bound(g, rad, dr.FLOAT32_A, dr.FLOAT32_B)
        assert ok[:, [0, 1, 4, 5]].all()                                       # the untouched pairs still pass
        assert ok[:, 2].mean() < 1e-3 and ok[:, 3].mean() < 1e-3
        # ... and a coordinate does not pass as its neighbouring pair's
        assert (np.abs(got[:, 0].astype(LD) - g[:, 2]) <= 1e-6 * np.abs(g[:, 2])).mean() < 1e-3


def test_fit_float32_bound_covers_its_samples():
    rng = np.random.default_rng(3)
    rad = np.abs(rng.standard_normal(10000)).astype(LD) + LD(0.01)
    t = rng.uniform(-1, 1, 10000).astype(LD)
    ref = rad * t
    got = ref + LD(dr.EPS32) * (LD(1.5) * np.abs(ref) * rng.uniform(-1, 1, 10000) + LD(0.7) * rad * rng.uniform(-1, 1, 10000))
    a, b = dr.fit_float32_bound(got, ref, rad)
    assert np.all(np.abs(got - ref) <= dr.float32_bound(ref, rad, a, b) * (1 + LD(1e-12)))
    assert 0 < b <= 0.7 + 0.15 + 1e-9 and 0 <= a <= 2.3


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", sorted(dr.ACCEPT_SHAPES))
def test_tie_caps_hold_for_the_accept_cases_of_the_gpu_test(shape, dtype):
    """For the very seeds, shapes and temperatures of the GPU accept test: the share of chains the tie band flags is under the
    cap (1e-3 in float32, none in float64), and at T = 1e-3 the reference accepts no uphill proposal at all."""
    nr, nc = shape
    for temp in dr.ACCEPT_TEMPS:
        g, accept, tie, p = dr.accept_case_reference(nr, nc, temp, dtype, (dr.FLOAT32_A, dr.FLOAT32_B))
        assert tie.mean() <= dr.ACCEPT_TIE_CAP[dtype], (temp, int(tie.sum()))
        if np.ndim(temp) == 0 and temp == 1e-3:
            assert not accept.any() and not tie.any()
        else:
            assert 0.005 < accept.mean() < 0.995        # the case decides something: hundreds of chains either way
    # close rungs are told apart: reading a neighbouring rung's constants flips decisions the band does not excuse
    g, accept, tie, p = dr.accept_case_reference(nr, nc, dr.ACCEPT_LADDER, dtype, (dr.FLOAT32_A, dr.FLOAT32_B))
    shifted = dr.chain_temps(np.roll(dr.ACCEPT_LADDER, 1), dr.ACCEPT_CHAINS)
    wd = np.concatenate(dr.ACCEPT_SHAPES[shape] + (dr.ACCEPT_SHAPES[shape][1],)).astype(LD)
    w = dr.words(dr.ACCEPT_SEED, dr.chain_ids(dr.ACCEPT_CHAINS, dr.ACCEPT_OFFSET), 0, philox.n_normal_words(nr + 2 * nc) + 1)
    wrong, _, _ = dr.accept_reference((wd * g * g).sum(axis=1), dr.units(w[:, -1], dtype), shifted, dtype, 0)
    assert ((wrong != accept) & ~tie).sum() >= 3
