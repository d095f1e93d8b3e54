#!/usr/bin/env python
"""Measure the constants of tests/draw_reference.py on the device (needs a GPU):

    python tools/measure_draw_conformance.py [--out FILE]

float32 normals: (A, B) of |g - g_ref| <= A eps32 |g_ref| + B eps32 r_ref by draw_reference.fit_float32_bound over 2^22
word pairs (16 real parameters, 2^18 chains, two seeds the committed test does not use), the worst relative error of the
radius hypot(g0, g1) where u1 > 1 - 2^-12, the worst magnitude-phase angle error (float32 in revolutions, float64 in
radians) and the worst float64 normal in ulp.  The committed constants are TWICE what this prints ("Draw
conformance").  One JSON object on stdout.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import draw_reference as dr                      # noqa: E402
import test_gpu_draw_conformance as t            # noqa: E402
import metropolisengine_amd as me                # noqa: E402
from metropolisengine_amd import _capi           # noqa: E402

SEEDS = (7001, 7002)
N = 1 << 18
LD = dr.LD


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    cli = ap.parse_args()
    assert t.SEED not in SEEDS and dr.ACCEPT_SEED not in SEEDS
    got32, ref32, rad32, ulp_real, ulp_cplx, tail = [], [], [], 0.0, 0.0, 0.0
    ph32, ph64, n_tail = 0.0, 0.0, 0
    radius_all, worst = (0.0, 0.0), (0.0, 0.0, 0.0, 0.0)
    for seed in SEEDS:
        ids = dr.chain_ids(N, t.OFFSET)
        w = dr.words(seed, ids, 0, 20)
        for dtype in ("f32", "f64"):
            eng = t.fresh_engine(me.IsoQuadratic(0.0), 16, 0, dtype, 0, seed=seed, n=N, temp=1.0, cov_mode="fixed")
            eng.step_all(1)
            x = eng._get(_capi.FIELD_PARAMS)
            g, rad = dr.coordinate_normals(w, 16, dtype)
            if dtype == "f32":
                got32.append(x.ravel()), ref32.append(g.ravel()), rad32.append(rad.ravel())
                # the radius where u1 is within 2^-12 of 1 (v_log_f32 beside its zero), seen through hypot(g0, g1)
                u1 = dr.units(w[:, 0:16:2], "f32")
                sel = (u1 > 1 - LD(2.0 ** -12)) & (rad[:, 0::2] > 0)
                r_dev = np.hypot(x[:, 0::2].astype(LD), x[:, 1::2].astype(LD))
                live = rad[:, 0::2] > 0
                rel = np.where(live, np.abs(r_dev - rad[:, 0::2]) / np.where(live, rad[:, 0::2], 1), 0)
                if float(rel.max()) > radius_all[0]:
                    radius_all = (float(rel.max()), float(u1.ravel()[rel.argmax()]))
                # the worst normal in units of eps32 r, and the (u1, u2) it belongs to
                e = np.where(rad > 0, np.abs(x.astype(LD) - g) / np.where(rad > 0, LD(dr.EPS32) * rad, 1), 0)
                if float(e.max()) > worst[0]:
                    c, j = np.unravel_index(e.argmax(), e.shape)
                    worst = (float(e.max()), float(u1[c, j // 2]), float(dr.units(w[c, 2 * (j // 2) + 1], "f32")),
                             float(abs(g[c, j]) / rad[c, j]))
                if sel.any():
                    tail = max(tail, float((np.abs(r_dev - rad[:, 0::2])[sel] / rad[:, 0::2][sel]).max()))
                    n_tail += int(sel.sum())
            else:
                ulp_real = max(ulp_real, float(dr.ulp_err(x, g).max()))
                eng = t.fresh_engine(me.IsoQuadratic(0.0), 4, 4, dtype, 0, seed=seed, n=N, temp=1.0, cov_mode="fixed")
                eng.step_all(1)
                x = eng._get(_capi.FIELD_PARAMS)
                gs, _ = dr.scale_complex(*dr.coordinate_normals(w, 12, dtype), 4)
                ulp_cplx = max(ulp_cplx, float(dr.ulp_err(x[:, 4:], gs[:, 4:]).max()))
            x = t.one_magphase_step(0, 3, dtype, 0, seed=seed, n=N)
            z = x[:, :3] + 1j * x[:, 3:]
            _, _, first_phase, _, _ = dr.magphase_words(3)
            err = float(np.abs(t.phase_errors(z, dr.phases(w[:, first_phase:first_phase + 3], dtype))).max())
            if dtype == "f32":
                ph32 = max(ph32, err / (2 * np.pi))
            else:
                ph64 = max(ph64, err)
    a, b = dr.fit_float32_bound(np.concatenate(got32), np.concatenate(ref32), np.concatenate(rad32))
    out = {"float32_word_pairs": int(sum(v.size for v in got32) // 2), "float32_A": a, "float32_B": b,
           "float32_radius_rel_err_u1_near_1": tail, "float32_radius_rel_err_u1_near_1_in_eps32": tail / dr.EPS32,
           "float32_pairs_u1_near_1": n_tail, "float32_radius_rel_err_worst_in_eps32": radius_all[0] / dr.EPS32,
           "float32_radius_rel_err_worst_u1": radius_all[1], "float32_worst_error_in_eps32_r": worst[0],
           "float32_worst_error_u1_u2_t": worst[1:], "float32_phase_rev": ph32, "float64_phase_rad": ph64,
           "float64_normal_ulp_real": ulp_real, "float64_normal_ulp_complex": ulp_cplx}
    text = json.dumps(out)
    print(text)
    if cli.out:
        with open(cli.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
