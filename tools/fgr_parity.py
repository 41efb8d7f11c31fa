#!/usr/bin/env python3
"""Parity figures of fast global registration (K12) on one MI355X against the NumPy statement of the definition
(tests/fgr_numpy.py), as markdown tables -- what profiles/fgr_parity.md quotes:
  1. the statement's own sensitivity to the order of its sums (math.fsum against np.sum over a permuted row order) and the
     device's distance from the fsum run, per set;
  2. one pass (sf_fgr_sums) against math.fsum at nine states per set: the worst error in units of k 2^-53 sum|term|;
  3. |R - R0|, |t - t0| of the public call on the six accuracy sets.
Needs an MI355X: without one the engine raises and nothing is printed.

    python tools/fgr_parity.py [--out profiles/fgr_parity_device.md]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fgr_numpy as F  # noqa: E402
import ransac_numpy as N  # noqa: E402

THR = 0.01
SYNTH = [(5000, 0.5), (5000, 0.2), (5000, 0.1), (20000, 0.5), (20000, 0.2), (20000, 0.1)]
ACCURACY_SETS = [(20000, 0.30, 0), (20000, 0.10, 1), (20000, 0.05, 2), (2000, 0.30, 3), (200000, 0.30, 4), (20000, 0.50, 5)]


def matches(name):
    if name == "duplicates":
        sk, rk, si, ri, r0, t0 = N.synthetic_matches(4000, 0.5, seed=11)
        return sk, rk, si, ri[np.random.default_rng(3).integers(0, 40, 4000)], r0, t0
    m, share = name
    return N.synthetic_matches(m, share, seed=m + int(100 * share))


def diff(r1, t1, r2, t2):
    return max(float(np.abs(r1 - r2).max()), float(np.abs(t1 - t2).max()))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None, help="also write the tables here")
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd.matching import fast_global_registration

    eng = s.Engine()
    lines = [f"library {eng.lib.sf_version().decode()}", "",
             "| set | statement: fsum vs permuted np.sum | device vs statement (fsum) | one pass, worst error / (k 2^-53 sum abs term), 9 states |",
             "|---|---|---|---|"]
    worst_own = worst_dev = 0.0
    for name in SYNTH + ["duplicates"]:
        sk, rk, si, ri, r0, t0 = matches(name)
        pa, pb = N.matched_points(si, ri, sk, rk)
        m = pa.shape[0]
        exact = F.fgr_rows(pa, pb, THR)
        other = F.fgr_rows(pa, pb, THR, how="np", order=np.random.default_rng(17).permutation(m))
        own = diff(exact["R"], exact["t"], other["R"], other["t"])
        da, db = eng.empty((m, 3)), eng.empty((m, 3))
        try:
            da.from_host(pa), db.from_host(pb)
            rt = eng.fgr_device(da, db, m, THR)[0]
            ca, cb, sc, x, y = F.normalise(pa, pb)
            t_true = (r0 @ ca + t0 - cb) / sc
            away = F.rodrigues(0.3 * np.array([2.0, -1.0, 2.0]) / 3.0) @ r0
            one_pass = 0.0
            for rot, t in ((np.eye(3), np.zeros(3)), (r0, t_true), (away, t_true)):
                for mu in (1.0, 1e-2, (THR / sc) ** 2):
                    got = eng.fgr_sums(da, db, m, np.concatenate([ca, cb, [sc], rot.reshape(9), t, [mu]]))
                    want = F.sums(x, y, rot, t, mu)
                    ok = want["abs"] > 0
                    one_pass = max(one_pass, float((np.abs(got[:29] - want["vec"])[ok] / (m * 2.0**-53 * want["abs"][ok])).max()))
        finally:
            da.free(), db.free()
        dev = diff(rt[:9].reshape(3, 3), rt[9:], exact["R"], exact["t"])
        worst_own, worst_dev = max(worst_own, own), max(worst_dev, dev)
        lines.append(f"| {name} | {own:.3e} | {dev:.3e} | {one_pass:.3g} |")
    lines += ["", f"largest sensitivity of the statement {worst_own:.3e}; bound of the device 10 x that = {10 * worst_own:.3e}; "
              f"largest device difference {worst_dev:.3e}", "",
              "| set (m, share, seed) | dR | dt | inlier ratio |", "|---|---|---|---|"]
    for case in ACCURACY_SETS:
        sk, rk, si, ri, r0, t0 = N.synthetic_matches(case[0], case[1], seed=case[2])
        ratio, tf, _ = fast_global_registration(si, ri, sk, rk, distance_threshold=THR, engine=eng)
        lines.append(f"| {case} | {np.linalg.norm(tf.rotation - r0):.2e} | {np.linalg.norm(tf.translation - t0):.2e} | {ratio:.4f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
