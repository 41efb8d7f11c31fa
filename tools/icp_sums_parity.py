#!/usr/bin/env python3
"""The parity table of point-to-point and point-to-plane ICP's sums: one sf_icp_accumulate call against the math.fsum value of the
NumPy statement (tests/icp_numpy.py) at the sizes of tests/test_hip_icp_sums.py, and `_refine`'s whole runs against the statement's,
beside the statement's own sensitivity to the order of its sums.  Needs an MI355X; the measurements are the test file's own
functions.

    python tools/icp_sums_parity.py [--out profiles/icp_sums_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import icp_numpy as I  # noqa: E402
import test_hip_icp_sums as T  # noqa: E402

NAMES = {I.POINT: "point-to-point (mode 0)", I.PLANE: "point-to-plane (mode 1)"}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_sums_parity.md"))
    a = ap.parse_args()
    from shot_fpfh_amd.engine import default_engine

    eng = default_engine()
    out = ["# ICP sums (point-to-point, point-to-plane): device against the fsum statement", "",
           f"Written by `tools/icp_sums_parity.py` on an MI355X ({eng.lib.sf_version().decode()}) from the measurements of",
           "`tests/test_hip_icp_sums.py`.  One `sf_icp_accumulate` call (`k_icp_sums<1, 0>`, `k_icp_sums<1, 1>`) is compared with the",
           "`math.fsum` value of each of its sums as `tests/icp_numpy.py` states them; mode 0 is centred on both sides with the",
           "centroids the device formed.  An entry is the worst |sum - fsum| / (k 2^-53 sum|term|) over the 40 slots and the three",
           "states (identity, true motion, 0.3 rad away) at d_max = 0.05; the pair counts are equal in every case.  The test's bound",
           f"is C: {T.C_ROUNDINGS[I.POINT]} for mode 0 (the chain of d2), {T.C_ROUNDINGS[I.PLANE]} for mode 1 (the chain of g_a h), counted in the test file.", "",
           "## One pass", "", "| scan rows | " + " | ".join(NAMES[m] for m in (I.POINT, I.PLANE)) + " |", "|---|---|---|"]
    for m in T.M_SIZES:
        row = [T.measure_one_pass(eng, mode, m) for mode in (I.POINT, I.PLANE)]
        out.append(f"| {m} | " + " | ".join(f"{r:.3g}" for r in row) + " |")
        print(out[-1])
    far = T.measure_far(eng)
    out += ["", "## Far from the origin", "",
            "Both clouds moved by 1000 on every axis, 5 000 scan rows, mode 0, with and without a transform; the magnitudes are those of",
            f"the centred factors |a_i b_j|.  Worst ratio: {far:.3g} (bound {T.C_ROUNDINGS[I.POINT]}).", "",
            "## Whole runs", "",
            "`_refine` from the identity on seed 0 of the corner set of `tests/gicp_numpy.py` (1 500 points, d_max = 0.15), a fixed number",
            "of iterations with `rms_threshold = 0`: max(|dR|, |dt|) of the device against the statement's fsum run, and of that run",
            "against four runs on row-permuted scans with NumPy's pairwise sums (the statement's own sensitivity; the test's bound is",
            "ten times it).  The rms stop is run at the geometric mean of two consecutive residuals of the statement.", "",
            "| mode | iterations | device vs statement | statement's own | rms (device) | rms (statement) | rms stop: threshold | iterations (device / statement) |",
            "|---|---|---|---|---|---|---|---|"]
    for mode in (I.POINT, I.PLANE):
        r = T.measure_whole_run(eng, mode)
        out.append(f"| {NAMES[mode]} | {r['iterations']} | {r['device_vs_statement']:.3e} | {r['own']:.3e} | {r['rms_device']:.15e} | "
                   f"{r['rms_statement']:.15e} | {r['stop_threshold']:.4e} | {r['stop_iterations']} / {r['stop_want']} |")
        print(out[-1])
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
