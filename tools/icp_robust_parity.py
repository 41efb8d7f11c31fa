#!/usr/bin/env python3
"""The parity and accuracy tables of ICP with a robust loss (K17): one sf_icp_accumulate_robust call against the math.fsum value of the
NumPy statement (tests/icp_robust_numpy.py) at the sizes of tests/test_hip_icp_robust.py, `icp_robust`'s whole runs against the
statement's, and what the losses are for -- the rotation error left on the clutter sets, three modes x five losses x seeds 0 .. 3,
for the statement and for the device.  Needs an MI355X; the measurements are the test files' own functions.

    python tools/icp_robust_parity.py [--out profiles/icp_robust_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gicp_numpy as G  # noqa: E402
import icp_robust_numpy as S  # noqa: E402
import test_hip_icp_robust as H  # noqa: E402
import test_icp_robust_host as HOST  # noqa: E402

MODE_NAMES = {v: k for k, v in S.MODES.items()}
LOSS_NAMES = {v: k for k, v in S.LOSSES.items()}


def device_row(mode_name, seed):
    """|R - R0| of `icp_robust` per loss on clutter_set(seed): 60 annealed iterations from the identity, every point kept"""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_robust

    scan, ref, r0, t0 = S.clutter_set(seed)
    nref = G.knn_normals(ref)
    na = G.knn_normals(scan) if mode_name == "generalized" else None
    row = {}
    for name in S.LOSSES:
        k, k0 = S.table_scales(mode_name, name)
        tf = icp_robust(scan, ref, RigidTransform(), S.D_MAX, mode=mode_name, loss=name, scale=k, scale_start=k0, division_factor=S.FACTOR,
                        ref_normals=nref, scan_normals=na, voxel_size=H.RUN_VOXEL, max_iter=S.ITERATIONS, rms_threshold=0.0,
                        step_tolerance=0.0)[0]
        row[name] = G.rotation_error(tf.rotation, r0)
    return row


def clean_row(seed):
    """the same scan WITHOUT the clutter, point-to-plane without a loss (statement)"""
    scan, ref, r0, t0 = G.corner_set(seed)
    r = S.refine(scan, None, ref, G.knn_normals(ref), S.PLANE, 0, S.D_MAX, S.SCALE, S.D_MAX, S.FACTOR, max_iter=S.ITERATIONS,
                 rms_threshold=0.0, step_tolerance=0.0, how="np")
    return G.rotation_error(r["R"], r0)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_robust_parity.md"))
    a = ap.parse_args()
    from shot_fpfh_amd.engine import default_engine
    from shot_fpfh_amd.icp import _Registration

    eng = default_engine()
    c = H.C_ROUNDINGS
    out = ["# ICP with a robust loss (K17): device against the fsum statement, and what the losses buy", "",
           f"Written by `tools/icp_robust_parity.py` on an MI355X ({eng.lib.sf_version().decode()}) from the measurements of",
           "`tests/test_hip_icp_robust.py` and `tests/test_icp_robust_host.py`.", "",
           "## One pass", "",
           "One `sf_icp_accumulate_robust` call (`k_icp_sums`, `k_icp_means`) against the `math.fsum` value of each of its 48 sums as",
           "`tests/icp_robust_numpy.py` states them; mode 0 is centred on both sides with the weighted centroids the device formed.  An",
           "entry is the worst |sum - fsum| / (k 2^-53 sum|term|) over the 48 slots, the five losses and the three states (identity, true",
           f"motion, 0.3 rad away) at d_max = {H.D_MAX}, scale {H.K_ONE[S.POINT]} (mode 2: {H.K_ONE[S.GICP]}); the pair counts are equal in every case.",
           f"The test's bound is C: {c[S.POINT]} (mode 0), {c[S.PLANE]} (mode 1), {c[S.GICP]} (mode 2), the chain of w r2 counted in the test file.", "",
           "| scan rows | " + " | ".join(f"{MODE_NAMES[m]} (mode {m})" for m in H.MODE_IDS) + " |", "|---|---|---|---|"]
    overall = 0.0
    for m in H.M_SIZES:
        row = [max(H.measure_one_pass(eng, mode, loss, m) for loss in H.LOSS_IDS) for mode in H.MODE_IDS]
        overall = max(overall, max(r / c[mode] for r, mode in zip(row, H.MODE_IDS)))
        out.append(f"| {m} | " + " | ".join(f"{r:.3g}" for r in row) + " |")
        print(out[-1])
    far = H.measure_far(eng)
    out += ["", f"Worst ratio against its bound over the table: {overall:.3g} of 1.", "",
            "Both clouds moved by 1000 on every axis, 5 000 scan rows, mode 0 with Cauchy, with and without a transform; the magnitudes",
            f"are those of the factors centred with the weighted centroids.  Worst ratio: {far:.3g} (bound {c[S.POINT]}).", "",
            "## Whole runs", "",
            f"`icp_robust` from the identity on `clutter_set(0)` (1 875 scan points, d_max = {S.D_MAX}), {H.RUN_ITERATIONS} iterations with",
            "`rms_threshold = 0` and `step_tolerance = 0`, the scale annealed as in the accuracy table: max(|dR|, |dt|) of the device against",
            "the statement's fsum run, and of that run against four runs on row-permuted scans with NumPy's pairwise sums (the",
            "statement's own sensitivity; the test's bound is ten times it).", "",
            "| mode | loss | device vs statement | statement's own | rms (device) | rms (statement) |", "|---|---|---|---|---|---|"]
    calls, real = [], _Registration.pairs
    _Registration.pairs = lambda self, *args, **kw: calls.append(kw.get("scale")) or real(self, *args, **kw)
    try:
        for mode_name in S.MODES:
            for loss_name in H.RUN_LOSSES:
                r = H.measure_whole_run(mode_name, loss_name, calls)
                out.append(f"| {mode_name} | {loss_name} | {r['device_vs_statement']:.3e} | {r['own']:.3e} | {r['rms_device']:.15e} | "
                           f"{r['rms_statement']:.15e} |")
                print(out[-1])
    finally:
        _Registration.pairs = real
    out += ["", "## Accuracy on the clutter sets", "",
            "`clutter_set(seed)`: the corner set of `tests/gicp_numpy.py` (1 500 + 1 500 points, sigma = 0.002, start at the identity, 0.12 rad",
            "off) with 375 points (25 %) added to the scan that the reference does not have, a patch hovering 0.04 above the z = 0 face,",
            f"inside d_max = {S.D_MAX}.  The scale starts at d_max and is divided by {S.FACTOR} per iteration down to {S.SCALE} (3 sigma; Tukey",
            f"{S.SCALE_TUKEY}); mode 2 measures the Mahalanobis distance, so both scales are divided by sqrt(2 epsilon) there.  {S.ITERATIONS}",
            "iterations.  An entry is |R - R0| (Frobenius), statement / device.  The test asserts, for point-to-plane and the statement,",
            f"that Cauchy, Geman-McClure and Tukey each stay at or below {HOST.ACCURACY_CAP} x the loss-none value on every seed; the inputs were",
            "not changed to meet the cap.  Everything else is tabulated, not asserted.  No real scan was measured.", "",
            "| mode | seed | " + " | ".join(S.LOSSES) + " |", "|---|---|" + "---|" * len(S.LOSSES)]
    for mode_name in S.MODES:
        for seed in range(4):
            st, dv = HOST.accuracy_row(mode_name, seed), device_row(mode_name, seed)
            out.append(f"| {mode_name} | {seed} | " + " | ".join(f"{st[n]:.2e} / {dv[n]:.2e}" for n in S.LOSSES) + " |")
            print(out[-1])
    clean = [clean_row(seed) for seed in range(4)]
    out += ["", "The same scans without the clutter, point-to-plane without a loss (statement): " + ", ".join(f"{x:.2e}" for x in clean) + ".", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
