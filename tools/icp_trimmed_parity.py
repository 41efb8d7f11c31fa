#!/usr/bin/env python3
"""The parity and accuracy tables of trimmed ICP (K18): one sf_icp_accumulate_trimmed call against the NumPy statement
(tests/icp_trimmed_numpy.py) at the sizes of tests/test_hip_icp_trimmed.py, `icp_trimmed`'s whole runs against the statement's, and
what the trimming is for -- the rotation error left on the clutter sets, three modes x overlaps 0.9 / 0.8 / 0.7 / 0.6, annealed and
not, x seeds 0 .. 3, for the statement and for the device, with K17's Cauchy and Geman-McClure rows beside them.  Needs an MI355X;
the measurements are the test files' own functions.

    python tools/icp_trimmed_parity.py [--out profiles/icp_trimmed_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gicp_numpy as G  # noqa: E402
import icp_robust_numpy as S  # noqa: E402
import icp_trimmed_numpy as TR  # noqa: E402
import test_hip_icp_robust as H  # noqa: E402
import test_hip_icp_trimmed as HT  # noqa: E402

MODE_NAMES = {v: k for k, v in S.MODES.items()}
OVERLAPS = (0.9, 0.8, 0.7, 0.6)
COLUMNS = [("no trim", 1.0, 0)] + [(f"{o}, annealed", o, TR.ANNEAL) for o in OVERLAPS] + [(f"{o}, from iteration 0", o, 0) for o in OVERLAPS]
K17 = ("cauchy", "geman_mcclure")


def accuracy_rows(mode_name, seed):
    """(statement, device): |R - R0| per column on clutter_set(seed), 60 iterations from the identity, every point kept; then K17's
    two losses with the table's annealed scales"""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_robust, icp_trimmed

    scan, ref, r0, t0 = S.clutter_set(seed)
    nref = G.knn_normals(ref)
    na = G.knn_normals(scan) if mode_name == "generalized" else None
    common = dict(mode=mode_name, ref_normals=nref, scan_normals=na, voxel_size=H.RUN_VOXEL, max_iter=S.ITERATIONS, rms_threshold=0.0,
                  step_tolerance=0.0)
    st, dv = [], []
    for _label, overlap, anneal in COLUMNS:
        r = TR.refine(scan, na, ref, nref, S.MODES[mode_name], S.D_MAX, overlap, anneal, max_iter=S.ITERATIONS, rms_threshold=0.0,
                      step_tolerance=0.0, how="np")
        st.append(G.rotation_error(r["R"], r0))
        tf = icp_trimmed(scan, ref, RigidTransform(), S.D_MAX, overlap=overlap, anneal_iterations=anneal, **common)[0]
        dv.append(G.rotation_error(tf.rotation, r0))
    for name in K17:
        k, k0 = S.table_scales(mode_name, name)
        r = S.refine(scan, na, ref, nref, S.MODES[mode_name], S.LOSSES[name], S.D_MAX, k, k0, S.FACTOR, max_iter=S.ITERATIONS,
                     rms_threshold=0.0, step_tolerance=0.0, how="np")
        st.append(G.rotation_error(r["R"], r0))
        tf = icp_robust(scan, ref, RigidTransform(), S.D_MAX, loss=name, scale=k, scale_start=k0, division_factor=S.FACTOR, **common)[0]
        dv.append(G.rotation_error(tf.rotation, r0))
    return st, dv


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_trimmed_parity.md"))
    a = ap.parse_args()
    from shot_fpfh_amd.engine import default_engine
    from shot_fpfh_amd.icp import _Registration

    eng = default_engine()
    c = H.C_ROUNDINGS
    out = ["# Trimmed ICP (K18): device against the statement, and what the trimming buys", "",
           f"Written by `tools/icp_trimmed_parity.py` on an MI355X ({eng.lib.sf_version().decode()}) from the measurements of",
           "`tests/test_hip_icp_trimmed.py` and the statement `tests/icp_trimmed_numpy.py`.", "",
           "## One pass", "",
           "One `sf_icp_accumulate_trimmed` call (`k_icp_keys`, the selection of `csrc/select.hip`, `k_icp_sums`, `k_icp_means`) against the",
           "statement: n0, the rank, the cut and the used pair count are EQUAL in every case (asserted), and an entry is the worst",
           "|sum - fsum| / (k 2^-53 sum|term|) over the 48 slots, the trims " + ", ".join(str(t) for t in HT.TRIMS) + ", no loss / Cauchy / Tukey and the",
           f"states of the test (identity, true motion, 0.3 rad away; the true motion alone at 65 537 rows) at d_max = {HT.D_MAX}.",
           f"The bound is K17's C: {c[S.POINT]} (mode 0), {c[S.PLANE]} (mode 1), {c[S.GICP]} (mode 2).", "",
           "| scan rows | " + " | ".join(f"{MODE_NAMES[m]} (mode {m})" for m in H.MODE_IDS) + " |", "|---|---|---|---|"]
    overall = 0.0
    for m in HT.T.M_SIZES:
        row = [max(HT.measure_one_pass(eng, mode, loss, m) for loss in HT.ONE_PASS_LOSSES) for mode in H.MODE_IDS]
        overall = max(overall, max(r / c[mode] for r, mode in zip(row, H.MODE_IDS)))
        out.append(f"| {m} | " + " | ".join(f"{r:.3g}" for r in row) + " |")
        print(out[-1])
    out += ["", f"Worst ratio against its bound over the table: {overall:.3g} of 1.", "",
            "## Whole runs", "",
            f"`icp_trimmed` from the identity on `clutter_set(0)` (1 875 scan points, d_max = {S.D_MAX}), overlap {TR.OVERLAP} annealed over",
            f"{TR.ANNEAL} iterations, {HT.RUN_ITERATIONS} iterations with `rms_threshold = 0` and `step_tolerance = 0`: max(|dR|, |dt|) of the device",
            "against the statement's fsum run, and of that run against four runs on row-permuted scans with NumPy's pairwise sums (the",
            "statement's own sensitivity; the test's bound is ten times it).  (n0, rank, used) of every iteration equal the statement's.", "",
            "| mode | device vs statement | statement's own | rms (device) | rms (statement) | last (n0, rank, used) |", "|---|---|---|---|---|---|"]
    calls, real = [], _Registration.pairs

    def pairs(self, *args, **kw):
        found = real(self, *args, **kw)
        calls.append((kw.get("trim", 1.0), found))
        return found

    _Registration.pairs = pairs
    try:
        for mode_name in S.MODES:
            r = HT.measure_whole_run(mode_name, calls)
            assert r["selections"] == r["want_selections"]
            out.append(f"| {mode_name} | {r['device_vs_statement']:.3e} | {r['own']:.3e} | {r['rms_device']:.15e} | {r['rms_statement']:.15e} | "
                       f"{r['selections'][-1]} |")
            print(out[-1])
    finally:
        _Registration.pairs = real
    out += ["", "## Accuracy on the clutter sets", "",
            "`clutter_set(seed)`: the corner set of `tests/gicp_numpy.py` (1 500 + 1 500 points, sigma = 0.002, start at the identity, 0.12 rad",
            "off) with 375 points added to the scan that the reference does not have (a fifth of the 1 875), a patch hovering 0.04 above the",
            f"z = 0 face, inside d_max = {S.D_MAX}.  {S.ITERATIONS} iterations, no loss.  \"annealed\": the share comes down linearly from 1 over",
            f"{TR.ANNEAL} iterations.  The last two columns are K17's losses with their annealed scales (`profiles/icp_robust_parity.md`).  An",
            "entry is |R - R0| (Frobenius), statement (NumPy's pairwise sums) / device.  tests/test_icp_trimmed_host.py asserts, for",
            "point-to-plane and the statement, that overlap 0.8 annealed leaves less than a fifth of the untrimmed error on every seed and",
            "that overlap 0.8 from iteration 0 is worse than no trimming.  Everything else is tabulated, not asserted.  No real scan was",
            "measured.", "",
            "| mode | seed | " + " | ".join(label for label, _o, _a in COLUMNS) + " | " + " | ".join(K17) + " |",
            "|---|---|" + "---|" * (len(COLUMNS) + len(K17))]
    for mode_name in S.MODES:
        for seed in range(4):
            st, dv = accuracy_rows(mode_name, seed)
            out.append(f"| {mode_name} | {seed} | " + " | ".join(f"{x:.2e} / {y:.2e}" for x, y in zip(st, dv)) + " |")
            print(out[-1])
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
