#!/usr/bin/env python3
"""Writes profiles/outliers_parity.md: what the outlier filters (K20) give on the MI355X next to the NumPy statement
(tests/outliers_numpy.py).

1. the per-case lines the GPU tests print (tests/test_hip_outliers.py, run here with -s): worst mean-distance error over its
   bound, errors of mu and sigma, the statement's smallest gap to the threshold, decisions that differ;
2. the contaminated sphere (20 000 surface points + 400 strays): strays and surface points removed at k = 8 / 20 / 50 and
   std_ratio = 1 / 2 / 3, device and statement;
3. tabulated, not asserted: ISS keypoints of the contaminated sphere before and after the statistical filter.

Needs an MI355X.    python tools/outliers_parity.py [--out profiles/outliers_parity.md]
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_lines() -> tuple[list[str], str]:
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hip_outliers.py"), "-m", "gpu", "-q", "-s",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
    lines = []
    for ln in r.stdout.splitlines():
        for tag in ("OUTLIERS_PARITY ", "OUTLIERS_RADIUS "):
            if tag in ln:
                lines.append(ln[ln.index(tag):])
    tail = [ln for ln in r.stdout.splitlines() if " passed" in ln or " failed" in ln]
    return lines, (tail[-1].strip() if tail else f"pytest exit code {r.returncode}")


def fields(line: str) -> dict:
    parts = line.split()
    return {"case": parts[1], **dict(p.split("=", 1) for p in parts[2:])}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outliers_parity.md"))
    a = ap.parse_args()
    import outliers_numpy as O
    import shot_fpfh_amd as s
    from shot_fpfh_amd.keypoint_selection import select_keypoints_iss

    lines, verdict = test_lines()
    engine = s.Engine()
    md = ["# Outlier removal (K20): the device next to the NumPy statement", "",
          f"Library `{engine.lib.sf_version().decode()}`; written by `tools/outliers_parity.py`.", "",
          f"## The GPU tests (`tests/test_hip_outliers.py`): {verdict}", "",
          "Bound of the mean distances: `(k + 4) 2^-52` relative; of mu and sigma: `n 2^-52` relative to `math.fsum` over the device's "
          "own array; the threshold: 2 ulp.  `gap`: the statement's smallest `|mean - threshold| / threshold`.", "",
          "| case | n | k | ratio | removed (statement / device) | worst mean error / bound | mu rel. | sigma rel. | threshold ulp | gap | decisions that differ |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for ln in lines:
        if ln.startswith("OUTLIERS_PARITY"):
            f = fields(ln)
            md.append(f"| {f['case']} | {f['n']} | {f['k']} | {f['std_ratio']} | {f['removed_numpy']} / {f['removed_device']} | "
                      f"{f['mean_err_over_bound']} | {f['mu_rel']} | {f['sigma_rel']} | {f['threshold_ulps']} | {f['statement_gap']} | "
                      f"{f['decisions_differ']} |")
    md += ["", "Radius filter (counts and kept sets equal the statement's exactly):", "",
           "| case | n | radius | min_neighbors | kept | ball sizes |", "|---|---|---|---|---|---|"]
    for ln in lines:
        if ln.startswith("OUTLIERS_RADIUS"):
            f = fields(ln)
            md.append(f"| {f['case']} | {f['n']} | {f['radius']} | {f['min_neighbors']} | {f['kept']} | {f['counts']} |")

    p = O.contaminated_sphere(20000, 400, 1)
    md += ["", "## Contaminated sphere: 20 000 surface points + 400 strays (`contaminated_sphere(20000, 400, 1)`)", "",
           "strays removed (of 400) / surface points removed, device; the statement's in brackets where it differs", "",
           "| k | std_ratio 1 | std_ratio 2 | std_ratio 3 |", "|---|---|---|---|"]
    cloud = engine.cloud(p)
    try:
        for k in (8, 20, 50):
            row = [str(k)]
            for ratio in (1.0, 2.0, 3.0):
                kept = cloud.statistical_outliers(k, ratio)
                gone = np.setdiff1d(np.arange(p.shape[0]), kept)
                dev = (int((gone >= 20000).sum()), int((gone < 20000).sum()))
                gone = np.setdiff1d(np.arange(p.shape[0]), O.statistical(p, k, ratio)[0])
                ref = (int((gone >= 20000).sum()), int((gone < 20000).sum()))
                row.append(f"{dev[0]} / {dev[1]}" + ("" if dev == ref else f" [{ref[0]} / {ref[1]}]"))
            md.append("| " + " | ".join(row) + " |")
        kept = cloud.statistical_outliers(20, 2.0)
    finally:
        cloud.free()
    md += ["", "## ISS keypoints of the contaminated sphere, before and after the filter (tabulated, not asserted)", "",
           "`select_keypoints_iss(points, 0.04, 0.03)`; after: `remove_statistical_outliers(points, 20, 2.0)` first.", "",
           "| cloud | points | keypoints | of them strays |", "|---|---|---|---|"]
    kp = select_keypoints_iss(p, 0.04, 0.03, engine=engine)
    md.append(f"| as loaded | {p.shape[0]} | {kp.size} | {int((kp >= 20000).sum())} |")
    kp = kept[select_keypoints_iss(p[kept], 0.04, 0.03, engine=engine)]
    md.append(f"| filtered | {kept.size} | {kp.size} | {int((kp >= 20000).sum())} |")
    text = "\n".join(md) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
