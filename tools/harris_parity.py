#!/usr/bin/env python3
"""Writes profiles/harris_parity.md: how close the Harris 3D detector (K23) on the MI355X comes to the NumPy statement of its
definition (tests/harris_numpy.py), per cloud and method -- the HARRIS_PARITY, HARRIS_SELECT and HARRIS_THRESHOLD lines that
tests/test_hip_harris.py prints before it asserts.  The ratios are measured error over derived bound (the derivation: that
test's docstring); 1.0 is the bound.

The tests run in a child process (this one never opens the GPU); a log of an earlier run can be tabulated instead.

Needs an MI355X.    python tools/harris_parity.py [--log FILE] [--out profiles/harris_parity.md]
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fields(line: str) -> dict:
    return dict(re.findall(r"(\w+)=(\S+)", line))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log", default=None, help="tabulate this output of `pytest -m gpu -s tests/test_hip_harris.py` instead of running it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harris_parity.md"))
    a = ap.parse_args()
    if a.log:
        text, verdict = open(a.log, errors="replace").read(), None
    else:
        run = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-s", "-q", os.path.join("tests", "test_hip_harris.py")],
                             cwd=ROOT, capture_output=True, text=True)
        text, verdict = run.stdout, run.returncode
    library = subprocess.run([sys.executable, "-c", "from shot_fpfh_amd import _ffi; print(_ffi.load().sf_version().decode())"],
                             cwd=ROOT, capture_output=True, text=True).stdout.strip()
    # (with -q -s a test's progress dot precedes its first printed line: the lines are found anywhere in a line of output)
    parity = [m.split() for m in re.findall(r"HARRIS_PARITY [^\n]*", text)]
    select = [m.split() for m in re.findall(r"HARRIS_SELECT [^\n]*", text)]
    thresh = re.findall(r"HARRIS_THRESHOLD [^\n]*", text)
    if not parity:
        print(text[-4000:])
        raise SystemExit("no HARRIS_PARITY line in the output: did the tests run on a GPU?")
    clouds, methods = sorted({w[1] for w in parity}), sorted({w[2] for w in parity})
    for what, rows in (("HARRIS_PARITY", parity), ("HARRIS_SELECT", select)):
        seen = sorted((w[1], w[2]) for w in rows)
        if seen != sorted((c, m) for c in clouds for m in methods) or len(methods) != 5:
            raise SystemExit(f"{what}: {len(rows)} lines for {len(clouds)} clouds x {len(methods)} methods -- one line per cloud and "
                             "method was expected, the output is incomplete")
    if len(thresh) != len(methods):
        raise SystemExit(f"HARRIS_THRESHOLD: {len(thresh)} lines for {len(methods)} methods")
    last = re.findall(r"^\d+ (?:passed|failed).*$", text, flags=re.M)
    md = ["# Harris 3D keypoints (K23): the device against the NumPy statement", "",
          f"Library `{library}`; written by `tools/harris_parity.py` from the lines `tests/test_hip_harris.py` prints"
          + (f" (pytest exit code {verdict})" if verdict is not None else "") + (f"; pytest: {last[-1]}" if last else "") + ".", "",
          "Ball sizes are equal on every cloud (asserted).  `tensor / bound`: the worst |C_dev - C| over 1.01 (k + 2) 2^-53 sum|n_a n_b| / k "
          "(curvature: the worst eigenvalue difference of the position covariance over 1e-9 e1).  `response / bound`: the worst "
          "|response_dev - response| over the method's bound, where both sides accept the point.  `differ`: accept / reject decisions that "
          "differ, all of them at points the statement flags as near a threshold (`near`).", "",
          "| cloud | method | n | r | largest ball | accepted (NumPy) | accepted (device) | tensor / bound | response / bound | differ | near | keypoints |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    kps = {(w[1], w[2]): fields(" ".join(w))["keypoints"] for w in select}
    for w in parity:
        f = fields(" ".join(w))
        md.append(f"| {w[1]} | {w[2]} | {f['n']} | {f['r']} | {f['max_ball']} | {f['accepted_numpy']} | {f['accepted_device']} | "
                  f"{float(f['tensor_over_bound']):.3f} | {float(f['response_over_bound']):.3f} | {f['decisions_differ']} | {f['near_threshold']} | "
                  f"{kps.get((w[1], w[2]), '')} |")
    tensor_rows = [w for w in parity if w[2] != "curvature"]
    md += ["", f"Worst over the {len(clouds)} clouds: tensor / bound "
           f"{max(float(fields(' '.join(w))['tensor_over_bound']) for w in tensor_rows):.3f}; response / bound "
           + ", ".join(f"{m} {max(float(fields(' '.join(w))['response_over_bound']) for w in parity if w[2] == m):.3g}" for m in
                       ("harris", "noble", "lowe", "tomasi", "curvature")) + "."]
    md += ["", "The keypoints are K10's suppression of the device's own response at the cloud's r_n, equal to `iss_numpy.select` on every "
           "row (asserted)."]
    if thresh:
        md += ["", "A threshold at the median positive response of the statement (uniform cloud):", "",
               "| method | threshold | accepted | of | decisions that differ |", "|---|---|---|---|---|"]
        for ln in thresh:
            m = re.match(r"HARRIS_THRESHOLD (\w+) median=(\S+) accepted=(\d+) of (\d+) differ=(\d+)", ln)
            md.append("| " + " | ".join(m.groups()) + " |")
    out = "\n".join(md) + "\n"
    print(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out)
    return 0 if not verdict else int(verdict)


if __name__ == "__main__":
    sys.exit(main())
