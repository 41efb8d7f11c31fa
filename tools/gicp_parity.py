#!/usr/bin/env python3
"""The parity table of generalized ICP (K16): point-to-point, point-to-plane and generalized ICP side by side on two independent
samplings of one surface (three unequal planar patches meeting at a corner; tests/gicp_numpy.py), from the NumPy statement of the
definition on the CPU and, where there is an MI355X, from the device (shot_fpfh_amd.icp, normals from its own k-NN pass).  Also
measures the statement's sensitivity to the order of its sums, the margin tests/test_hip_gicp.py takes for the whole run.

    python tools/gicp_parity.py [--out profiles/gicp_parity.md] [--no-device]
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

D_MAX, K, EPS, CAP = 0.15, 20, 1e-3, 60
SETS = [("1 500 points, sigma = 0.002", 1500, 0.002), ("4 000 points, sigma = 0.002", 4000, 0.002), ("1 500 points, noise-free", 1500, 0.0)]


def statement_row(scan, ref, r0):
    na, nref = G.knn_normals(scan, K), G.knn_normals(ref, K)
    p = G.icp_point_to_point(scan, ref, D_MAX, max_iter=CAP)
    q = G.icp_point_to_plane(scan, ref, nref, D_MAX, max_iter=CAP)
    g = G.icp_generalized(scan, na, ref, nref, D_MAX, eps=EPS, max_iter=CAP)
    return [(G.rotation_error(x["R"], r0), x["iterations"]) for x in (p, q, g)]


def device_row(scan, ref, r0):
    from shot_fpfh_amd import compute_normals, icp
    from shot_fpfh_amd.core import RigidTransform

    kw = dict(d_max=D_MAX, voxel_size=0.01, max_iter=CAP, rms_threshold=0.0)
    p = icp.icp_point_to_point(scan, ref, RigidTransform(), **kw)[0]
    q = icp.icp_point_to_plane(scan, ref, compute_normals(ref, ref, k=K), RigidTransform(), **kw)[0]
    g = icp.icp_generalized(scan, ref, RigidTransform(), k_normals=K, epsilon=EPS, **kw)[0]
    return [G.rotation_error(x.rotation, r0) for x in (p, q, g)]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_parity.md"))
    ap.add_argument("--no-device", action="store_true")
    a = ap.parse_args()
    device = None
    if not a.no_device:
        try:
            from shot_fpfh_amd.engine import default_engine

            device = default_engine().lib.sf_version().decode()
        except Exception as exc:  # noqa: BLE001 -- no GPU here: the statement's columns alone
            print(f"no device columns: {exc}", file=sys.stderr)
    out = ["# Generalized ICP (K16): parity with point-to-point and point-to-plane ICP", "",
           "Written by `tools/gicp_parity.py`.  The surface is three unequal planar patches meeting at a corner (1.0 x 0.8, 1.0 x 0.6,",
           "0.8 x 0.6); scan and reference are sampled independently.  The true motion is 0.12 rad about (2, -1, 2)/3 and",
           f"t = (0.04, -0.03, 0.05); every run starts at the identity with d_max = {D_MAX}, normals from {K} neighbours, epsilon = {EPS:g},",
           f"at most {CAP} iterations.  Entries are the Frobenius norm of R - R0; in brackets the statement's iterations until no",
           "component of its step reaches 1e-9.  The statement is `tests/gicp_numpy.py` (float64 NumPy on the CPU).", ""]
    if device:
        out += [f"Device columns: `shot_fpfh_amd.icp` on an MI355X ({device}), voxel size 0.01 (nearly every point is kept),",
                f"`rms_threshold = 0`: point-to-point and point-to-plane run all {CAP} iterations, generalized ICP until its step test.", ""]
    else:
        out += ["No device columns: this table was written without a GPU.", ""]
    ratios, plane = {}, {}
    for title, n, sigma in SETS:
        out += [f"## {title}", ""]
        head = "| seed | point-to-point | point-to-plane | generalized | p2p / generalized |"
        rule = "|---|---|---|---|---|"
        if device:
            head += " device: point-to-point | device: point-to-plane | device: generalized |"
            rule += "---|---|---|"
        out += [head, rule]
        for seed in range(4):
            scan, ref, r0, t0 = G.corner_set(seed, n, sigma)
            row = statement_row(scan, ref, r0)
            ratios.setdefault(title, []).append(row[0][0] / row[2][0])
            plane.setdefault(title, []).append(row[1][0] / row[2][0])
            line = f"| {seed} | " + " | ".join(f"{e:.2e} ({it})" for e, it in row) + f" | {row[0][0] / row[2][0]:.1f} |"
            if device:
                line += " " + " | ".join(f"{e:.2e}" for e in device_row(scan, ref, r0)) + " |"
            out.append(line)
            print(line)
        out.append("")
    out += ["## What the table says", ""]
    for title, r in ratios.items():
        out.append(f"- {title}: generalized ICP's rotation error is {min(r):.1f} to {max(r):.1f} times smaller than point-to-point's.")
    for title, r in plane.items():
        out.append(f"- {title}: point-to-plane's error is {min(r):.2f} to {max(r):.2f} times generalized ICP's.")
    out += ["- On the noisy sets generalized ICP is on a par with point-to-plane, better on some seeds and worse on others, not better:",
            "  both remove the pull of sample points onto sample points.  What it adds is that the caller brings no normals, and the",
            "  noise-free sets, where the scan's own surface counts too.", ""]
    # the statement's own sensitivity to the order of its sums (seed 0, 1 500 points)
    scan, ref, r0, t0 = G.corner_set(0)
    na, nref = G.knn_normals(scan, K), G.knn_normals(ref, K)
    exact = G.icp_generalized(scan, na, ref, nref, D_MAX, max_iter=CAP, step_tolerance=2e-9)
    own = 0.0
    for s in range(4):
        order = np.random.default_rng(17 + s).permutation(scan.shape[0])
        other = G.icp_generalized(scan[order], na[order], ref, nref, D_MAX, max_iter=CAP, step_tolerance=2e-9, how="np")
        own = max(own, float(np.abs(exact["R"] - other["R"]).max()), float(np.abs(exact["t"] - other["t"]).max()))
    out += ["## The statement's sensitivity to the order of its sums", "",
            f"Seed 0, 1 500 points, step tolerance 2e-9: {exact['iterations']} iterations, steps "
            + ", ".join(f"{x:.1e}" for x in exact["steps"]) + ".",
            f"The run with `math.fsum` against four runs on row-permuted scans with NumPy's pairwise sums: R and t differ by at most {own:.2e}.",
            "`tests/test_hip_gicp.py` holds the device's whole run to ten times this figure, measured again in the test.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
