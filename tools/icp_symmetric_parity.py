#!/usr/bin/env python3
"""The parity table of symmetric point-to-plane ICP (K19): point-to-plane, generalized and symmetric ICP side by side, from the
NumPy statements on the CPU (tests/gicp_numpy.py, tests/icp_robust_numpy.py, tests/icp_trimmed_numpy.py,
tests/icp_symmetric_numpy.py) and, where there is an MI355X, from the device (shot_fpfh_amd.icp), both with the statement's normals
(20 neighbours) and every scan point kept:
  the corner sets and the curved patch, seeds 0 .. 3, noisy and noise-free, from the identity (0.12 rad off);
  starts 0.17 to 0.7 off in |R - R0| on corner seed 0 and curved seed 0;
  the clutter sets with Cauchy, Geman-McClure and an overlap of 0.8 annealed over 10 iterations.
Entries are |R - R0| (Frobenius), in brackets the iterations.

    python tools/icp_symmetric_parity.py [--out profiles/icp_symmetric_parity.md] [--no-device]
"""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gicp_numpy as G  # noqa: E402
import icp_robust_numpy as S  # noqa: E402
import icp_symmetric_numpy as Y  # noqa: E402
import icp_trimmed_numpy as TR  # noqa: E402

D_MAX, K, EPS, CAP, VOXEL = 0.15, 20, 1e-3, 60, 1e-4
MODES = ("point-to-plane", "generalized", "symmetric")


def with_normals(scan, ref):
    return scan, G.knn_normals(scan, K), ref, G.knn_normals(ref, K)


def statement_row(scan, na, ref, nref, r0, R=None, t=None):
    q = G.icp_point_to_plane(scan, ref, nref, D_MAX, R=R, t=t, max_iter=CAP)
    g = G.icp_generalized(scan, na, ref, nref, D_MAX, R=R, t=t, eps=EPS, max_iter=CAP)
    y = Y.refine(scan, na, ref, nref, D_MAX, R=R, t=t, max_iter=CAP, rms_threshold=0.0)
    return [(G.rotation_error(x["R"], r0), x["iterations"]) for x in (q, g, y)]


def _counted(reg_cls):
    """wrap _Registration.pairs to count the device calls of a run"""
    calls, real = [], reg_cls.pairs

    def pairs(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)

    return calls, real, pairs


def device_row(scan, na, ref, nref, r0, R=None, t=None, robust=None):
    """robust: None, or dict(loss=, scale per mode, overlap=) for the clutter rows"""
    from shot_fpfh_amd import icp
    from shot_fpfh_amd.core import RigidTransform

    start = RigidTransform() if R is None else RigidTransform(R, t)
    kw = dict(voxel_size=VOXEL, max_iter=CAP, rms_threshold=0.0)
    calls, real, pairs = _counted(icp._Registration)
    icp._Registration.pairs = pairs
    row = []
    try:
        for mode in MODES:
            del calls[:]
            if robust is None:
                if mode == "point-to-plane":  # its loop has no step test: all CAP iterations
                    tf = icp.icp_point_to_plane(scan, ref, nref, start, D_MAX, **kw)[0]
                elif mode == "generalized":
                    tf = icp.icp_generalized(scan, ref, start, D_MAX, scan_normals=na, ref_normals=nref, epsilon=EPS, **kw)[0]
                else:
                    tf = icp.icp_symmetric(scan, ref, start, D_MAX, scan_normals=na, ref_normals=nref, **kw)[0]
            else:
                loss, overlap = robust["loss"], robust["overlap"]
                scale, scale_start = robust["scales"][mode]
                if mode == "symmetric":
                    tf = icp.icp_symmetric(scan, ref, start, D_MAX, scan_normals=na, ref_normals=nref, loss=loss, scale=scale,
                                           scale_start=scale_start, overlap=overlap, **kw)[0]
                else:
                    name = "point_to_plane" if mode == "point-to-plane" else "generalized"
                    tf = icp.icp_trimmed(scan, ref, start, D_MAX, overlap=overlap, mode=name, loss=loss, scale=scale, scale_start=scale_start,
                                         ref_normals=nref, scan_normals=na if name == "generalized" else None, epsilon=EPS, **kw)[0]
            row.append((G.rotation_error(tf.rotation, r0), len(calls)))
    finally:
        icp._Registration.pairs = real
    return row


def robust_statement_row(scan, na, ref, nref, r0, loss, overlap):
    scales = {"point-to-plane": S.table_scales("point_to_plane", loss, EPS), "generalized": S.table_scales("generalized", loss, EPS)}
    scales["symmetric"] = scales["point-to-plane"]  # h is a length in both
    row = []
    for mode, kind in (("point-to-plane", S.PLANE), ("generalized", S.GICP)):
        x = TR.refine(scan, na, ref, nref, kind, D_MAX, overlap, TR.ANNEAL, loss=S.LOSSES[loss], scale=scales[mode][0], scale_start=scales[mode][1],
                      eps=EPS, max_iter=CAP, rms_threshold=0.0)
        row.append((G.rotation_error(x["R"], r0), x["iterations"]))
    y = Y.refine(scan, na, ref, nref, D_MAX, loss=S.LOSSES[loss], scale=scales["symmetric"][0], scale_start=scales["symmetric"][1],
                 overlap=overlap, anneal_iterations=TR.ANNEAL, max_iter=CAP, rms_threshold=0.0)
    row.append((G.rotation_error(y["R"], r0), y["iterations"]))
    return row, scales


def cells(row):
    return " | ".join(f"{e:.4e} ({it})" for e, it in row)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_symmetric_parity.md"))
    ap.add_argument("--no-device", action="store_true")
    a = ap.parse_args()
    device = None
    if not a.no_device:
        try:
            from shot_fpfh_amd.engine import default_engine

            device = default_engine().lib.sf_version().decode()
        except Exception as exc:  # noqa: BLE001 -- no GPU here: the statement's columns alone
            print(f"no device columns: {exc}", file=sys.stderr)
    head = "| seed | " + " | ".join(MODES) + " | plane / symmetric |" + (" " + " | ".join("device: " + m for m in MODES) + " |" if device else "")
    rule = "|---|---|---|---|---|" + ("---|---|---|" if device else "")
    out = ["# Symmetric point-to-plane ICP (K19): parity with point-to-plane and generalized ICP", "",
           "Written by `tools/icp_symmetric_parity.py`.  Scan and reference are sampled independently from one surface, 1 500 points each;",
           "the true motion is 0.12 rad about (2, -1, 2)/3 and t = (0.04, -0.03, 0.05).  Every run has d_max = 0.15, the normals of both clouds",
           f"from {K} neighbours (`gicp_numpy.knn_normals`), epsilon = {EPS:g} for generalized ICP, at most {CAP} iterations.  Entries are the",
           "Frobenius norm of R - R0, in brackets the iterations.  The statement columns stop once no component of the step reaches 1e-9.", ""]
    if device:
        out += [f"Device columns: `shot_fpfh_amd.icp` on an MI355X ({device}) with the same normals given, voxel size {VOXEL:g} (every point kept),",
                f"`rms_threshold = 0`: `icp_point_to_plane` has no step test and runs all {CAP} iterations (and applies the reference's Euler",
                "product, not the exponential the statement's point-to-plane applies); the other two stop on their step.", ""]
    else:
        out += ["No device columns: this table was written without a GPU.", ""]
    ratios = {}
    for family, make in (("corner of three planar patches", G.corner_set), ("curved patch", Y.curved_set)):
        for title, sigma in (("sigma = 0.002", 0.002), ("noise-free", 0.0)):
            out += [f"## {family}, {title}, from the identity", "", head, rule]
            for seed in range(4):
                scan, ref, r0, t0 = make(seed, 1500, sigma)
                sets = with_normals(scan, ref)
                row = statement_row(*sets, r0)
                ratios.setdefault(f"{family}, {title}", []).append(row[0][0] / row[2][0])
                line = f"| {seed} | {cells(row)} | {row[0][0] / row[2][0]:.2f} |"
                if device:
                    line += f" {cells(device_row(*sets, r0))} |"
                out.append(line)
                print(line, flush=True)
            out.append("")
    out += ["## Starts farther off (seed 0, sigma = 0.002)", "",
            "The start is a rotation about the true motion's axis, away from it, so that |R_start - R0| is the figure of the first column;",
            "t_start = 0.  No claim of a wider basin: the table shows where each mode ends.", "",
            "| set | start off by | " + " | ".join(MODES) + " |" + (" " + " | ".join("device: " + m for m in MODES) + " |" if device else ""),
            "|---|---|---|---|---|" + ("---|---|---|" if device else "")]
    for family, make in (("corner", G.corner_set), ("curved", Y.curved_set)):
        scan, ref, r0, t0 = make(0)
        sets = with_normals(scan, ref)
        for off in (2.0 * math.sqrt(2.0) * math.sin(0.06), 0.3, 0.5, 0.7):
            theta = 2.0 * math.asin(off / (2.0 * math.sqrt(2.0)))
            R = G.rodrigues((G.TRUE_ANGLE - theta) * G.TRUE_AXIS)
            row = statement_row(*sets, r0, R=R, t=np.zeros(3))
            line = f"| {family} | {G.rotation_error(R, r0):.2f} | {cells(row)} |"
            if device:
                line += f" {cells(device_row(*sets, r0, R=R, t=np.zeros(3)))} |"
            out.append(line)
            print(line, flush=True)
    out += ["", "## The clutter sets (a fifth of the scan is a patch the reference does not have), seeds 0 .. 3", "",
            "`icp_robust_numpy.clutter_set`; the loss's scale comes down from d_max to 0.006 (`table_scales`; generalized ICP's in its own unit),",
            "the share from 1 to the overlap over 10 iterations; point-to-plane and generalized ICP through `icp_trimmed`.", "",
            "| loss, overlap | seed | " + " | ".join(MODES) + " |" + (" " + " | ".join("device: " + m for m in MODES) + " |" if device else ""),
            "|---|---|---|---|---|" + ("---|---|---|" if device else "")]
    for loss, overlap in (("none", 1.0), ("cauchy", 1.0), ("geman_mcclure", 1.0), ("none", 0.8), ("cauchy", 0.8)):
        for seed in range(4):
            scan, ref, r0, t0 = S.clutter_set(seed)
            sets = with_normals(scan, ref)
            row, scales = robust_statement_row(*sets, r0, loss, overlap)
            line = f"| {loss}, {overlap:g} | {seed} | {cells(row)} |"
            if device:
                line += f" {cells(device_row(*sets, r0, robust=dict(loss=loss, overlap=overlap, scales=scales)))} |"
            out.append(line)
            print(line, flush=True)
    out += ["", "## What the table says", ""]
    for title, r in ratios.items():
        out.append(f"- {title}: point-to-plane's rotation error is {min(r):.2f} to {max(r):.2f} times the symmetric objective's.")
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
