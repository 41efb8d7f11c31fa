#!/usr/bin/env python3
"""Writes profiles/pfh_parity.md: how well Point Feature Histograms (K22) find a keypoint's true counterpart next to FPFH, SHOT
and USC, from the NumPy statement (tests/pfh_numpy.py; the others: as tools/usc_parity.py takes them) and from the MI355X.
Tabulated, not asserted.

The experiment is tools/usc_parity.py's: one bumpy sphere sampled twice, independently, with Gaussian noise along the ray, the
same --keypoints surface locations added to both samplings, the second sampling turned by a rigid rotation; a keypoint counts
when the nearest row of the other cloud is its counterpart's.  PFH's statement is quadratic in the ball size on the host, so the
default cloud is smaller than that tool's (--n 10000: about 225 points per ball at radius 0.15).

Needs an MI355X.    python tools/pfh_parity.py [--n 10000] [--keypoints 300] [--radius 0.15] [--out profiles/pfh_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from usc_parity import directions, hit_share, sampling  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--keypoints", type=int, default=300)
    ap.add_argument("--radius", type=float, default=0.15)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfh_parity.md"))
    a = ap.parse_args()
    import pfh_numpy as P
    import usc_numpy as U
    from sklearn.neighbors import KDTree

    import shot_fpfh_amd as s
    from oracle import oracle as O
    from shot_fpfh_amd.descriptors import ShotMultiprocessor, compute_normals, compute_pfh_descriptor, compute_usc_descriptor

    engine = s.Engine()
    R, m, S = a.radius, a.keypoints, a.bins
    kp_idx = np.arange(m)
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))
    rot = q * np.sign(np.linalg.det(q))
    md = ["# Point Feature Histograms (K22) next to FPFH, SHOT and USC: nearest row = true counterpart", "",
          f"Library `{engine.lib.sf_version().decode()}`; written by `tools/pfh_parity.py`.  {a.n} samples + {m} keypoints per cloud, "
          f"radius {R}, PFH {S} bins per angle, FPFH 5 bins, SHOT single scale (min_neighborhood_size 10), USC 14 x 14 x 10 bins.  "
          "Share of the keypoints of the first sampling whose nearest row among the second sampling's is their counterpart's; "
          "tabulated, not asserted.", "",
          "| noise (of r) | mean ball | PFH statement | PFH device | PFH rows equal | FPFH oracle | FPFH device | SHOT oracle | SHOT device | USC statement | USC device |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for noise in (0.0, 0.002, 0.005, 0.01):
        rng = np.random.default_rng(11)
        key_dirs = directions(m, rng)
        clouds = [sampling(a.n, key_dirs, noise, rng), sampling(a.n, key_dirs, noise, rng) @ rot.T]
        rows, ball = {}, []
        for side, p in enumerate(clouds):
            nrm = compute_normals(p, p, k=20)
            centre = p.mean(axis=0)
            nrm *= np.sign(((p - centre) * nrm).sum(axis=1))[:, None]
            kp = p[kp_idx]
            lists = KDTree(p).query_radius(kp, R)
            ball.append(np.mean([len(b) for b in lists]))
            rows["pfh_dev", side] = compute_pfh_descriptor(kp_idx, p, nrm, R, S, engine=engine)
            rows["pfh_np", side] = P.rows(p, nrm, lists, S)
            rows["fpfh_dev", side] = s.compute_fpfh_descriptor(kp_idx, p, nrm, R, 5, verbose=False)
            rows["fpfh_np", side] = O.compute_fpfh_descriptor(kp_idx, p, nrm, R, 5)
            with ShotMultiprocessor(min_neighborhood_size=10, verbose=False) as sm:
                rows["shot_dev", side] = sm.compute_descriptor_single_scale(p, nrm, kp, R)
            rows["shot_np", side] = O.shot_single_scale(p, nrm, kp, R, True, 10)
            rows["usc_dev", side] = compute_usc_descriptor(p, kp, R, engine=engine)
            rows["usc_np", side] = U.rows(p, kp, lists, O.shot_lrf(p, kp, R).reshape(-1, 3, 3), U.density_weights(p, R / 5), R)
        same = all(np.array_equal(rows["pfh_dev", side], rows["pfh_np", side]) for side in (0, 1))
        share = {k: hit_share(rows[k, 0], rows[k, 1]) for k in ("pfh_np", "pfh_dev", "fpfh_np", "fpfh_dev", "shot_np", "shot_dev",
                                                                "usc_np", "usc_dev")}
        md.append(f"| {noise} | {np.mean(ball):.0f} | {share['pfh_np']:.3f} | {share['pfh_dev']:.3f} | {'yes' if same else 'NO'} | "
                  f"{share['fpfh_np']:.3f} | {share['fpfh_dev']:.3f} | {share['shot_np']:.3f} | {share['shot_dev']:.3f} | "
                  f"{share['usc_np']:.3f} | {share['usc_dev']:.3f} |")
    md += ["", "The PFH statement takes its lists from a KDTree, the device from its own search: the rows are equal bit for bit when "
           "the two agree on every ball (a row does not depend on the order of a list)."]
    text = "\n".join(md) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
