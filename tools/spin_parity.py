#!/usr/bin/env python3
"""Writes profiles/spin_parity.md: how well spin images (K24) find a keypoint's true counterpart next to FPFH, SHOT, USC and PFH,
from the NumPy statement (tests/spin_numpy.py, on the CPU) and from the MI355X.  Tabulated, not asserted.

The experiment is tools/usc_parity.py's: one bumpy sphere sampled twice, independently, with Gaussian noise along the ray, the
same --keypoints surface locations added to both samplings, the second sampling turned by a rigid rotation; a keypoint counts
when the nearest row of the other cloud is its counterpart's.  Spin images come twice: the signed image about normals oriented
outwards, and the unsigned image about the k-NN (PCA) normals as compute_normals returns them, signs arbitrary.  The other four
descriptors are the device's, with the oriented normals.  The statement takes its lists from a brute-force ball test, the device
from its own search: the rows are equal bit for bit when the two agree on every ball.

Needs an MI355X.    python tools/spin_parity.py [--n 10000] [--keypoints 300] [--radius 0.15] [--out profiles/spin_parity.md]
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
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spin_parity.md"))
    a = ap.parse_args()
    import spin_numpy as S

    import shot_fpfh_amd as s
    from shot_fpfh_amd.descriptors import (ShotMultiprocessor, compute_normals, compute_pfh_descriptor, compute_spin_image_descriptor,
                                           compute_usc_descriptor)

    engine = s.Engine()
    R, m, W = a.radius, a.keypoints, a.width
    kp_idx = np.arange(m)
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))
    rot = q * np.sign(np.linalg.det(q))
    md = ["# Spin images (K24) next to FPFH, SHOT, USC and PFH: nearest row = true counterpart", "",
          f"Library `{engine.lib.sf_version().decode()}`; written by `tools/spin_parity.py`.  {a.n} samples + {m} keypoints per cloud, "
          f"radius {R}, spin images of width {W} (signed: 153 nodes about normals oriented outwards; unsigned: 81 nodes about the k-NN "
          "normals with their arbitrary signs), FPFH 5 bins, SHOT single scale (min_neighborhood_size 10), USC 14 x 14 x 10 bins, PFH 5 "
          "bins per angle.  Share of the keypoints of the first sampling whose nearest row among the second sampling's is their "
          "counterpart's; the statement's columns are computed on the CPU; tabulated, not asserted.", "",
          "| noise (of r) | mean ball | spin signed statement | spin signed device | spin unsigned statement | spin unsigned device | "
          "spin rows equal | FPFH device | SHOT device | USC device | PFH device |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
    for noise in (0.0, 0.002, 0.005, 0.01):
        rng = np.random.default_rng(11)
        key_dirs = directions(m, rng)
        clouds = [sampling(a.n, key_dirs, noise, rng), sampling(a.n, key_dirs, noise, rng) @ rot.T]
        rows, ball, same = {}, [], True
        for side, p in enumerate(clouds):
            pca = compute_normals(p, p, k=20)
            centre = p.mean(axis=0)
            nrm = pca * np.sign(((p - centre) * pca).sum(axis=1))[:, None]
            kp = p[kp_idx]
            lists = [np.flatnonzero(((p - c) ** 2).sum(axis=1) <= R * R) for c in kp]
            ball.append(np.mean([len(b) for b in lists]))
            rows["signed_dev", side] = compute_spin_image_descriptor(kp_idx, p, nrm, R, W, engine=engine)
            rows["signed_np", side] = S.rows(p, None, kp, nrm[kp_idx], lists, R, W, True)
            rows["unsigned_dev", side] = compute_spin_image_descriptor(kp_idx, p, pca, R, W, signed_beta=False, engine=engine)
            rows["unsigned_np", side] = S.rows(p, None, kp, pca[kp_idx], lists, R, W, False)
            same = same and all(np.array_equal(rows[f"{k}_dev", side], rows[f"{k}_np", side]) for k in ("signed", "unsigned"))
            rows["fpfh", side] = s.compute_fpfh_descriptor(kp_idx, p, nrm, R, 5, verbose=False)
            with ShotMultiprocessor(min_neighborhood_size=10, verbose=False) as sm:
                rows["shot", side] = sm.compute_descriptor_single_scale(p, nrm, kp, R)
            rows["usc", side] = compute_usc_descriptor(p, kp, R, engine=engine)
            rows["pfh", side] = compute_pfh_descriptor(kp_idx, p, nrm, R, 5, engine=engine)
        share = {k: hit_share(rows[k, 0], rows[k, 1]) for k in ("signed_np", "signed_dev", "unsigned_np", "unsigned_dev", "fpfh", "shot",
                                                                "usc", "pfh")}
        md.append(f"| {noise} | {np.mean(ball):.0f} | {share['signed_np']:.3f} | {share['signed_dev']:.3f} | {share['unsigned_np']:.3f} | "
                  f"{share['unsigned_dev']:.3f} | {'yes' if same else 'NO'} | {share['fpfh']:.3f} | {share['shot']:.3f} | "
                  f"{share['usc']:.3f} | {share['pfh']:.3f} |")
    md += ["", "One synthetic surface; real scans are not measured."]
    text = "\n".join(md) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
