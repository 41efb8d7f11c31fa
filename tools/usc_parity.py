#!/usr/bin/env python3
"""Writes profiles/usc_parity.md: how well Unique Shape Context (K21) finds a keypoint's true counterpart next to SHOT and FPFH,
from the NumPy statement (tests/usc_numpy.py; SHOT and FPFH: the CPU oracle) and from the MI355X.  Tabulated, not asserted.

One surface -- a sphere of radius 0.5 with bumps, r = 0.5 (1 + 0.1 sin 9 theta sin 8 phi) -- is sampled twice, independently,
with Gaussian noise along the ray; the same --keypoints surface locations are added to both samplings (a keypoint's counterpart
is the keypoint of the same number), and the second sampling is turned by a rigid rotation.  Normals: the package's own k-NN
normals, oriented outwards.  A keypoint counts when the nearest row of the other cloud (brute-force arg-min) is its counterpart's.

Needs an MI355X.    python tools/usc_parity.py [--n 40000] [--keypoints 300] [--radius 0.15] [--out profiles/usc_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def surface(direction: np.ndarray) -> np.ndarray:
    theta = np.arccos(np.clip(direction[:, 2], -1, 1))
    phi = np.arctan2(direction[:, 1], direction[:, 0])
    return direction * (0.5 * (1.0 + 0.1 * np.sin(9 * theta) * np.sin(8 * phi)))[:, None]


def directions(n: int, rng) -> np.ndarray:
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1)[:, None]


def sampling(n: int, key_dirs: np.ndarray, noise: float, rng) -> np.ndarray:
    """the keypoints first (exact surface points), then n noisy samples"""
    d = directions(n, rng)
    return np.vstack([surface(key_dirs), surface(d) * (1.0 + noise * rng.standard_normal((n, 1)))])


def hit_share(a: np.ndarray, b: np.ndarray) -> float:
    """share of rows of a whose nearest row of b (both non-empty) has the same number"""
    ok = a.any(axis=1)
    best = np.array([np.argmin(((b - row) ** 2).sum(axis=1)) if keep else -1 for row, keep in zip(a, ok)])
    return float((best == np.arange(a.shape[0])).mean())


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--keypoints", type=int, default=300)
    ap.add_argument("--radius", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usc_parity.md"))
    a = ap.parse_args()
    import usc_numpy as U
    from sklearn.neighbors import KDTree

    import shot_fpfh_amd as s
    from oracle import oracle as O
    from shot_fpfh_amd.descriptors import ShotMultiprocessor, compute_normals, compute_usc_descriptor

    engine = s.Engine()
    R, m = a.radius, a.keypoints
    kp_idx = np.arange(m)
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((3, 3)))
    rot = q * np.sign(np.linalg.det(q))
    md = ["# Unique Shape Context (K21) next to SHOT and FPFH: nearest row = true counterpart", "",
          f"Library `{engine.lib.sf_version().decode()}`; written by `tools/usc_parity.py`.  {a.n} samples + {m} keypoints per cloud, "
          f"radius {R}, USC 14 x 14 x 10 bins (min_radius R / 10, density_radius R / 5), SHOT single scale (min_neighborhood_size 10), "
          "FPFH 5 bins.  Share of the keypoints of the first sampling whose nearest row among the second sampling's is their "
          "counterpart's; tabulated, not asserted.", "",
          "| noise (of r) | USC statement | USC device | USC rows equal | SHOT oracle | SHOT device | FPFH oracle | FPFH device |",
          "|---|---|---|---|---|---|---|---|"]
    for noise in (0.0, 0.002, 0.005, 0.01):
        rng = np.random.default_rng(11)
        key_dirs = directions(m, rng)
        clouds = [sampling(a.n, key_dirs, noise, rng), sampling(a.n, key_dirs, noise, rng) @ rot.T]
        rows = {}
        for side, p in enumerate(clouds):
            nrm = compute_normals(p, p, k=20)
            centre = p.mean(axis=0)
            nrm *= np.sign(((p - centre) * nrm).sum(axis=1))[:, None]
            kp = p[kp_idx]
            rows["usc_dev", side] = compute_usc_descriptor(p, kp, R, engine=engine)
            lists = KDTree(p).query_radius(kp, R)
            rows["usc_np", side] = U.rows(p, kp, lists, O.shot_lrf(p, kp, R).reshape(-1, 3, 3), U.density_weights(p, R / 5), R)
            with ShotMultiprocessor(min_neighborhood_size=10, verbose=False) as sm:
                rows["shot_dev", side] = sm.compute_descriptor_single_scale(p, nrm, kp, R)
            rows["shot_np", side] = O.shot_single_scale(p, nrm, kp, R, True, 10)
            rows["fpfh_dev", side] = s.compute_fpfh_descriptor(kp_idx, p, nrm, R, 5, verbose=False)
            rows["fpfh_np", side] = O.compute_fpfh_descriptor(kp_idx, p, nrm, R, 5)
        same = all(np.array_equal(rows["usc_dev", side], rows["usc_np", side]) for side in (0, 1))
        share = {k: hit_share(rows[k, 0], rows[k, 1]) for k in ("usc_np", "usc_dev", "shot_np", "shot_dev", "fpfh_np", "fpfh_dev")}
        md.append(f"| {noise} | {share['usc_np']:.3f} | {share['usc_dev']:.3f} | {'yes' if same else 'no (frames differ in the last bits)'} | "
                  f"{share['shot_np']:.3f} | {share['shot_dev']:.3f} | {share['fpfh_np']:.3f} | {share['fpfh_dev']:.3f} |")
    md += ["", "The USC statement here takes its frames from the CPU oracle and its lists and weights from a KDTree, the device its own: "
           "rows are equal only where the two frames agree to the last bit (the GPU tests feed the statement the device's frames and "
           "compare exactly)."]
    text = "\n".join(md) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
