#!/usr/bin/env python3
"""Generate tests/golden/shot_cosine_bins.npz by IMPORTING the reference (aubin-tchoi/shot-fpfh): its serial
compute_shot_descriptor (shot.py:310-499) with n_cosine_bins other than 11.

Runs only in the build container, where /root/reference exists:

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_shot_bins.py

Stores only data: for every case its inputs, parameters and the reference's rows, or the name of the exception the
reference raised (the even-n planes with normals along the frame's z axis, n = 0, n = -1), plus the library versions.
Keys: <case>_points, <case>_normals, <case>_kp, <case>_radius, <case>_min_nb, <case>_ns, and per n either
<case>_rows_<n> (with <case>_sel_<n>, the keypoint rows it holds) or <case>_raises_<n>.
"""
from __future__ import annotations

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import sklearn  # noqa: E402
from shot_fpfh.descriptors.shot import compute_shot_descriptor  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
VERSIONS = np.array([f"numpy {np.__version__}", f"scipy {scipy.__version__}", f"sklearn {sklearn.__version__}"])


def f32(a):
    """Values on the float32 grid (stored as float32, exactly: the fixture stays under the size limit of a committed file)."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def unit(rng, n):
    nr = rng.standard_normal((n, 3))
    return f32(nr / np.linalg.norm(nr, axis=1)[:, None])


def cloud(n, seed):
    """Synthetic input convention of BASELINE.md 4: float32-grid coordinates, (float32-rounded) unit normals."""
    rng = np.random.default_rng(seed)
    return f32(rng.random((n, 3), dtype=np.float32)), unit(rng, n), rng


def run(arrs, case, p, nr, kp, radius, min_nb, ns, sel=None):
    """The reference on (p, nr, kp) for every n of `ns`; sel: n -> keypoint rows to keep (default: all)."""
    assert all(np.array_equal(f32(a), a) for a in (p, nr, kp))
    arrs[f"{case}_points"], arrs[f"{case}_normals"], arrs[f"{case}_kp"] = (a.astype(np.float32) for a in (p, nr, kp))
    arrs[f"{case}_radius"], arrs[f"{case}_min_nb"], arrs[f"{case}_ns"] = np.float64(radius), np.int64(min_nb), np.array(ns)
    for n in ns:
        rows = np.arange(len(kp)) if sel is None or n not in sel else sel[n]
        try:
            d = compute_shot_descriptor(kp[rows], p, nr, radius, min_neighborhood_size=min_nb, n_cosine_bins=n)
        except Exception as exc:  # noqa: BLE001 -- the exception IS the recorded outcome
            arrs[f"{case}_raises_{n}"] = np.array(type(exc).__name__)
            print(f"  {case} n={n}: {type(exc).__name__}")
            continue
        assert d.shape == (len(rows), 32 * max(n, 0)), d.shape
        arrs[f"{case}_rows_{n}"] = d
        arrs[f"{case}_sel_{n}"] = rows.astype(np.int64)
        print(f"  {case} n={n}: {d.shape}, {int(d.any(axis=1).sum())} non-zero rows")


def main():
    arrs = {}
    # a random cloud, ~60 keypoints: cloud points, random positions, an empty keypoint far off, a sparse one off a corner
    p, nr, rng = cloud(6000, 4101)
    kp = f32(np.vstack([p[:40], rng.random((18, 3)), [[5.0, 5.0, 5.0]], [[1.07, 1.07, 1.07]]]))
    few = np.arange(0, 60, 3)
    run(arrs, "random", p, nr, kp, 0.12, 10, [1, 2, 3, 5, 8, 10, 16, 17, 32, 64], sel={32: few, 64: few})
    # exact duplicates (points and normals): zero-distance neighbours leave the support, equal keys in the elections
    p, nr, rng = cloud(2000, 4102)
    p, nr = np.vstack([p, p[:60], p[:20]]), np.vstack([nr, nr[:60], nr[:20]])
    kp = f32(np.vstack([p[:30], rng.random((10, 3))]))
    run(arrs, "dups", p, nr, kp, 0.17, 5, [3, 8])
    # clustered: lists above 255 and above 3 072 points
    p, nr, rng = cloud(3000, 4103)
    p, nr = np.vstack([p, f32(0.5 + 0.03 * rng.standard_normal((5000, 3)))]), np.vstack([nr, unit(rng, 5000)])
    kp = f32(np.vstack([p[3000:3006], [[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.5, 0.64, 0.45]], p[:3]]))
    from sklearn.neighbors import KDTree

    counts = KDTree(p).query_radius(kp, 0.12, count_only=True)
    assert counts.max() > 3072 and ((counts > 255) & (counts <= 3072)).any(), counts
    arrs["cluster_counts"] = counts.astype(np.int64)
    run(arrs, "cluster", p, nr, kp, 0.12, 10, [5, 16, 64], sel={64: np.array([0, 7, 8, 9])})
    # z = 0 planes: normals +x (cosine 0: a half-integer bin position for every even n) and +z (cosine +1: bin n for even n)
    rng = np.random.default_rng(4104)
    xy = rng.random((2000, 2), dtype=np.float32).astype(np.float64)
    p = np.hstack([xy, np.zeros((2000, 1))])
    kp = p[rng.choice(2000, 24, replace=False)]
    for axis, case in ((0, "plane_x"), (2, "plane_z")):
        nr = np.zeros((2000, 3))
        nr[:, axis] = 1.0
        run(arrs, case, p, nr, kp, 0.1, 10, [1, 2, 3, 4, 5, 8, 11, 16, 0, -1])
    path = os.path.join(OUT, "shot_cosine_bins.npz")
    np.savez_compressed(path, versions=VERSIONS, **arrs)
    print(f"shot_cosine_bins.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
