#!/usr/bin/env python3
"""Times the serial SHOT (compute_shot_descriptor's device path) on a 1M-point cloud, 100 000 keypoints, r = 0.03: the kernel
with the bin count as an argument (shot_bins.hip, k5_shot_bins) at n = 5, 11, 16, 32, 64 and the tuned K5 (k5_shot*) at n = 11.
One search, K4 and the descriptor kernel per call; kernel times from the engine's event profiler (median of the timed
calls), wall time per call with the rows left on the device (sf_shot_serial has no device output: its wall time includes
the 28 MB copy to the host).  Prints one JSON object; --out FILE writes it there as well.

    python tools/bench_shot_bins.py [--reps 5] [--out profiles/shot_bins_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bench import make_cloud  # noqa: E402
from shot_fpfh_amd import _ffi  # noqa: E402
from shot_fpfh_amd.engine import Cloud, Engine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = Engine()
    pts, nrm = make_cloud(1_000_000, 3)
    rng = np.random.default_rng(5)
    kp = pts[np.sort(rng.choice(len(pts), 100_000, replace=False))]
    cloud = Cloud(eng, pts, nrm)
    nb = cloud.radius_search(kp, 0.03)
    m = nb.m
    res = {"points": len(pts), "keypoints": m, "radius": 0.03, "version": _ffi.load().sf_version().decode(), "runs": []}

    def timed(label, n, fn):
        fn()  # (warm-up: first-call allocations)
        eng.sync()
        walls, kern = [], {}
        for _ in range(args.reps):
            eng.profile_reset()
            eng.profile(True)
            t0 = time.perf_counter()
            fn()
            eng.sync()
            walls.append(time.perf_counter() - t0)
            eng.profile(False)
            for k, (launches, ms) in eng.profile_report().items():
                if launches and (k.startswith("k5") or k.startswith("k4")):
                    kern.setdefault(k, []).append(ms)
        ks = {k: round(float(np.median(v)), 4) for k, v in sorted(kern.items())}
        desc_ms = sum(v for k, v in ks.items() if k.startswith("k5"))
        row = {"form": label, "n_cosine_bins": n, "wall_ms": round(float(np.median(walls)) * 1e3, 3), "kernels_ms": ks,
               "descriptor_kernel_ms": round(desc_ms, 4),
               "row_store_GBps": round(m * 256 * n / (desc_ms * 1e-3) / 1e9, 1) if desc_ms else None}
        res["runs"].append(row)
        print(json.dumps(row), file=sys.stderr)

    timed("tuned K5 (sf_shot_serial)", 11, lambda: nb.shot_serial(10))
    for n in (5, 11, 16, 32, 64):
        out = eng.empty((m, 32 * n))
        timed("shot_bins (sf_shot_serial_bins)", n, lambda: nb.shot_serial(10, n_cosine_bins=n, out=out))
        out.free()
    k5 = res["runs"][0]["descriptor_kernel_ms"]
    new11 = next(r for r in res["runs"][1:] if r["n_cosine_bins"] == 11)["descriptor_kernel_ms"]
    res["ratio_new_over_tuned_at_11"] = round(new11 / k5, 3) if k5 else None
    nb.free()
    cloud.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
