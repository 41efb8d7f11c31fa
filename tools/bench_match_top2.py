#!/usr/bin/env python3
"""Times K8's top-2 (sf_match_top2) against its arg-min (sf_match_argmin) in one process, on device-resident SHOT-like rows
(sparse, non-negative, unit norm) at 16 384^2 and 65 536^2 x 352.  The arg-min runs with SF_MATCH_HALF=0 SF_MATCH_I8=0 (set
here, before the library reads them), so both calls take the FP64 matrix-core path.  Wall time per call (median of --reps,
stream synchronised), TFLOP/s as 2 m1 m2 d / t, kernel times from the engine's event profiler, and the rows the exact kernel
decided (n_exact).  Prints one JSON object; --out FILE writes it there as well.

    python tools/bench_match_top2.py [--reps 5] [--sizes 16384,65536] [--out profiles/match_top2_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ["SF_MATCH_HALF"] = "0"
os.environ["SF_MATCH_I8"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from shot_fpfh_amd import _ffi  # noqa: E402
from shot_fpfh_amd.engine import Engine  # noqa: E402


def shot_like(rng, m, d):
    x = rng.random((m, d)) * (rng.random((m, d)) < 0.3)
    x[:, 0] += 1e-3
    return x / np.linalg.norm(x, axis=1)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="16384,65536")
    ap.add_argument("--d", type=int, default=352)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = Engine()
    d = args.d
    res = {"d": d, "rows": "SHOT-like: 30 % non-zero, non-negative, unit norm", "env": "SF_MATCH_HALF=0 SF_MATCH_I8=0",
           "version": _ffi.load().sf_version().decode(), "sizes": []}
    for m in (int(s) for s in args.sizes.split(",")):
        rng = np.random.default_rng(m)
        da, db = eng.empty((m, d)).from_host(shot_like(rng, m, d)), eng.empty((m, d)).from_host(shot_like(rng, m, d))
        idx2, dist2 = eng.empty((m, 2), np.int64), eng.empty((m, 2))
        idx1, dist1 = eng.empty((m,), np.int64), eng.empty((m,))
        flop = 2.0 * m * m * d
        row = {"m1": m, "m2": m, "flop": flop}

        def timed(label, fn):
            fn()  # warm-up: first-call allocations
            eng.sync()
            walls, kern, extra = [], {}, None
            for _ in range(args.reps):
                eng.profile_reset()
                eng.profile(True)
                t0 = time.perf_counter()
                extra = fn()
                eng.sync()
                walls.append(time.perf_counter() - t0)
                eng.profile(False)
                for k, (launches, ms) in eng.profile_report().items():
                    if launches and k.startswith("k8"):
                        kern.setdefault(k, []).append(ms)
            t = float(np.median(walls))
            row[label] = {"wall_ms": round(t * 1e3, 3), "TFLOPs": round(flop / t / 1e12, 2),
                          "kernels_ms": {k: round(float(np.median(v)), 4) for k, v in sorted(kern.items())}}
            if extra is not None:
                row[label]["n_exact"] = extra

        timed("argmin", lambda: eng.match_argmin_device(da, db, idx1, dist1))
        timed("top2", lambda: eng.match_top2_device(da, db, idx2, dist2))
        assert np.array_equal(idx2.to_host()[:, 0], idx1.to_host())
        row["top2_over_argmin"] = round(row["top2"]["wall_ms"] / row["argmin"]["wall_ms"], 3)
        res["sizes"].append(row)
        print(json.dumps(row), file=sys.stderr)
        for x in (da, db, idx2, dist2, idx1, dist1):
            x.free()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
