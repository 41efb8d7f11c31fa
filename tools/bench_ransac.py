#!/usr/bin/env python3
"""Times of the coarse registration on one MI355X, host to host, in one process: 10^4 draws over 10^6 matches,
  (a) ransac_on_matches (host Kabsch in stacks, K9 over every draw),
  (b) ransac_prerejective(edge_similarity=0, refit_iterations=0): the same scoring work with the Kabsch fits on the device (K11),
  (c) ransac_prerejective at its defaults: draws that fail the edge-length test are never scored, the winner is refitted.
The three are run in turn inside every repeat, after --warmup rounds; every figure is the median of --repeats (>= 20) rounds
of the host clock around calls that end in a device synchronisation.  Kernel times come from HIP events around the named
launches (Engine.profile) in rounds of their own.  Needs an MI355X: without one the engine raises and nothing is printed.

    python tools/bench_ransac.py [--matches 1000000] [--draws 10000] [--repeats 21] [--warmup 3] [--out profiles/ransac_prerejective_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_matches(m: int, inlier_share: float, sigma: float = 0.002, seed: int = 0):
    """m matches in the unit cube: a share of true ones b = R0 a + t0 + N(0, sigma), the others paired at random."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    r0 = q * np.sign(np.linalg.det(q))
    t0 = rng.uniform(-0.5, 0.5, 3)
    scan = rng.random((m, 3))
    true = rng.random(m) < inlier_share
    ref = np.where(true[:, None], scan.dot(r0.T) + t0 + rng.normal(scale=sigma, size=(m, 3)), rng.random((m, 3)).dot(r0.T) + t0)
    idx = np.arange(m, dtype=np.int64)
    return scan, ref, idx, idx, r0, t0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--matches", type=int, default=1_000_000)
    ap.add_argument("--draws", type=int, default=10_000)
    ap.add_argument("--inlier-share", type=float, default=0.3)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd.matching import ransac_on_matches, ransac_prerejective

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    scan, ref, si, ri, r0, t0 = synthetic_matches(a.matches, a.inlier_share)
    common = dict(n_draws=a.draws, distance_threshold=a.threshold, engine=engine)
    runs = {
        "a_ransac_on_matches": lambda: ransac_on_matches(si, ri, scan, ref, draw_size=4, disable_progress_bar=True, **common),
        "b_prerejective_all_scored": lambda: ransac_prerejective(si, ri, scan, ref, edge_similarity=0.0, refit_iterations=0, **common),
        "c_prerejective_defaults": lambda: ransac_prerejective(si, ri, scan, ref, **common),
    }
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
    times = {k: [] for k in runs}
    last = {}
    for _ in range(a.repeats):  # the three in turn: what the box does meanwhile falls on all of them alike
        for k, fn in runs.items():
            t = time.perf_counter()
            last[k] = fn()
            times[k].append((time.perf_counter() - t) * 1e3)
    res = {"tool": "tools/bench_ransac.py", "library": engine.lib.sf_version().decode(), "matches": a.matches, "draws": a.draws,
           "inlier_share": a.inlier_share, "threshold": a.threshold, "repeats": a.repeats, "warmup": a.warmup, "calls": {}}
    for k in runs:
        out = last[k]
        tf = out[1]
        row = {"host_to_host_ms_median": statistics.median(times[k]), "host_to_host_ms_min": min(times[k]),
               "host_to_host_ms_max": max(times[k]), "inlier_ratio": float(out[0]),
               "rotation_error": float(np.linalg.norm(tf.rotation - r0)), "translation_error": float(np.linalg.norm(tf.translation - t0))}
        if len(out) > 2:
            rec = out[2]
            row.update(scored=rec.n_scored, rejected=rec.n_rejected, degenerate=rec.n_degenerate, share_scored=rec.n_scored / rec.n_draws,
                       winner_draw=rec.winner_draw, winner_inliers=rec.winner_inliers, refit_inliers=rec.refit_inliers)
        # per-kernel device times: rounds of their own (two event records per launch cost host time)
        engine.profile(True)
        per = {}
        try:
            for _ in range(5):
                engine.profile_reset()
                runs[k]()
                engine.sync()
                for name, (launches, ms) in engine.profile_report().items():
                    if launches:
                        per.setdefault(name, []).append((launches, ms))
        finally:
            engine.profile(False)
        row["kernels_ms_median"] = {name: {"launches": v[0][0], "ms": statistics.median(x[1] for x in v)} for name, v in sorted(per.items())}
        res["calls"][k] = row
    ta, tb, tc = (res["calls"][k]["host_to_host_ms_median"] for k in runs)
    res["b_over_a"], res["c_over_b"] = tb / ta, tc / tb
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
