#!/usr/bin/env python3
"""Times of fast global registration (K12) on one MI355X beside the two RANSAC calls, in one process: 10^6 matches, 30 % true,
  (a) ransac_on_matches, (b) ransac_prerejective at its defaults, (c) fast_global_registration at its defaults (all matches),
host to host -- the three in turn inside every repeat, after --warmup rounds, every figure the median of --repeats (>= 20) rounds
of the host clock around calls that end in a device synchronisation -- and (c) again on matched points already resident
(sf_fgr alone: "device only").  Kernel times come from HIP events around the named launches (Engine.profile) in rounds of their
own.  A second table gives each call's |R - R0|, |t - t0| on sets of falling inlier share.  Needs an MI355X: without one the
engine raises and nothing is printed.

    python tools/bench_fgr.py [--matches 1000000] [--repeats 21] [--warmup 3] [--out profiles/fgr_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_ransac import synthetic_matches  # noqa: E402
from ransac_numpy import synthetic_matches as shuffled_matches  # noqa: E402 -- the sets of the accuracy tests

ACCURACY_SETS = [(20000, 0.30, 0), (20000, 0.10, 1), (20000, 0.05, 2), (2000, 0.30, 3), (200000, 0.30, 4), (20000, 0.50, 5)]


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
    import shot_fpfh_amd.matching.ransac as R
    from shot_fpfh_amd.matching import fast_global_registration, ransac_on_matches, ransac_prerejective

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    scan, ref, si, ri, r0, t0 = synthetic_matches(a.matches, a.inlier_share)
    runs = {
        "a_ransac_on_matches": lambda: ransac_on_matches(si, ri, scan, ref, n_draws=a.draws, draw_size=4, distance_threshold=a.threshold,
                                                         disable_progress_bar=True, engine=engine),
        "b_prerejective_defaults": lambda: ransac_prerejective(si, ri, scan, ref, n_draws=a.draws, distance_threshold=a.threshold,
                                                               engine=engine),
        "c_fast_global_registration": lambda: fast_global_registration(si, ri, scan, ref, distance_threshold=a.threshold, engine=engine),
    }
    da, db = engine.empty((a.matches, 3)), engine.empty((a.matches, 3))
    da.from_host(scan[si]), db.from_host(ref[ri])
    device_only = lambda: engine.fgr_device(da, db, a.matches, a.threshold)  # noqa: E731
    for _ in range(a.warmup):
        for fn in runs.values():
            fn()
        device_only()
    times = {k: [] for k in runs}
    dev_times, last = [], {}
    for _ in range(a.repeats):  # in turn: what the box does meanwhile falls on all of them alike
        for k, fn in runs.items():
            t = time.perf_counter()
            last[k] = fn()
            times[k].append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        device_only()
        dev_times.append((time.perf_counter() - t) * 1e3)
    res = {"tool": "tools/bench_fgr.py", "library": engine.lib.sf_version().decode(), "matches": a.matches, "draws": a.draws,
           "inlier_share": a.inlier_share, "threshold": a.threshold, "repeats": a.repeats, "warmup": a.warmup, "calls": {}}

    def kernels(fn):
        engine.profile(True)
        per = {}
        try:
            for _ in range(5):
                engine.profile_reset()
                fn()
                engine.sync()
                for name, (launches, ms) in engine.profile_report().items():
                    if launches:
                        per.setdefault(name, []).append((launches, ms))
        finally:
            engine.profile(False)
        return {name: {"launches": v[0][0], "ms": statistics.median(x[1] for x in v)} for name, v in sorted(per.items())}

    for k in runs:
        out = last[k]
        res["calls"][k] = {"host_to_host_ms_median": statistics.median(times[k]), "host_to_host_ms_min": min(times[k]),
                           "host_to_host_ms_max": max(times[k]), "inlier_ratio": float(out[0]),
                           "rotation_error": float(np.linalg.norm(out[1].rotation - r0)),
                           "translation_error": float(np.linalg.norm(out[1].translation - t0)), "kernels_ms_median": kernels(runs[k])}
    rec = last["c_fast_global_registration"][2]
    kern = kernels(device_only)
    res["fgr_device_only"] = {"ms_median": statistics.median(dev_times), "ms_min": min(dev_times), "ms_max": max(dev_times),
                              "iterations": rec.iterations, "final_mu": rec.mu, "kernels_ms_median": kern,
                              "split_ms": {"moments_and_setup": sum(v["ms"] for n, v in kern.items() if n in ("k12_fgr_moments", "k12_fgr_setup")),
                                           "sums_passes": kern.get("k12_fgr_sums", {}).get("ms"),
                                           "step_kernels": kern.get("k12_fgr_step", {}).get("ms")}}
    sums_ms = kern.get("k12_fgr_sums", {}).get("ms")
    if sums_ms:  # the passes against what they stream: 48 bytes a match a pass
        res["fgr_device_only"]["sums_pass_us"] = 1e3 * sums_ms / rec.iterations
        res["fgr_device_only"]["sums_stream_TB_per_s"] = 48.0 * a.matches * rec.iterations / (sums_ms * 1e-3) / 1e12
    c = res["calls"]["c_fast_global_registration"]
    res["fgr_gather_upload_and_count_ms"] = c["host_to_host_ms_median"] - res["fgr_device_only"]["ms_median"]
    res["c_over_b"] = c["host_to_host_ms_median"] / res["calls"]["b_prerejective_defaults"]["host_to_host_ms_median"]
    da.free(), db.free()
    # accuracy against the inlier share, all three calls
    table = []
    for m, share, seed in ACCURACY_SETS:
        sk, rk, i0, i1, q0, u0 = shuffled_matches(m, share, seed=seed)
        R.rng = np.random.default_rng(seed=72)
        row = {"matches": m, "true_share": share, "seed": seed}
        for name, fn in (("ransac_on_matches", lambda: ransac_on_matches(i0, i1, sk, rk, n_draws=a.draws, draw_size=4, distance_threshold=a.threshold,
                                                                          disable_progress_bar=True, engine=engine)),
                         ("ransac_prerejective", lambda: ransac_prerejective(i0, i1, sk, rk, n_draws=a.draws, distance_threshold=a.threshold, engine=engine)),
                         ("fast_global_registration", lambda: fast_global_registration(i0, i1, sk, rk, distance_threshold=a.threshold, engine=engine))):
            try:
                out = fn()
                row[name] = {"rotation_error": float(np.linalg.norm(out[1].rotation - q0)),
                             "translation_error": float(np.linalg.norm(out[1].translation - u0)), "inlier_ratio": float(out[0])}
            except ValueError as exc:
                row[name] = {"error": str(exc)}
        table.append(row)
    res["accuracy"] = table
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
