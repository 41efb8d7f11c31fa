#!/usr/bin/env python3
"""Times of the four ICP modes on one MI355X, in one process: a 10^5-point scan against a 10^6-point reference, two independent
samplings of the corner surface of the parity tables (tests/gicp_numpy.py), normals given,
  (a) icp_point_to_point, (b) icp_point_to_plane, (c) icp_generalized (K16), (d) icp_symmetric (K19), a fixed number of iterations
each, host to host -- the four in turn inside every round, after --warmup rounds, every figure the median of --repeats (>= 20)
rounds of the host clock around calls that end in a device synchronisation -- then ONE iteration's device call (sf_icp_accumulate,
sf_icp_accumulate_gicp, sf_icp_accumulate_symmetric on resident clouds) the same way, and its kernels from HIP events around the
named launches (Engine.profile) in rounds of their own, split into the transform, the k = 1 search and the sums passes
(`i1_icp_sums`, two launches) with their two single-block folds.  Needs an MI355X: without one the engine raises and nothing is
printed.

    python tools/bench_icp_symmetric.py [--scan 100000] [--ref 1000000] [--repeats 21] [--warmup 3] [--out profiles/icp_symmetric_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gicp_numpy as G  # noqa: E402 -- the surface and the true motion of the parity table

FOLDS = ("i1_icp_means", "i1_icp_final")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scan", type=int, default=100_000)
    ap.add_argument("--ref", type=int, default=1_000_000)
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--d-max", type=float, default=0.15)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--voxel", type=float, default=1e-3, help="of the scan's subsampling (the default keeps nearly every point)")
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd import icp
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.engine import default_engine

    engine = default_engine()  # the engine the calls use (raises without a GPU: no figure is ever printed from a CPU)
    rng = np.random.default_rng(16)
    ref = G.corner_surface(a.ref, rng, a.sigma)
    r0, t0 = G.true_motion()
    scan = (G.corner_surface(a.scan, rng, a.sigma) - t0) @ r0
    scan_normals, ref_normals = s.compute_normals(scan, scan, k=20), s.compute_normals(ref, ref, k=20)
    start = RigidTransform()
    common = dict(d_max=a.d_max, voxel_size=a.voxel, max_iter=a.iterations, rms_threshold=0.0)  # no stop before max_iter
    both = dict(scan_normals=scan_normals, ref_normals=ref_normals, step_tolerance=0.0)
    runs = {
        "a_point_to_point": lambda: icp.icp_point_to_point(scan, ref, start, **common),
        "b_point_to_plane": lambda: icp.icp_point_to_plane(scan, ref, ref_normals, start, **common),
        "c_generalized": lambda: icp.icp_generalized(scan, ref, start, **both, **common),
        "d_symmetric": lambda: icp.icp_symmetric(scan, ref, start, **both, **common),
    }
    modes = {"a_point_to_point": icp._POINT, "b_point_to_plane": icp._PLANE, "c_generalized": icp._GICP, "d_symmetric": icp._SYMMETRIC}
    reg = icp._Registration(scan, ref, ref_normals, engine=engine, scan_normals=scan_normals)
    at = RigidTransform(r0, t0)
    one = {k: (lambda mode=mode: reg.pairs(mode, a.d_max, moved_by=at)) for k, mode in modes.items()}
    for _ in range(a.warmup):
        for k in runs:
            runs[k](), one[k]()
    times, one_times, last = {k: [] for k in runs}, {k: [] for k in runs}, {}
    for _ in range(a.repeats):  # in turn: what the box does meanwhile falls on all of them alike
        for k in runs:
            t = time.perf_counter()
            last[k] = runs[k]()
            times[k].append((time.perf_counter() - t) * 1e3)
        for k in runs:
            t = time.perf_counter()
            found = one[k]()
            one_times[k].append((time.perf_counter() - t) * 1e3)
            last[k + "_pairs"] = found.count

    def kernels(fn):
        reg.engine.profile(True)
        per = {}
        try:
            for _ in range(5):
                reg.engine.profile_reset()
                fn()
                reg.engine.sync()
                for name, (launches, ms) in reg.engine.profile_report().items():
                    if launches:
                        per.setdefault(name, []).append((launches, ms))
        finally:
            reg.engine.profile(False)
        return {name: {"launches": v[0][0], "ms": statistics.median(x[1] for x in v)} for name, v in sorted(per.items())}

    res = {"tool": "tools/bench_icp_symmetric.py", "library": engine.lib.sf_version().decode(), "scan_points": a.scan, "ref_points": a.ref,
           "sigma": a.sigma, "d_max": a.d_max, "iterations": a.iterations, "voxel": a.voxel, "repeats": a.repeats, "warmup": a.warmup,
           "calls": {}}
    for k in runs:
        tf = last[k][0]
        kern = kernels(one[k])
        sums_ms = kern.get("i1_icp_sums", {}).get("ms", 0.0)
        folds_ms = sum(v["ms"] for n, v in kern.items() if n in FOLDS)
        move_ms = kern.get("i0_transform", {}).get("ms", 0.0)
        res["calls"][k] = {
            "whole_call_host_to_host_ms_median": statistics.median(times[k]), "whole_call_ms_min": min(times[k]),
            "whole_call_ms_max": max(times[k]), "rotation_error": float(np.linalg.norm(tf.rotation - r0)),
            "translation_error": float(np.linalg.norm(tf.translation - t0)),
            "one_iteration_host_to_host_ms_median": statistics.median(one_times[k]), "one_iteration_ms_min": min(one_times[k]),
            "one_iteration_ms_max": max(one_times[k]), "one_iteration_pairs": last[k + "_pairs"],
            "one_iteration_kernels_ms_median": kern,
            "one_iteration_split_ms": {"transform": move_ms, "two_sums_passes": sums_ms, "two_folds": folds_ms,
                                       "search_and_the_rest": sum(v["ms"] for v in kern.values()) - sums_ms - folds_ms - move_ms},
        }
    b, c, d = (res["calls"][k] for k in ("b_point_to_plane", "c_generalized", "d_symmetric"))
    res["d_over_b_whole_call"] = d["whole_call_host_to_host_ms_median"] / b["whole_call_host_to_host_ms_median"]
    res["d_over_b_one_iteration"] = d["one_iteration_host_to_host_ms_median"] / b["one_iteration_host_to_host_ms_median"]
    res["two_sums_passes_us"] = {"b_point_to_plane": 1e3 * b["one_iteration_split_ms"]["two_sums_passes"],
                                 "c_generalized": 1e3 * c["one_iteration_split_ms"]["two_sums_passes"],
                                 "d_symmetric": 1e3 * d["one_iteration_split_ms"]["two_sums_passes"]}
    reg.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
