#!/usr/bin/env python3
"""What a robust loss costs per ICP iteration on one MI355X, in one process: a 10^5-point scan against a 10^6-point reference, the
setting of tools/bench_gicp.py (two independent samplings of the corner surface of tests/gicp_numpy.py, normals computed once).
ONE iteration's device call on resident clouds, host to host: for every mode, loss none through the plain entry point
(sf_icp_accumulate / sf_icp_accumulate_gicp) and every loss, none included, through sf_icp_accumulate_robust -- all of them in turn
inside every round, after --warmup rounds, every figure the median of --repeats (21) rounds of the host clock around calls that
end in a device synchronisation.  Then the sums kernels alone, from HIP events around the named launches (Engine.profile), in
rounds of their own.  Every robust figure is also given as its ratio to the same process's call without a loss.  Needs an
MI355X: without one the engine raises and nothing is printed.

    python tools/bench_icp_robust.py [--scan 100000] [--ref 1000000] [--repeats 21] [--warmup 3] [--out profiles/icp_robust_bench.json]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gicp_numpy as G  # noqa: E402 -- the surface and the true motion of the parity table

SUMS = ("i1_icp_sums", "i1_icp_means", "i1_icp_final")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scan", type=int, default=100_000)
    ap.add_argument("--ref", type=int, default=1_000_000)
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--d-max", type=float, default=0.15)
    ap.add_argument("--scale", type=float, default=0.006, help="of the loss, as a length (3 sigma); mode 2 divides it by sqrt(2 epsilon)")
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd import icp
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.engine import default_engine

    engine = default_engine()  # raises without a GPU: no figure is ever printed from a CPU
    rng = np.random.default_rng(16)
    ref = G.corner_surface(a.ref, rng, a.sigma)
    r0, t0 = G.true_motion()
    scan = (G.corner_surface(a.scan, rng, a.sigma) - t0) @ r0
    scan_normals, ref_normals = s.compute_normals(scan, scan, k=20), s.compute_normals(ref, ref, k=20)
    reg = icp._Registration(scan, ref, ref_normals, engine=engine, scan_normals=scan_normals)
    at = RigidTransform(r0, t0)
    eps = 1e-3
    modes = {"point_to_point": icp._POINT, "point_to_plane": icp._PLANE, "generalized": icp._GICP}
    calls = {}
    for name, mode in modes.items():
        k = a.scale / math.sqrt(2 * eps) if mode == icp._GICP else a.scale
        calls[(name, "plain")] = lambda mode=mode: reg.pairs(mode, a.d_max, moved_by=at, epsilon=eps)
        for loss_name, loss in icp.LOSSES.items():
            calls[(name, loss_name)] = lambda mode=mode, loss=loss, k=k: reg.pairs(mode, a.d_max, moved_by=at, epsilon=eps, loss=loss, scale=k)
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    times, found = {key: [] for key in calls}, {}
    for _ in range(a.repeats):  # in turn: what the machine does meanwhile falls on all of them alike
        for key, fn in calls.items():
            t = time.perf_counter()
            found[key] = fn()
            times[key].append((time.perf_counter() - t) * 1e3)

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

    res = {"tool": "tools/bench_icp_robust.py", "library": engine.lib.sf_version().decode(), "scan_points": a.scan, "ref_points": a.ref,
           "sigma": a.sigma, "d_max": a.d_max, "scale": a.scale, "epsilon": eps, "repeats": a.repeats, "warmup": a.warmup, "modes": {}}
    for name in modes:
        base = statistics.median(times[(name, "plain")])
        rows = {}
        for (mode_name, which), fn in calls.items():
            if mode_name != name:
                continue
            kern = kernels(fn)
            sums_ms = sum(v["ms"] for n, v in kern.items() if n in SUMS)
            med = statistics.median(times[(name, which)])
            rows[which] = {"entry_point": "plain" if which == "plain" else "sf_icp_accumulate_robust",
                           "one_iteration_host_to_host_ms_median": med, "one_iteration_ms_min": min(times[(name, which)]),
                           "one_iteration_ms_max": max(times[(name, which)]), "ratio_to_plain_call": med / base,
                           "pairs": found[(name, which)].count,
                           "sum_w": float(found[(name, which)].raw[7]) if which != "plain" else None,
                           "sums_kernels_ms": sums_ms,
                           "sums_kernels": {n: v for n, v in kern.items() if n in SUMS}}
        for which, row in rows.items():
            row["sums_kernels_ratio_to_plain"] = row["sums_kernels_ms"] / rows["plain"]["sums_kernels_ms"]
        res["modes"][name] = rows
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
