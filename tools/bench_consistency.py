#!/usr/bin/env python3
"""Times of the geometric-consistency filter (K13) on one MI355X, in one process, every figure the median of --repeats (>= 20)
rounds of the host clock around calls that end in a device synchronisation, after --warmup rounds.  For each size m (30 % true
matches), on matched points already resident:
  (a) the degree pass alone (sf_consistency_degree + a synchronisation), in ms and pairs per second (m^2 ordered pairs), and as
      a share of the FP64 vector peak from the FP64 instructions the compiler's listing shows per pair;
  (b) the whole chain (sf_consistency_group: degree, arg-max, mark, count, masked degree; one wait);
host to host: (c) geometric_consistency_filter, and beside it ransac_prerejective and fast_global_registration on all matches and
on the kept ones, the calls in turn inside every repeat.  Kernel times come from HIP events around the named launches
(Engine.profile) in rounds of their own.  Needs an MI355X: without one the engine raises and nothing is printed.

    python tools/bench_consistency.py [--sizes 5000 20000 100000] [--repeats 21] [--warmup 3] [--out profiles/consistency_bench.json]
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

from bench_ransac import synthetic_matches  # noqa: E402

# One pair of the inner loop of k13_degree, from `hipcc -S` of csrc/consistency.hip (the loop is unrolled four times: 192 FP64
# instructions for 4 pairs): 6 subtractions, 6 multiplications, 4 additions, two square roots of 15 each (v_rsq_f64, two
# v_ldexp_f64, 9 fused steps of the refinement, a scale test and a class test), dp - dq and three compares.
FP64_INSTRUCTIONS_PER_PAIR = 48
# FP64 vector instructions per second of the chip: 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz (78.6 TFLOP/s counts an FMA twice)
FP64_LANE_INSTRUCTIONS_PER_S = 256 * 4 * 16 * 2.4e9


def median_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 20000, 100000])
    ap.add_argument("--inlier-share", type=float, default=0.3)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--draws", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd import _ffi
    from shot_fpfh_amd.matching import fast_global_registration, geometric_consistency_filter, ransac_prerejective

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    thr = a.threshold
    res = {"tool": "tools/bench_consistency.py", "library": engine.lib.sf_version().decode(), "inlier_share": a.inlier_share,
           "threshold": thr, "repeats": a.repeats, "warmup": a.warmup, "fp64_instructions_per_pair": FP64_INSTRUCTIONS_PER_PAIR,
           "sizes": []}

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

    for m in a.sizes:
        scan, ref, si, ri, r0, t0 = synthetic_matches(m, a.inlier_share)
        da, db = engine.empty((m, 3)), engine.empty((m, 3))
        ddeg, dmem, dgdeg = engine.empty((m,), np.uint32), engine.empty((m,), np.uint8), engine.empty((m,), np.uint32)
        da.from_host(scan[si]), db.from_host(ref[ri])

        def degree_pass():
            _ffi.check(engine.lib.sf_consistency_degree(engine.h, da.ptr, db.ptr, m, None, thr, thr, ddeg.ptr), "sf_consistency_degree")
            engine.sync()

        chain = lambda: engine.consistency_group_device(da, db, m, thr, thr, ddeg, dmem, dgdeg)  # noqa: E731
        kept_s, kept_r, rec = geometric_consistency_filter(si, ri, scan, ref, distance_threshold=thr, engine=engine)
        runs = {
            "geometric_consistency_filter": lambda: geometric_consistency_filter(si, ri, scan, ref, distance_threshold=thr, engine=engine),
            "ransac_prerejective_all": lambda: ransac_prerejective(si, ri, scan, ref, n_draws=a.draws, distance_threshold=thr, engine=engine),
            "fast_global_registration_all": lambda: fast_global_registration(si, ri, scan, ref, distance_threshold=thr, engine=engine),
            "ransac_prerejective_kept": lambda: ransac_prerejective(kept_s, kept_r, scan, ref, n_draws=a.draws, distance_threshold=thr,
                                                                    engine=engine),
            "fast_global_registration_kept": lambda: fast_global_registration(kept_s, kept_r, scan, ref, distance_threshold=thr,
                                                                              engine=engine),
        }
        for _ in range(a.warmup):
            degree_pass(), chain()
            for fn in runs.values():
                fn()
        row = {"matches": m, "pairs": m * m, "true": int(round(a.inlier_share * m)), "kept": int(kept_s.shape[0]),
               "group_size": rec.group_size, "degree_pass": median_ms(degree_pass, a.repeats), "chain": median_ms(chain, a.repeats)}
        times, last = {k: [] for k in runs}, {}
        for _ in range(a.repeats):  # in turn: what the box does meanwhile falls on all of them alike
            for k, fn in runs.items():
                t = time.perf_counter()
                last[k] = fn()
                times[k].append((time.perf_counter() - t) * 1e3)
        row["degree_pass"]["kernels_ms_median"] = kernels(degree_pass)
        row["chain"]["kernels_ms_median"] = kernels(chain)
        k_ms = row["degree_pass"]["kernels_ms_median"]["k13_degree"]["ms"]
        for key, ms in (("host_clock", row["degree_pass"]["ms_median"]), ("kernel", k_ms)):
            rate = m * m / (ms * 1e-3)
            row["degree_pass"][f"pairs_per_s_{key}"] = rate
            row["degree_pass"][f"share_of_fp64_vector_peak_{key}"] = rate * FP64_INSTRUCTIONS_PER_PAIR / FP64_LANE_INSTRUCTIONS_PER_S
        row["host_to_host"] = {}
        for k in runs:
            entry = {"ms_median": statistics.median(times[k]), "ms_min": min(times[k]), "ms_max": max(times[k])}
            if k != "geometric_consistency_filter":
                entry["rotation_error"] = float(np.linalg.norm(last[k][1].rotation - r0))
                entry["translation_error"] = float(np.linalg.norm(last[k][1].translation - t0))
            row["host_to_host"][k] = entry
        res["sizes"].append(row)
        for d in (da, db, ddeg, dmem, dgdeg):
            d.free()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
