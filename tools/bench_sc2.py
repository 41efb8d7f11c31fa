#!/usr/bin/env python3
"""Times of the second-order consistency filter (K14) on one MI355X, in one process, every figure the median of --repeats (>= 21)
rounds of the host clock around calls that end in a device synchronisation, after --warmup rounds.  For each size m, on matched
points already resident:
  (a) the matrix pass alone (sf_consistency_matrix + a synchronisation), in ms and pairs per second;
  (b) the sc2 pass alone (sf_consistency_sc2 + a synchronisation), in ms and as a share of the 3.8 Pop/s that
      tools/ubench/mfma_rates.hip measured for v_mfma_i32_32x32x32_i8 -- twice: for the 2 m_pad^3 integer operations of the
      product C C^T (what a caller gets), and for the operations the matrix cores really execute, the tiles J >= I only
      (what the kernel sustains);
  (c) the whole chain (sf_consistency_sc2_group: matrix, sc2, arg-max, mark, count, masked degree; one wait);
  (d) the density of the compatibility matrix (from K13's degree: the same integers), for a later decision on a sparse form;
host to host: (e) second_order_consistency_filter beside geometric_consistency_filter, in turn inside every repeat.  Kernel
times come from HIP events around the named launches (Engine.profile) in rounds of their own.  Needs an MI355X: without one the
engine raises and nothing is printed.

    python tools/bench_sc2.py [--sizes 5000 20000 32768] [--repeats 21] [--warmup 3] [--out profiles/sc2_bench.json]
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

I8_OPS_PER_S_MEASURED = 3.8e15  # tools/ubench/mfma_rates.hip, v_mfma_i32_32x32x32_i8 on random operands (csrc/match_i8.hip)


def median_ms(fn, repeats):
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 20000, 32768])
    ap.add_argument("--inlier-share", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    if a.repeats < 21:
        ap.error("--repeats must be at least 21")
    import shot_fpfh_amd as s
    from shot_fpfh_amd import _ffi
    from shot_fpfh_amd.matching import geometric_consistency_filter, second_order_consistency_filter

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    thr = a.threshold
    res = {"tool": "tools/bench_sc2.py", "library": engine.lib.sf_version().decode(), "inlier_share": a.inlier_share,
           "threshold": thr, "repeats": a.repeats, "warmup": a.warmup, "i8_ops_per_s_measured": I8_OPS_PER_S_MEASURED, "sizes": []}

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
        pad = engine.sc2_padded(m)
        tiles = pad // engine.SC2_TILE
        da, db = engine.empty((m, 3)), engine.empty((m, 3))
        ds2, dmem, dgdeg = engine.empty((m,), np.uint32), engine.empty((m,), np.uint8), engine.empty((m,), np.uint32)
        cmat = engine.empty((pad, pad), np.uint8)
        da.from_host(scan[si]), db.from_host(ref[ri])

        def matrix_pass():
            engine.consistency_matrix(da, db, m, thr, thr, out=cmat)
            engine.sync()

        def sc2_pass():
            _ffi.check(engine.lib.sf_consistency_sc2(engine.h, cmat.ptr, m, ds2.ptr), "sf_consistency_sc2")
            engine.sync()

        chain = lambda: engine.consistency_sc2_group_device(da, db, m, thr, thr, ds2, dmem, dgdeg)  # noqa: E731
        runs = {
            "second_order_consistency_filter": lambda: second_order_consistency_filter(si, ri, scan, ref, distance_threshold=thr, engine=engine),
            "geometric_consistency_filter": lambda: geometric_consistency_filter(si, ri, scan, ref, distance_threshold=thr, engine=engine),
        }
        for _ in range(a.warmup):
            matrix_pass(), sc2_pass(), chain()
            for fn in runs.values():
                fn()
        degree = engine.consistency_degree(da, db, m, thr, thr)
        row = {"matches": m, "padded": pad, "true": int(round(a.inlier_share * m)),
               "density": float(degree.sum(dtype=np.int64)) / float(m * m),
               "matrix_pass": median_ms(matrix_pass, a.repeats), "sc2_pass": median_ms(sc2_pass, a.repeats),
               "chain": median_ms(chain, a.repeats)}
        times, last = {k: [] for k in runs}, {}
        for _ in range(a.repeats):  # in turn: what the box does meanwhile falls on both alike
            for k, fn in runs.items():
                t = time.perf_counter()
                last[k] = fn()
                times[k].append((time.perf_counter() - t) * 1e3)
        row["matrix_pass"]["kernels_ms_median"] = kernels(matrix_pass)
        row["sc2_pass"]["kernels_ms_median"] = kernels(sc2_pass)
        row["chain"]["kernels_ms_median"] = kernels(chain)
        row["matrix_pass"]["pairs_per_s_host_clock"] = m * m / (row["matrix_pass"]["ms_median"] * 1e-3)
        for key, ms in (("host_clock", row["sc2_pass"]["ms_median"]), ("kernel", row["sc2_pass"]["kernels_ms_median"]["k14_sc2"]["ms"])):
            rate = 2.0 * pad ** 3 / (ms * 1e-3)
            executed = rate * (tiles * (tiles + 1) // 2) / (tiles * tiles)
            row["sc2_pass"][f"ops_per_s_{key}"] = rate
            row["sc2_pass"][f"share_of_measured_i8_rate_{key}"] = rate / I8_OPS_PER_S_MEASURED
            row["sc2_pass"][f"executed_ops_per_s_{key}"] = executed
            row["sc2_pass"][f"executed_share_of_measured_i8_rate_{key}"] = executed / I8_OPS_PER_S_MEASURED
        row["host_to_host"] = {}
        for k in runs:
            row["host_to_host"][k] = {"ms_median": statistics.median(times[k]), "ms_min": min(times[k]), "ms_max": max(times[k]),
                                      "kept": int(last[k][0].shape[0]), "group_size": int(last[k][2].group_size)}
        res["sizes"].append(row)
        for d in (da, db, ds2, dmem, dgdeg, cmat):
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
