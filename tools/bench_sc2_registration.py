#!/usr/bin/env python3
"""Times of SC2 registration (K15) on one MI355X, in one process, every figure the median of --repeats (>= 21) rounds after
--warmup rounds.  For each size m, on the sets of tools/bench_sc2.py (2 % true matches):
  (a) the chain sf_sc2_registration on resident matched points (host clock around the call: one wait), and the time of each of
      its kernels from HIP events around the named launches (Engine.profile) in rounds of their own;
  (b) the seed-row pass alone (sf_sc2_seed_rows + a synchronisation) at 64 and at --seeds seeds, and beside it the time ONE read
      of the m_pad^2 byte matrix would take at --hbm-bytes-per-s (no figure of this tool is a bandwidth measurement itself);
  (c) host to host, in turn inside every repeat: sc2_registration, and the pair of existing calls it stands beside,
      second_order_consistency_filter followed by fast_global_registration on what it keeps.
Needs an MI355X: without one the engine raises and nothing is printed.

    python tools/bench_sc2_registration.py [--sizes 5000 20000 32768] [--seeds 256] [--out profiles/sc2_registration_bench.json]
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
from bench_sc2 import median_ms  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 20000, 32768])
    ap.add_argument("--inlier-share", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--seeds", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-bytes-per-s", type=float, default=6.3e12,
                    help="the HBM read rate to set one read of C against: about 6.3 TB/s is what a streaming copy reaches on an "
                         "MI355X (8 TB/s specified); 0 leaves the comparison out")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    if a.repeats < 21:
        ap.error("--repeats must be at least 21")
    import shot_fpfh_amd as s
    from shot_fpfh_amd.matching import fast_global_registration, sc2_registration, second_order_consistency_filter

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    thr = a.threshold
    res = {"tool": "tools/bench_sc2_registration.py", "library": engine.lib.sf_version().decode(), "inlier_share": a.inlier_share,
           "threshold": thr, "n_seeds": a.seeds, "repeats": a.repeats, "warmup": a.warmup, "hbm_bytes_per_s": a.hbm_bytes_per_s,
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
        pad = engine.sc2_padded(m)
        held = [engine.empty((m, 3)), engine.empty((m, 3)), engine.empty((pad, pad), np.uint8), engine.empty((m,), np.uint32),
                engine.empty((a.seeds,), np.int32), engine.empty((a.seeds, pad), np.uint32)]
        da, db, cmat, ds2, dseeds, drows = held
        da.from_host(scan[si]), db.from_host(ref[ri])
        engine.consistency_matrix(da, db, m, thr, thr, out=cmat)
        ds2.from_host(engine.consistency_sc2(cmat, m))
        engine.sc2_seeds_device(ds2, m, a.seeds, dseeds)
        engine.sync()

        def chain():
            return engine.sc2_registration_device(da, db, m, thr, thr, a.seeds, 0.5)

        def rows_pass(n):
            engine.sc2_seed_rows_device(cmat, m, dseeds, n, drows)
            engine.sync()

        def filter_then_fgr():
            ks, kr, rec = second_order_consistency_filter(si, ri, scan, ref, distance_threshold=thr, engine=engine)
            return fast_global_registration(ks, kr, scan, ref, distance_threshold=thr, engine=engine)

        runs = {"sc2_registration": lambda: sc2_registration(si, ri, scan, ref, distance_threshold=thr, n_seeds=a.seeds, engine=engine),
                "second_order_consistency_filter + fast_global_registration": filter_then_fgr}
        few = min(64, a.seeds)
        for _ in range(a.warmup):
            chain(), rows_pass(few), rows_pass(a.seeds)
            for fn in runs.values():
                fn()
        row = {"matches": m, "padded": pad, "true": int(round(a.inlier_share * m)), "chain": median_ms(chain, a.repeats),
               f"seed_rows_{few}": median_ms(lambda: rows_pass(few), a.repeats),
               f"seed_rows_{a.seeds}": median_ms(lambda: rows_pass(a.seeds), a.repeats)}
        row["chain"]["kernels_ms_median"] = kernels(chain)
        row["chain"]["result"] = [int(x) for x in chain()[0]]
        for n in sorted({few, a.seeds}):
            entry = row[f"seed_rows_{n}"]
            entry["kernels_ms_median"] = kernels(lambda: rows_pass(n))
            ms = entry["kernels_ms_median"]["k15_seed_rows"]["ms"]
            entry["ops_per_s_kernel"] = 2.0 * n * pad * pad / (ms * 1e-3)
            entry["matrix_bytes_per_s_kernel"] = pad * pad / (ms * 1e-3)  # ONE read of C over the pass's time
            if a.hbm_bytes_per_s > 0:
                entry["one_read_of_c_ms_at_hbm_rate"] = pad * pad / a.hbm_bytes_per_s * 1e3
                entry["kernel_over_one_read"] = ms / entry["one_read_of_c_ms_at_hbm_rate"]
        times, last = {k: [] for k in runs}, {}
        for _ in range(a.repeats):  # in turn: what the box does meanwhile falls on both alike
            for k, fn in runs.items():
                t = time.perf_counter()
                last[k] = fn()
                times[k].append((time.perf_counter() - t) * 1e3)
        row["host_to_host"] = {}
        for k in runs:
            ratio, tf = last[k][0], last[k][1]
            row["host_to_host"][k] = {"ms_median": statistics.median(times[k]), "ms_min": min(times[k]), "ms_max": max(times[k]),
                                      "inlier_ratio": float(ratio), "rotation_error": float(np.linalg.norm(tf.rotation - r0)),
                                      "translation_error": float(np.linalg.norm(tf.translation - t0))}
        res["sizes"].append(row)
        for d in held:
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
