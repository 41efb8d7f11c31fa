#!/usr/bin/env python3
"""What trimming costs per ICP iteration on one MI355X, in one process: a 10^5-point scan against a 10^6-point reference, the
setting of tools/bench_icp_robust.py (two independent samplings of the corner surface of tests/gicp_numpy.py, normals computed
once).  ONE iteration's device call on resident clouds, host to host: for every mode the plain entry point, sf_icp_accumulate_robust
without a loss (the untrimmed call of the same mode) and sf_icp_accumulate_trimmed at --trim (0.8) without a loss and with Cauchy --
all of them in turn inside every round, after --warmup rounds, every figure the median of --repeats (21) rounds of the host clock
around calls that end in a device synchronisation.  Then the kernels of one call from HIP events around the named launches
(Engine.profile), in rounds of their own: the device time per iteration and what the key pass and the selection add to it.
Last, sf_select_kth alone at n = 10^5, 10^6 and 10^7 random keys against ONE read of the keys at the copy rate measured in the
same process (a device-to-device copy of the keys moves 2 x 8 n bytes: one read takes half its time).  Needs an MI355X: without
one the engine raises and nothing is printed.

    python tools/bench_icp_trimmed.py [--scan 100000] [--ref 1000000] [--trim 0.8] [--repeats 21] [--warmup 3] [--out profiles/icp_trimmed_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
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

CHAIN = ("i0_transform", "i1_icp_sums", "i1_icp_means", "i1_icp_final")
TRIM = ("i2_icp_keys", "i2_select_hist", "i2_select_final")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scan", type=int, default=100_000)
    ap.add_argument("--ref", type=int, default=1_000_000)
    ap.add_argument("--sigma", type=float, default=0.002)
    ap.add_argument("--d-max", type=float, default=0.15)
    ap.add_argument("--trim", type=float, default=0.8)
    ap.add_argument("--scale", type=float, default=0.006, help="of the loss, as a length (3 sigma); mode 2 divides it by sqrt(2 epsilon)")
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--select-sizes", type=int, nargs="*", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd import _ffi, icp
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
    none, cauchy = icp.LOSSES["none"], icp.LOSSES["cauchy"]
    calls = {}
    for name, mode in modes.items():
        k = a.scale / math.sqrt(2 * eps) if mode == icp._GICP else a.scale
        calls[(name, "plain")] = lambda mode=mode: reg.pairs(mode, a.d_max, moved_by=at, epsilon=eps)
        calls[(name, "untrimmed")] = lambda mode=mode: reg.pairs(mode, a.d_max, moved_by=at, epsilon=eps, loss=none)
        calls[(name, "trimmed")] = lambda mode=mode: reg.pairs(mode, a.d_max, moved_by=at, epsilon=eps, loss=none, trim=a.trim)
        calls[(name, "trimmed_cauchy")] = lambda mode=mode, k=k: reg.pairs(mode, a.d_max, moved_by=at, epsilon=eps, loss=cauchy, scale=k,
                                                                            trim=a.trim)
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

    res = {"tool": "tools/bench_icp_trimmed.py", "library": engine.lib.sf_version().decode(), "scan_points": a.scan, "ref_points": a.ref,
           "sigma": a.sigma, "d_max": a.d_max, "trim": a.trim, "scale": a.scale, "epsilon": eps, "repeats": a.repeats, "warmup": a.warmup,
           "modes": {}, "select_kth": {}}
    entry = {"plain": "plain", "untrimmed": "sf_icp_accumulate_robust", "trimmed": "sf_icp_accumulate_trimmed",
             "trimmed_cauchy": "sf_icp_accumulate_trimmed"}
    for name in modes:
        rows = {}
        for (mode_name, which), fn in calls.items():
            if mode_name != name:
                continue
            kern = kernels(fn)
            med = statistics.median(times[(name, which)])
            f = found[(name, which)]
            rows[which] = {"entry_point": entry[which], "one_iteration_host_to_host_ms_median": med,
                           "one_iteration_ms_min": min(times[(name, which)]), "one_iteration_ms_max": max(times[(name, which)]),
                           "pairs_used": f.count, "pairs_inside_d_max": f.inside if which.startswith("trimmed") else f.count,
                           "rank": f.rank if which.startswith("trimmed") else None, "cut": f.cut if which.startswith("trimmed") else None,
                           "device_ms_all_kernels": sum(v["ms"] for v in kern.values()),
                           "device_ms_chain_kernels": sum(v["ms"] for n, v in kern.items() if n in CHAIN),
                           "device_ms_key_pass_and_selection": sum(v["ms"] for n, v in kern.items() if n in TRIM),
                           "kernels": kern}
        for which, row in rows.items():
            row["host_to_host_ratio_to_untrimmed"] = row["one_iteration_host_to_host_ms_median"] / rows["untrimmed"]["one_iteration_host_to_host_ms_median"]
            row["device_ratio_to_untrimmed"] = row["device_ms_all_kernels"] / rows["untrimmed"]["device_ms_all_kernels"]
        res["modes"][name] = rows
    reg.close()

    # ---- the selection alone
    out = np.zeros(4)
    for n in a.select_sizes:
        keys = np.random.default_rng(n).random(n)
        dev, other = engine.empty((n,)).from_host(keys), engine.empty((n,))
        rank = (n + 1) // 2

        def select():
            _ffi.check(engine.lib.sf_select_kth(engine.h, dev.ptr, n, rank, out.ctypes.data_as(C.c_void_p)), "sf_select_kth")

        def copy():
            other.copy_from_device(dev)
            engine.sync()

        for _ in range(a.warmup):
            select(), copy()
        ts, tc = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            select()
            ts.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            copy()
            tc.append((time.perf_counter() - t) * 1e3)
        kern = kernels(select)
        assert out[0] == np.partition(keys, rank - 1)[rank - 1]
        copy_ms = statistics.median(tc)
        device_ms = sum(v["ms"] for v in kern.values())
        one_read_ms = 0.5 * copy_ms
        res["select_kth"][str(n)] = {"rank": rank, "host_to_host_ms_median": statistics.median(ts), "device_ms_all_kernels": device_ms,
                                     "kernels": kern, "copy_host_to_host_ms_median": copy_ms,
                                     "copy_rate_GB_per_s": 2 * 8 * n / (copy_ms * 1e-3) / 1e9, "one_read_of_the_keys_ms": one_read_ms,
                                     "device_time_in_reads_of_the_keys": device_ms / one_read_ms,
                                     "host_to_host_in_reads_of_the_keys": statistics.median(ts) / one_read_ms}
        dev.free(), other.free()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
