#!/usr/bin/env python3
"""Times of Unique Shape Context (K21) on a 1M-point cloud resident in HBM, next to the project's own kernels in the same
process: 100 000 keypoints (cloud points), R = 0.03, the default 14 x 14 x 10 bins, everything staying on the device.

  * the density-weights pass (sf_usc_weights at R / 5) beside sf_ball_counts at the same radius;
  * sf_usc (frames by K4, the weights into grid order, k_usc) beside sf_shot_single_scale on the same lists;
  * a device-to-device copy of as many bytes as the rows: what writing them costs at the least.

Kernel times come from HIP events around the named launches (Engine.profile), call and copy times from the host clock around
work that ends in a device synchronisation; every figure is the median of --repeats rounds after --warmup rounds.  Needs an
MI355X: without one the engine raises and nothing is printed.

    python tools/bench_usc.py [--n 1000000] [--keypoints 100000] [--radius 0.03] [--repeats 21] [--out profiles/usc_bench.json]
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


def profiled_rounds(engine, fn, repeats: int, warmup: int) -> list[dict]:
    """the per-name event times of `repeats` calls of fn()"""
    for _ in range(warmup):
        fn()
    engine.profile(True)
    out = []
    try:
        for _ in range(repeats):
            engine.profile_reset()
            fn()
            engine.sync()
            out.append({k: v[1] for k, v in engine.profile_report().items() if v[0]})
    finally:
        engine.profile(False)
    return out


def call_ms(engine, fn, repeats: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    engine.sync()
    vals = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        engine.sync()
        vals.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(vals)


def by_name(rounds: list[dict]) -> dict:
    return {name: statistics.median(r.get(name, 0.0) for r in rounds) for name in sorted(set().union(*rounds))}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--keypoints", type=int, default=100_000)
    ap.add_argument("--radius", type=float, default=0.03)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    rng = np.random.default_rng(7)
    p = rng.random((a.n, 3), dtype=np.float32).astype(np.float64)
    nr = rng.standard_normal((a.n, 3))
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    kp = p[np.sort(rng.choice(a.n, a.keypoints, replace=False))]
    R, L, K, J = a.radius, 14, 14, 10
    D = L * K * J
    res = {"tool": "tools/bench_usc.py", "library": engine.lib.sf_version().decode(), "repeats": a.repeats, "warmup": a.warmup,
           "n": a.n, "keypoints": a.keypoints, "radius": R, "density_radius": R / 5, "bins": [L, K, J], "row_bytes": 8 * D}
    cloud = engine.cloud(p, nr)
    weights, counts = engine.empty((a.n,)), engine.empty((a.n,), np.int32)
    rows, rows2, shot = engine.empty((a.keypoints, D)), engine.empty((a.keypoints, D)), engine.empty((a.keypoints, 352))
    try:
        # ---- the weights pass beside sf_ball_counts at the same radius (both rebuild nothing after their first round) ----
        rounds = profiled_rounds(engine, lambda: cloud.usc_weights(R / 5, out=weights), a.repeats, a.warmup)
        res["weights"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                          "call_ms": call_ms(engine, lambda: cloud.usc_weights(R / 5, out=weights), a.repeats, a.warmup)}
        lib, flags = engine.lib, s._ffi.SF_OUT_DEVICE
        ball = lambda: s._ffi.check(lib.sf_ball_counts(engine.h, cloud.h, R / 5, counts.ptr, flags), "sf_ball_counts")  # noqa: E731
        rounds = profiled_rounds(engine, ball, a.repeats, a.warmup)
        res["ball_counts"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                              "call_ms": call_ms(engine, ball, a.repeats, a.warmup)}
        res["weights_over_ball_counts"] = res["weights"]["kernels_ms"] / res["ball_counts"]["kernels_ms"]
        w_host = weights.to_host()
        res["mean_ball_at_density_radius"] = float((1.0 / w_host).mean())
        # ---- sf_usc beside sf_shot_single_scale on the same lists ----
        nb = cloud.radius_search(kp, R)
        try:
            res["mean_list"], res["longest_list"] = nb.total / max(nb.m, 1), int(nb.max_count)
            usc = lambda: nb.usc(weights, R / 10, out=rows)  # noqa: E731
            rounds = profiled_rounds(engine, usc, a.repeats, a.warmup)
            res["usc"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                          "k21_usc_ms": statistics.median(r["k21_usc"] for r in rounds), "call_ms": call_ms(engine, usc, a.repeats, a.warmup)}
            sh = lambda: nb.shot_single_scale(True, 10, out=shot)  # noqa: E731
            rounds = profiled_rounds(engine, sh, a.repeats, a.warmup)
            res["shot_single_scale"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                                        "call_ms": call_ms(engine, sh, a.repeats, a.warmup)}
            res["usc_over_shot_kernels"] = res["usc"]["kernels_ms"] / res["shot_single_scale"]["kernels_ms"]
        finally:
            nb.free()
        # ---- the floor: a device copy of the rows' bytes ----
        res["rows_bytes"] = rows.nbytes
        res["rows_copy_ms"] = call_ms(engine, lambda: rows2.copy_from_device(rows), a.repeats, a.warmup)
        res["k21_usc_over_rows_copy"] = res["usc"]["k21_usc_ms"] / res["rows_copy_ms"]
        res["k21_usc_row_store_GBps"] = rows.nbytes / (res["usc"]["k21_usc_ms"] * 1e-3) / 1e9
    finally:
        for d in (weights, counts, rows, rows2, shot):
            d.free()
        cloud.free()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
