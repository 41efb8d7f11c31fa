#!/usr/bin/env python3
"""Times of Point Feature Histograms (K22) on a 1M-point cloud resident in HBM, next to the project's other descriptors in the
same process on the same keypoints: 100 000 keypoints (cloud points), R = 0.03 (about 110 entries per list), 5 bins, everything
staying on the device.

  * sf_pfh (k_pfh) on the keypoints' lists: its time, and pairs per second;
  * beside it the FPFH chain (self search of the whole cloud + K6 + K7), sf_shot_single_scale and sf_usc on those keypoints;
  * k_pfh's distance from its own issue floor: the float64 vector instructions of one round of 64 pairs (--f64-per-pair,
    counted from the build's ISA listing) x rounds x 4 cycles over the chip's 1024 SIMDs at --clock-ghz;
  * one run at --long-radius (about 496 entries per ball) on fewer keypoints: the lists the streaming form serves.

Kernel times come from HIP events around the named launches (Engine.profile), chain times from the host clock around work that
ends in a device synchronisation; every figure is the median of --repeats rounds after --warmup rounds.  Needs an MI355X: without
one the engine raises and nothing is printed.

    python tools/bench_pfh.py [--n 1000000] [--keypoints 100000] [--radius 0.03] [--repeats 21] [--out profiles/pfh_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_usc import by_name, call_ms, profiled_rounds  # noqa: E402

SIMDS = 256 * 4  # of the chip


def pfh_figures(engine, nb, rows, S, a) -> dict:
    k = nb.counts().astype(np.int64)
    pairs = int((k * (k - 1) // 2).sum())
    rounds64 = int(((k * (k - 1) // 2 + 63) // 64).sum())  # a lower bound of the rounds: every lane at work
    run = lambda: nb.pfh(S, out=rows)  # noqa: E731
    rounds = profiled_rounds(engine, run, a.repeats, a.warmup)
    ms = statistics.median(r["k22_pfh"] for r in rounds)
    floor_ms = a.f64_per_pair * (pairs / 64.0) * 4.0 / (SIMDS * a.clock_ghz * 1e9) * 1e3
    return {"mean_list": float(k.mean()), "longest_list": int(k.max()), "lists_over_128": int((k > 128).sum()), "pairs": pairs,
            "rounds_of_64_at_least": rounds64, "k22_pfh_ms": ms, "pairs_per_second": pairs / (ms * 1e-3),
            "ns_per_pair_per_simd": ms * 1e6 * SIMDS / pairs, "call_ms": call_ms(engine, run, a.repeats, a.warmup),
            "f64_vector_instructions_per_pair": a.f64_per_pair, "clock_ghz_assumed": a.clock_ghz, "issue_floor_ms": floor_ms,
            "k22_pfh_over_issue_floor": ms / floor_ms}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--keypoints", type=int, default=100_000)
    ap.add_argument("--radius", type=float, default=0.03)
    ap.add_argument("--long-radius", type=float, default=0.0491, help="about 496 entries per ball at 1M points")
    ap.add_argument("--long-keypoints", type=int, default=30_000)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--f64-per-pair", type=float, default=119.0,
                    help="float64 vector instructions of one round of k_pfh<5> (csrc/pfh.hip's ISA listing: v_*_f64 in the round loop)")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock the floor is computed at (the chip's maximum: the "
                    "sustained clock is not measured here, so the floor is a lower bound and the ratio an upper bound)")
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
    kp_idx = np.sort(rng.choice(a.n, a.keypoints, replace=False))
    kp = p[kp_idx]
    R, S = a.radius, a.bins
    res = {"tool": "tools/bench_pfh.py", "library": engine.lib.sf_version().decode(), "repeats": a.repeats, "warmup": a.warmup,
           "n": a.n, "keypoints": a.keypoints, "radius": R, "bins": S, "row_bytes": 8 * S ** 3}
    cloud = engine.cloud(p, nr)
    weights = engine.empty((a.n,))
    rows, fpfh_rows = engine.empty((a.keypoints, S ** 3)), engine.empty((a.keypoints, 125))
    shot, usc = engine.empty((a.keypoints, 352)), engine.empty((a.keypoints, 1960))
    try:
        cloud.usc_weights(R / 5, out=weights)  # (first: it rebuilds the grid)
        nb = cloud.radius_search(kp, R)
        try:
            res["pfh"] = pfh_figures(engine, nb, rows, S, a)
            sh = lambda: nb.shot_single_scale(True, 10, out=shot)  # noqa: E731
            rounds = profiled_rounds(engine, sh, a.repeats, a.warmup)
            res["shot_single_scale"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds)}
            us = lambda: nb.usc(weights, R / 10, out=usc)  # noqa: E731
            rounds = profiled_rounds(engine, us, a.repeats, a.warmup)
            res["usc"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                          "k21_usc_ms": statistics.median(r["k21_usc"] for r in rounds)}
        finally:
            nb.free()

        # ---- the FPFH chain: the whole cloud's self search, K6 on every point, K7 for the keypoints ----
        def fpfh_chain():
            self_nb = cloud.radius_search_self(R)
            try:
                table = engine.spfh(cloud, 5, self_nb.max_count, R)
                try:
                    table.compute(self_nb)
                    table.fpfh(self_nb, kp_idx, out=fpfh_rows)
                finally:
                    table.free()
            finally:
                self_nb.free()

        rounds = profiled_rounds(engine, fpfh_chain, a.repeats, a.warmup)
        res["fpfh_chain"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                             "call_ms": call_ms(engine, fpfh_chain, a.repeats, a.warmup)}
        res["k22_pfh_over_fpfh_chain_kernels"] = res["pfh"]["k22_pfh_ms"] / res["fpfh_chain"]["kernels_ms"]
        res["k22_pfh_over_shot_kernels"] = res["pfh"]["k22_pfh_ms"] / res["shot_single_scale"]["kernels_ms"]
        res["k22_pfh_over_k21_usc"] = res["pfh"]["k22_pfh_ms"] / res["usc"]["k21_usc_ms"]

        # ---- long lists: the streaming form ----
        m_long = min(a.long_keypoints, a.keypoints)
        nb = cloud.radius_search(kp[:: max(a.keypoints // m_long, 1)][:m_long], a.long_radius)
        try:
            res["pfh_long_lists"] = dict(radius=a.long_radius, keypoints=nb.m, **pfh_figures(engine, nb, rows, S, a))
        finally:
            nb.free()
        res["ns_per_pair_long_over_short"] = res["pfh_long_lists"]["ns_per_pair_per_simd"] / res["pfh"]["ns_per_pair_per_simd"]
    finally:
        for d in (weights, rows, fpfh_rows, shot, usc):
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
