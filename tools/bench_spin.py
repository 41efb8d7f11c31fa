#!/usr/bin/env python3
"""Times of spin images (K24) on a 1M-point cloud resident in HBM, next to the project's own kernels on the same lists in the
same process: 100 000 keypoints (cloud points), image width 8, everything staying on the device.  Two clouds:

  * uniform: the unit cube, R = 0.03 (about 110 entries per list), random unit normals as axes -- the entries spread over the image;
  * sphere: a noisy sphere of radius 0.5 (noise --sphere-noise of the radius), outward normals as axes, --sphere-radius chosen for
    about as many entries per list -- the entries sit near beta = 0 and their adds pile onto few nodes: the LDS-atomic contention
    shows here if anywhere.

Per cloud: k_spin (signed and unsigned image) beside sf_shot_single_scale and k_usc on those lists; a device-to-device copy of as
many bytes as the rows (what writing them costs at the least); k_spin's float64 issue floor, --f64-per-entry float64 vector
instructions (counted from the build's ISA listing: the list walk of csrc/spin.hip, two entries per lane and step) x entries / 64 x
4 cycles over the chip's 1024 SIMDs at --clock-ghz.

Kernel times come from HIP events around the named launches (Engine.profile), copy times from the host clock around work that ends
in a device synchronisation; every figure is the median of --repeats rounds after --warmup rounds.  Needs an MI355X: without one the
engine raises and nothing is printed.

    python tools/bench_spin.py [--n 1000000] [--keypoints 100000] [--radius 0.03] [--repeats 21] [--out profiles/spin_bench.json]
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


def one_cloud(engine, p, nr, kp_idx, R, W, a) -> dict:
    m = kp_idx.shape[0]
    D_signed, D_unsigned = (W + 1) * (2 * W + 1), (W + 1) * (W + 1)
    res = {"radius": R}
    cloud = engine.cloud(p, nr)
    weights = engine.empty((p.shape[0],))
    rows, rows2 = engine.empty((m, D_signed)), engine.empty((m, D_signed))
    axes, shot, usc = engine.empty((m, 3)), engine.empty((m, 352)), engine.empty((m, 1960))
    try:
        axes.from_host(nr[kp_idx])
        cloud.usc_weights(R / 5, out=weights)  # (first: it rebuilds the grid)
        nb = cloud.radius_search(p[kp_idx], R)
        try:
            k = nb.counts().astype(np.int64)
            entries = int(k.sum())
            res.update(mean_list=float(k.mean()), longest_list=int(k.max()), entries=entries)
            for name, signed in (("spin_signed", True), ("spin_unsigned", False)):
                run = lambda: nb.spin_images(axes, W, signed_beta=signed, out=rows)  # noqa: E731
                rounds = profiled_rounds(engine, run, a.repeats, a.warmup)
                ms = statistics.median(r["k24_spin"] for r in rounds)
                _, contrib = nb.spin_images(axes, W, signed_beta=signed, out=rows, return_counts=True)
                res[name] = {"row_bytes": 8 * (D_signed if signed else D_unsigned), "k24_spin_ms": ms,
                             "call_ms": call_ms(engine, run, a.repeats, a.warmup), "mean_contributing": float(contrib.mean()),
                             "ns_per_entry_per_simd": ms * 1e6 * SIMDS / entries}
            floor_ms = a.f64_per_entry * (entries / 64.0) * 4.0 / (SIMDS * a.clock_ghz * 1e9) * 1e3
            res["f64_vector_instructions_per_entry"] = a.f64_per_entry
            res["clock_ghz_assumed"] = a.clock_ghz
            res["issue_floor_ms"] = floor_ms
            res["k24_spin_over_issue_floor"] = res["spin_signed"]["k24_spin_ms"] / floor_ms
            sh = lambda: nb.shot_single_scale(True, 10, out=shot)  # noqa: E731
            rounds = profiled_rounds(engine, sh, a.repeats, a.warmup)
            res["shot_single_scale"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds)}
            us = lambda: nb.usc(weights, R / 10, out=usc)  # noqa: E731
            rounds = profiled_rounds(engine, us, a.repeats, a.warmup)
            res["usc"] = {"launches_ms": by_name(rounds), "kernels_ms": statistics.median(sum(r.values()) for r in rounds),
                          "k21_usc_ms": statistics.median(r["k21_usc"] for r in rounds)}
        finally:
            nb.free()
        # ---- the row-write floor: a device copy of the rows' bytes ----
        res["rows_bytes"] = rows.nbytes
        res["rows_copy_ms"] = call_ms(engine, lambda: rows2.copy_from_device(rows), a.repeats, a.warmup)
        ms = res["spin_signed"]["k24_spin_ms"]
        res["k24_spin_over_rows_copy"] = ms / res["rows_copy_ms"]
        res["k24_spin_over_shot_kernels"] = ms / res["shot_single_scale"]["kernels_ms"]
        res["k24_spin_over_k21_usc"] = ms / res["usc"]["k21_usc_ms"]
    finally:
        for d in (weights, rows, rows2, axes, shot, usc):
            d.free()
        cloud.free()
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--keypoints", type=int, default=100_000)
    ap.add_argument("--radius", type=float, default=0.03)
    ap.add_argument("--sphere-radius", type=float, default=0.0105, help="about 110 entries per list on the sphere at 1M points")
    ap.add_argument("--sphere-noise", type=float, default=0.001, help="standard deviation of the radial noise, as a share of the radius")
    ap.add_argument("--width", type=int, default=8)
    ap.add_argument("--f64-per-entry", type=float, default=46.0,
                    help="float64 vector instructions per list entry of k_spin without the support angle (csrc/spin.hip's ISA "
                         "listing: 104 v_*_f64 in the list walk of two entries per lane and step, 12 of them the support angle's)")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the clock the floor is computed at (the chip's maximum: the "
                    "sustained clock is not measured here, so the floor is a lower bound and the ratio an upper bound)")
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    rng = np.random.default_rng(7)
    res = {"tool": "tools/bench_spin.py", "library": engine.lib.sf_version().decode(), "repeats": a.repeats, "warmup": a.warmup,
           "n": a.n, "keypoints": a.keypoints, "image_width": a.width}
    kp_idx = np.sort(rng.choice(a.n, a.keypoints, replace=False))
    p = rng.random((a.n, 3), dtype=np.float32).astype(np.float64)
    nr = rng.standard_normal((a.n, 3))
    nr /= np.linalg.norm(nr, axis=1)[:, None]
    res["uniform"] = one_cloud(engine, p, nr, kp_idx, a.radius, a.width, a)
    d = rng.standard_normal((a.n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = (0.5 + 0.5 * d * (1.0 + a.sphere_noise * rng.standard_normal((a.n, 1)))).astype(np.float32).astype(np.float64)
    res["sphere"] = dict(noise=a.sphere_noise, **one_cloud(engine, p, d, kp_idx, a.sphere_radius, a.width, a))
    res["sphere_over_uniform_ns_per_entry"] = (res["sphere"]["spin_signed"]["ns_per_entry_per_simd"]
                                               / res["uniform"]["spin_signed"]["ns_per_entry_per_simd"])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
