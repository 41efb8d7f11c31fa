#!/usr/bin/env python3
"""Times of the Harris 3D keypoint detector (K23) on 1M-point clouds resident in HBM, next to the project's own sweeps at the
same radius in the same process:

  k_harris_tensor   against sf_ball_counts' count sweep (the same sweep without the normal loads and the six accumulations)
                    and against sf_normals_radius' k_radius_cov (the sweep plus an LDS list and two reductions);
  k_harris_response against nothing (one lane per point);
  the suppression of the Harris response against k10_iss_nms on ISS's saliency (the same kernel, other scores);
  the resident call (Cloud.harris_keypoints) and the host-to-host call (select_keypoints_harris).

Kernel times come from HIP events around the named launches (Engine.profile), call times from the host clock around calls that
end in a device synchronisation; every figure is the median of --repeats rounds after --warmup rounds, all in one process.
The normals are compute_normals(radius=r)'s.  Needs an MI355X: without one the engine raises and nothing is printed.

    python tools/bench_harris.py [--n 1000000] [--radius 0.03] [--repeats 21] [--warmup 2] [--out profiles/harris_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from bench_iss import call_ms, kernel_ms, noisy_sphere, uniform_cloud  # noqa: E402

# k_harris_tensor's sweep loop in the build's ISA listing: per step of 128 candidates and wave, 127 instructions
# of which 42 are float64 vector instructions (4 cycles each on a SIMD) and 6 are 16-byte loads (one wave instruction per 16
# cycles on a CU's vector-memory pipe); 1 024 SIMDs, 256 CUs, 2.4 GHz at most
SWEEP_F64, SWEEP_LOADS, SIMDS, CUS, MAX_GHZ = 42, 6, 1024, 256, 2.4


def bench_cloud(engine, name: str, p, r: float, repeats: int, warmup: int) -> dict:
    from shot_fpfh_amd.descriptors import compute_normals
    from shot_fpfh_amd.keypoint_selection import select_keypoints_harris

    n = p.shape[0]
    nr = compute_normals(p, p, radius=r, engine=engine)
    cloud = engine.cloud(p, nr)
    out = {"cloud": name, "n": n, "radius": r, "methods": []}
    try:
        res, cnt = cloud.harris_response(r, "harris", return_counts=True)
        out["mean_ball"] = float(cnt.mean())
        out["max_ball"] = int(cnt.max())
        # every ball member is a candidate and a step takes 128 candidates: a lower bound of the steps the sweep makes (it
        # visits about three candidates per member: the window of search_util.h), hence of its time at the maximum clock
        steps = int(np.ceil(cnt / 128.0).sum())
        out["min_sweep_steps"] = steps
        out["float64_issue_floor_ms"] = steps * SWEEP_F64 * 4 / (SIMDS * MAX_GHZ * 1e9) * 1e3
        out["load_issue_floor_ms"] = steps * SWEEP_LOADS * 16 / (CUS * MAX_GHZ * 1e9) * 1e3
        normals = engine.empty((n, 3))
        # the three sweeps on the same grid (each call leaves the grid of r behind)
        out["harris_tensor_ms"] = kernel_ms(engine, ["k23h_harris_tensor"], lambda: cloud.harris_response(r), repeats, warmup)
        out["normals_soa_ms"] = kernel_ms(engine, ["k23h_normals_soa"], lambda: cloud.harris_response(r), repeats, 0)
        out["ball_count_ms"] = kernel_ms(engine, ["k20_ball_count"], lambda: cloud.ball_counts(r), repeats, warmup)
        out["radius_cov_ms"] = kernel_ms(engine, ["k23_radius_cov"], lambda: cloud.normals_radius_self(r, normals), repeats, warmup)
        out["tensor_over_load_issue_floor"] = out["harris_tensor_ms"] / out["load_issue_floor_ms"]
        out["tensor_over_count"] = out["harris_tensor_ms"] / out["ball_count_ms"]
        out["tensor_over_radius_cov"] = out["harris_tensor_ms"] / out["radius_cov_ms"]
        normals.free()
        sal = cloud.iss_saliency(r)
        out["iss_salient"] = int((sal > 0).sum())
        out["iss_nms_ms"] = kernel_ms(engine, ["k10_iss_nms"], lambda: cloud.iss_select(sal, r), repeats, warmup)
        for method in ("harris", "noble", "lowe", "tomasi", "curvature"):
            res = cloud.harris_response(r, method)
            kp = cloud.iss_select(res, r)
            row = {"method": method, "accepted": int((res > 0).sum()), "keypoints": int(kp.size)}
            row["response_kernel_ms"] = kernel_ms(engine, ["k23h_harris_response"], lambda: cloud.harris_response(r, method), repeats, warmup)
            if method == "curvature":
                row["position_cov_ms"] = kernel_ms(engine, ["k23h_position_cov"], lambda: cloud.harris_response(r, method), repeats, 0)
            row["nms_kernel_ms"] = kernel_ms(engine, ["k10_iss_nms"], lambda: cloud.iss_select(res, r), repeats, warmup)
            row["nms_over_iss_nms"] = row["nms_kernel_ms"] / out["iss_nms_ms"]
            row["suppression_ms"] = kernel_ms(engine, ["k10_iss_gather", "k10_iss_nms", "k10_iss_compact"], lambda: cloud.iss_select(res, r),
                                              repeats, 0)
            row["keypoints_call_ms"] = call_ms(lambda: cloud.harris_keypoints(r, r, method), repeats, warmup)
            if method in ("harris", "curvature"):
                row["select_keypoints_harris_ms"] = call_ms(
                    lambda: select_keypoints_harris(p, None if method == "curvature" else nr, r, method=method, engine=engine),
                    max(3, repeats // 3), 1)
            out["methods"].append(row)
    finally:
        cloud.free()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--radius", type=float, default=0.03)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    res = {"tool": "tools/bench_harris.py", "library": engine.lib.sf_version().decode(), "repeats": a.repeats, "warmup": a.warmup,
           "clouds": [bench_cloud(engine, "uniform", uniform_cloud(a.n), a.radius, a.repeats, a.warmup),
                      bench_cloud(engine, "noisy_sphere", noisy_sphere(a.n), a.radius, a.repeats, a.warmup)]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
