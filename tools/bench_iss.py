#!/usr/bin/env python3
"""Times of the ISS keypoint detector (K10) on 1M-point clouds resident in HBM, next to the project's own kernels in the
same process: the saliency pass against compute_normals(radius=r_s) (the same sweep + a heavier eigen-solve), the suppression
pass against K2's count pass at r_n (the same sweep, one load less, no early exit).

Kernel times come from HIP events around the named launches (Engine.profile), call times from the host clock around calls
that end in a device synchronisation; every figure is the median of --repeats runs after --warmup runs.  Needs an MI355X:
without one the engine raises and nothing is printed.

    python tools/bench_iss.py [--n 1000000] [--repeats 9] [--warmup 2] [--out profiles/iss_bench.json]
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


def uniform_cloud(n: int) -> np.ndarray:
    return np.random.default_rng(7).random((n, 3), dtype=np.float32).astype(np.float64)


def noisy_sphere(n: int) -> np.ndarray:
    rng = np.random.default_rng(1)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (0.5 + 0.5 * d * (1.0 + 0.01 * rng.standard_normal((n, 1)))).astype(np.float32).astype(np.float64)


def kernel_ms(engine, names, fn, repeats: int, warmup: int) -> float:
    """median over the repeats of the summed event time of the launches called `names` inside fn()"""
    for _ in range(warmup):
        fn()
    engine.profile(True)
    vals = []
    try:
        for _ in range(repeats):
            engine.profile_reset()
            fn()
            engine.sync()
            rep = engine.profile_report()
            missing = [k for k in names if k not in rep or rep[k][0] == 0]
            if missing:
                raise RuntimeError(f"no launch named {missing} was recorded (have {sorted(rep)})")
            vals.append(sum(rep[k][1] for k in names))
    finally:
        engine.profile(False)
    return statistics.median(vals)


def call_ms(fn, repeats: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    vals = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        vals.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(vals)


def bench_cloud(engine, name: str, p: np.ndarray, repeats: int, warmup: int) -> dict:
    from shot_fpfh_amd.keypoint_selection import select_keypoints_iss

    n = p.shape[0]
    cloud = engine.cloud(p)
    out = {"cloud": name, "n": n, "radii": []}
    try:
        rho = cloud.resolution(p)
        out["resolution"] = rho
        normals = engine.empty((n, 3))
        for label, r_s, r_n in (("automatic", 6.0 * rho, 4.0 * rho), ("r_s=0.03", 0.03, 0.02)):
            sal, cnt = cloud.iss_saliency(r_s, return_counts=True)
            kp = cloud.iss_select(sal, r_n)
            row = {"radii": label, "salient_radius": r_s, "non_max_radius": r_n, "mean_ball_salient": float(cnt.mean()),
                   "salient": int((sal > 0).sum()), "keypoints": int(kp.size)}
            # the saliency pass and its yardstick on the same grid (iss_saliency leaves the grid of r_s behind)
            row["saliency_ms"] = kernel_ms(engine, ["k10_iss_cov", "k10_iss_saliency"], lambda: cloud.iss_saliency(r_s), repeats, warmup)
            row["normals_radius_ms"] = kernel_ms(engine, ["k23_radius_cov", "k3_normals"],
                                                 lambda: cloud.normals_radius_self(r_s, normals), repeats, warmup)
            row["saliency_over_normals"] = row["saliency_ms"] / row["normals_radius_ms"]
            # the suppression pass and K2's count pass (the exact count -> scan -> fill scheme, the count launch alone)
            row["suppression_ms"] = kernel_ms(engine, ["k10_iss_gather", "k10_iss_nms", "k10_iss_compact"],
                                              lambda: cloud.iss_select(sal, r_n), repeats, warmup)
            row["nms_kernel_ms"] = kernel_ms(engine, ["k10_iss_nms"], lambda: cloud.iss_select(sal, r_n), repeats, 0)
            os.environ["SF_K2_EXACT"] = "1"
            try:
                row["k2_count_ms"] = kernel_ms(engine, ["k2_radius_count"], lambda: cloud.radius_search_self(r_n), repeats, warmup)
            finally:
                del os.environ["SF_K2_EXACT"]
            row["suppression_over_count"] = row["suppression_ms"] / row["k2_count_ms"]
            # whole calls: both passes on the resident cloud (grid builds and the read-back of the indices included), and the
            # public function from host points (upload and, for automatic radii, the resolution included)
            row["keypoints_call_ms"] = call_ms(lambda: cloud.iss_keypoints(r_s, r_n), repeats, warmup)
            auto = label == "automatic"
            row["select_keypoints_iss_ms"] = call_ms(
                lambda: select_keypoints_iss(p, None if auto else r_s, None if auto else r_n, engine=engine), max(3, repeats // 3), 1)
            out["radii"].append(row)
        normals.free()
    finally:
        cloud.free()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    res = {"tool": "tools/bench_iss.py", "library": engine.lib.sf_version().decode(), "repeats": a.repeats, "warmup": a.warmup,
           "clouds": [bench_cloud(engine, "uniform", uniform_cloud(a.n), a.repeats, a.warmup),
                      bench_cloud(engine, "noisy_sphere", noisy_sphere(a.n), a.repeats, a.warmup)]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
