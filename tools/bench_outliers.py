#!/usr/bin/env python3
"""Times of the two outlier filters (K20) on 1M-point clouds resident in HBM, next to the project's own kernels in the same
process.  Statistical filter (k = 20, std_ratio = 2): the self k-NN search at k + 1 in front (every launch of it: grid builds,
query sort, k-NN kernels, status counts), the mean-distance pass, the two statistics passes with their folds, the select -- all
from ONE profiled call per round -- and the public call host to host.  Radius filter: the count sweep beside the count pass of
sf_radius_search_self (exact scheme) at the same radius, and the public call.

Kernel times come from HIP events around the named launches (Engine.profile), call times from the host clock around calls that
end in a device synchronisation; every figure is the median of --repeats rounds after --warmup rounds.  Needs an MI355X: without
one the engine raises and nothing is printed.

    python tools/bench_outliers.py [--n 1000000] [--repeats 21] [--warmup 2] [--out profiles/outliers_bench.json]
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


def contaminated_sphere(n: int) -> np.ndarray:
    """noisy sphere (bench_iss.py's) with 2 % of the n points replaced by strays, uniform in [-0.25, 1.25)^3"""
    n_out = n // 50
    rng = np.random.default_rng(1)
    d = rng.standard_normal((n - n_out, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    sphere = (0.5 + 0.5 * d * (1.0 + 0.01 * rng.standard_normal((n - n_out, 1)))).astype(np.float32).astype(np.float64)
    strays = np.random.default_rng(101).random((n_out, 3), dtype=np.float32) * 1.5 - 0.25
    return np.vstack([sphere, strays.astype(np.float64)])


GROUPS = {"mean_distance_ms": ("k20_mean_distance",), "stats_ms": ("k20_stats",), "select_ms": ("k20_select",)}


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


def call_ms(fn, repeats: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    vals = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        vals.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(vals)


def bench_cloud(engine, name: str, p: np.ndarray, k: int, ratio: float, repeats: int, warmup: int) -> dict:
    from shot_fpfh_amd.outlier_removal import remove_radius_outliers, remove_statistical_outliers

    n = p.shape[0]
    cloud = engine.cloud(p)
    out = {"cloud": name, "n": n, "k": k, "std_ratio": ratio}
    try:
        kept, mean, st = cloud.statistical_outliers(k, ratio, return_stats=True)
        out.update(kept=int(kept.size), mu=float(st[0]), sigma=float(st[1]), threshold=float(st[2]))
        rounds = profiled_rounds(engine, lambda: cloud.statistical_outliers(k, ratio), repeats, warmup)
        for key, names in GROUPS.items():
            missing = [x for x in names if x not in rounds[0]]
            if missing:
                raise RuntimeError(f"no launch named {missing} was recorded (have {sorted(rounds[0])})")
            out[key] = statistics.median(sum(r[x] for x in names) for r in rounds)
        # the search in front: every launch of the call that is not one of K20's
        out["knn_search_ms"] = statistics.median(sum(v for x, v in r.items() if not x.startswith("k20_")) for r in rounds)
        out["knn_search_launches"] = sorted(x for x in rounds[0] if not x.startswith("k20_"))
        after = out["mean_distance_ms"] + out["stats_ms"] + out["select_ms"]
        out["after_search_ms"] = after
        out["after_search_over_search"] = after / out["knn_search_ms"]
        out["mean_distance_over_search"] = out["mean_distance_ms"] / out["knn_search_ms"]
        out["resident_call_ms"] = call_ms(lambda: cloud.statistical_outliers(k, ratio), repeats, warmup)
        out["remove_statistical_outliers_ms"] = call_ms(lambda: remove_statistical_outliers(p, k, ratio, engine=engine),
                                                        max(3, repeats // 3), 1)
        # radius filter at three times the cloud's resolution
        radius = 3.0 * cloud.resolution(p)
        counts = cloud.ball_counts(radius)
        row = {"radius": radius, "min_neighbors": 6, "mean_ball": float(counts.mean()), "kept": int(cloud.radius_outliers(radius, 6).size)}
        rounds = profiled_rounds(engine, lambda: cloud.radius_outliers(radius, 6), repeats, warmup)
        row["ball_count_ms"] = statistics.median(r["k20_ball_count"] for r in rounds)
        row["scatter_ms"] = statistics.median(r["k20_scatter"] for r in rounds)
        row["select_ms"] = statistics.median(r["k20_select"] for r in rounds)
        os.environ["SF_K2_EXACT"] = "1"
        try:
            rounds = profiled_rounds(engine, lambda: cloud.radius_search_self(radius).free(), repeats, warmup)
        finally:
            del os.environ["SF_K2_EXACT"]
        row["k2_radius_count_ms"] = statistics.median(r["k2_radius_count"] for r in rounds)
        row["ball_count_over_k2_count"] = row["ball_count_ms"] / row["k2_radius_count_ms"]
        row["resident_call_ms"] = call_ms(lambda: cloud.radius_outliers(radius, 6), repeats, warmup)
        row["remove_radius_outliers_ms"] = call_ms(lambda: remove_radius_outliers(p, radius, 6, engine=engine), max(3, repeats // 3), 1)
        out["radius_filter"] = row
    finally:
        cloud.free()
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--std-ratio", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    import shot_fpfh_amd as s

    engine = s.Engine()  # (raises without a GPU: no figure is ever printed from a CPU)
    res = {"tool": "tools/bench_outliers.py", "library": engine.lib.sf_version().decode(), "repeats": a.repeats, "warmup": a.warmup,
           "clouds": [bench_cloud(engine, "uniform", uniform_cloud(a.n), a.k, a.std_ratio, a.repeats, a.warmup),
                      bench_cloud(engine, "contaminated_sphere", contaminated_sphere(a.n), a.k, a.std_ratio, a.repeats, a.warmup)]}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
