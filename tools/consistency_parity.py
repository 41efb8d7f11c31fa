#!/usr/bin/env python3
"""What the geometric-consistency filter does to sets of matches of falling true share, on one MI355X: writes
profiles/consistency_parity.md.  Table 1: per set the degrees of true and false matches, the group, what is kept, and the share of
the group each kind is compatible with -- down to the shares at which the filter stops separating.  Table 2: |R - R0| of
ransac_prerejective and fast_global_registration before and after the filter on the six accuracy sets of README.

    python tools/consistency_parity.py [--out profiles/consistency_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from consistency_numpy import compat_rows, synthetic_truth  # noqa: E402
from ransac_numpy import matched_points, synthetic_matches  # noqa: E402

THR = 0.01
SEPARATION_SETS = [(5000, 0.10, 5010), (5000, 0.05, 1), (2000, 0.05, 2), (2000, 0.30, 3), (20000, 0.05, 2), (20000, 0.10, 1),
                   (20000, 0.02, 6), (20000, 0.01, 7)]
ACCURACY_SETS = [(20000, 0.30, 0), (20000, 0.10, 1), (20000, 0.05, 2), (2000, 0.30, 3), (200000, 0.30, 4), (20000, 0.50, 5)]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consistency_parity.md"))
    a = ap.parse_args()
    import shot_fpfh_amd as s
    from shot_fpfh_amd.matching import fast_global_registration, geometric_consistency_filter, ransac_prerejective

    engine = s.Engine()
    lines = ["# Geometric-consistency filter (K13) on synthetic matches", "",
             f"Library `{engine.lib.sf_version().decode()}`, written by `tools/consistency_parity.py` on one MI355X. Sets of",
             "`tests/ransac_numpy.synthetic_matches` (sigma 0.002), `distance_threshold` = `min_edge` = 0.01, `group_share` 0.4 (the default).",
             "", "## What is kept", "",
             "| m, share, seed | true | degree of true: min / median | degree of false: max / median | seed is true | group | kept | true kept | false kept | in-group share: true min / false max |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for m, share, seed in SEPARATION_SETS:
        sk, rk, si, ri, r0, t0 = synthetic_matches(m, share, seed=seed)
        true, _ = synthetic_truth(m, share, seed)
        is_true = np.zeros(m, dtype=bool)
        is_true[true] = True
        _, _, rec = geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=engine)
        kept = np.zeros(m, dtype=bool)
        kept[rec.keep] = True
        member = compat_rows(*matched_points(si, ri, sk, rk), [rec.seed], THR)[0]  # (the seed's row, on the host)
        member[rec.seed] = True
        assert int(member.sum()) == rec.group_size
        frac = rec.group_degree / max(rec.group_size - 1, 1)
        t_in, f_in = frac[is_true & member], frac[~is_true & member]
        lines.append(f"| {m}, {share:.2f}, {seed} | {true.size} | {rec.degree[is_true].min()} / {int(np.median(rec.degree[is_true]))} | "
                     f"{rec.degree[~is_true].max()} / {int(np.median(rec.degree[~is_true]))} | {'yes' if is_true[rec.seed] else 'NO'} | "
                     f"{rec.group_size} | {rec.keep.size} | {int((kept & is_true).sum())} | {int((kept & ~is_true).sum())} | "
                     f"{(t_in.min() if t_in.size else float('nan')):.3f} / {(f_in.max() if f_in.size else float('nan')):.3f} |")
    lines += ["", "The in-group share is a member's degree inside the group over g - 1; for false matches it is taken over the false",
              "members of the group. Where the largest degree of a false match exceeds the smallest of a true one the seed can still be",
              "true (it is the maximum); the filter stops separating where the seed itself is false or true members fall under the share.",
              "", "## The two estimators before and after", "",
              "‖R − R₀‖ (Frobenius) on README's six accuracy sets, `ransac_prerejective` at its defaults (10 000 draws) and",
              "`fast_global_registration` at its defaults.", "",
              "| m, share, seed | kept / true | `ransac_prerejective` all | kept | `fast_global_registration` all | kept |", "|---|---|---|---|---|---|"]
    for m, share, seed in ACCURACY_SETS:
        sk, rk, si, ri, r0, t0 = synthetic_matches(m, share, seed=seed)
        true, _ = synthetic_truth(m, share, seed)
        ks, kr, rec = geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=engine)
        cells = []
        for fn in (lambda x, y: ransac_prerejective(x, y, sk, rk, n_draws=10000, distance_threshold=THR, engine=engine),
                   lambda x, y: fast_global_registration(x, y, sk, rk, distance_threshold=THR, engine=engine)):
            for x, y in ((si, ri), (ks, kr)):
                try:
                    cells.append(f"{np.linalg.norm(fn(x, y)[1].rotation - r0):.2e}")
                except ValueError as exc:
                    cells.append(f"error: {exc}")
        lines.append(f"| {m}, {share:.2f}, {seed} | {rec.keep.size} / {true.size} | " + " | ".join(cells) + " |")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
