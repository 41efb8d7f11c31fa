#!/usr/bin/env python3
"""Where one second-order seed stops being enough, and what many seeds recover: a table computed from the NumPy statements of
tests/ (sc2_numpy, sc2_registration_numpy; CPU only), and -- with --device, on an MI355X -- the worst measured multiples of the two
floating-point bounds the device's fits are held to (tests/test_hip_sc2_registration.py).

Per set synthetic_matches(m, share, seed), distance_threshold = min_edge = 0.01: the true matches, whether the filter's seed (the
first maximum of s2) is true and what the filter keeps, and for S = 1, 16, 64, 256 seeds the winner of sc2_registration: its
inliers after the refit and |R - R0|.  The seeds of S are the first S of 256, so one pass at 256 serves all four.

    python tools/sc2_registration_parity.py [--device] [--no-table] [--out profiles/sc2_registration_parity.md]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import consistency_numpy as C  # noqa: E402
import ransac_numpy as N  # noqa: E402
import sc2_numpy as S  # noqa: E402
import sc2_registration_numpy as R  # noqa: E402

THR = 0.01
EPS = 2.0 ** -52
SEEDS = (1, 16, 64, 256)
THIN_SETS = [(5000, 0.004, 1), (5000, 0.003, 1), (5000, 0.003, 2)]
README_SETS = [(2000, 0.05, 2), (5000, 0.05, 1), (5000, 0.02, 3), (5000, 0.01, 4), (5000, 0.006, 5), (8000, 0.01, 7), (8000, 0.005, 8)]
DEVICE_SETS = [(2000, 0.05, 2), (5000, 0.004, 1), (5000, 0.01, 4)]


def statement_row(case):
    m, share, seed = case
    sk, rk, si, ri, r0, t0 = N.synthetic_matches(m, share, seed=seed)
    true = C.synthetic_truth(m, share, seed)[0]
    a, b = N.matched_points(si, ri, sk, rk)
    hyp = R.hypotheses(a, b, THR, n_seeds=max(SEEDS))
    is_true = np.zeros(m, dtype=bool)
    is_true[true] = True
    first = int(hyp["seeds"][0])
    kept = np.flatnonzero(hyp["member"][0])  # the filter's own rule on the first seed's row
    scored = np.flatnonzero(hyp["status"] == 0)
    counts = N.score(a, b, hyp["rt"][scored], THR)
    cells = []
    for n in SEEDS:
        use = scored < n
        if not use.any():
            cells.append(f"S = {n}: nothing scored")
            continue
        w = N.first_max(counts[use])
        rank = int(scored[use][w])
        rt, count, _ = N.refit(a, b, hyp["rt"][rank], int(counts[use][w]), THR, 2)
        cells.append(f"S = {n}: {count} ({np.linalg.norm(rt[:9].reshape(3, 3) - r0):.1e}), rank {rank}")
    return (f"| {m}, {share}, {seed} | {true.size} | {'yes' if is_true[first] else '**no**'} | "
            f"{int(is_true[kept].sum())} / {int((~is_true[kept]).sum())} | " + " · ".join(cells) + " |")


def device_rows():
    import shot_fpfh_amd as s

    eng = s.Engine()  # (raises without a GPU)
    out = []
    for case in DEVICE_SETS:
        sk, rk, si, ri = N.synthetic_matches(case[0], case[1], seed=case[2])[:4]
        a, b = N.matched_points(si, ri, sk, rk)
        m, pad, n = a.shape[0], eng.sc2_padded(a.shape[0]), 64
        want = R.hypotheses(a, b, THR, n_seeds=n)
        held = [eng.empty((m, 3)).from_host(a), eng.empty((m, 3)).from_host(b), eng.empty((pad, pad), np.uint8)]
        try:
            da, db, dmat = held
            eng.consistency_matrix(da, db, m, THR, THR, out=dmat)
            held.append(eng.empty((m,), np.uint32).from_host(eng.consistency_sc2(dmat, m)))
            for shape, dt in (((n,), np.int32), ((n, pad), np.uint32), ((n,), np.uint8), ((n,), np.int32), ((n, 12), np.float64),
                              ((n, 24), np.float64)):
                held.append(eng.empty(shape, dt))
            ds2, dseeds, drows, dst, dsz, drt, dsums = held[3:]
            eng.sc2_seeds_device(ds2, m, n, dseeds)
            eng.sc2_seed_rows_device(dmat, m, dseeds, n, drows)
            eng.sc2_seed_fits_device(da, db, m, dseeds, drows, n, 0.5, dst, dsz, drt, dsums)
            status, size, rt, sums = dst.to_host(), dsz.to_host(), drt.to_host(), dsums.to_host()
        finally:
            for h in held:
                h.free()
        exact = np.array_equal(status, want["status"]) and np.array_equal(size, want["size"])
        w_sum = w_r = w_t = 0.0
        for k in np.flatnonzero(status == 0):
            ws, tol = want["sums"][k], float(size[k]) * EPS
            for mine, ref, scale in ((sums[k, 17:20], ws["sum_a"], ws["sum_a_abs"]), (sums[k, 20:23], ws["sum_b"], ws["sum_b_abs"]),
                                     (sums[k, 7:16].reshape(3, 3), ws["h"], ws["h_abs"])):
                w_sum = max(w_sum, float((np.abs(mine - ref) / (tol * scale)).max()))
            unit = EPS * want["cond"][k]
            w_r = max(w_r, float(np.abs(rt[k, :9] - want["rt"][k, :9]).max() / unit))
            w_t = max(w_t, float(np.abs(rt[k, 9:] - want["rt"][k, 9:]).max() / (unit * (1 + np.linalg.norm(ws["abar"])))))
        out.append(f"| {case[0]}, {case[1]}, {case[2]} | {int((status == 0).sum())} of {n} | {'yes' if exact else '**no**'} | "
                   f"{w_sum:.3f} | {w_r:.2f} | {w_t:.2f} |")
    return eng.lib.sf_version().decode(), out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", action="store_true", help="also measure the device's fits against the statement (needs an MI355X)")
    ap.add_argument("--no-table", action="store_true", help="leave the CPU table out (to refresh the device figures alone)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# SC2 registration: one seed against many", "",
             "Computed by `tools/sc2_registration_parity.py` from the NumPy statements of `tests/` (`synthetic_matches(m, share, "
             "seed)`, `distance_threshold = min_edge = 0.01`, `group_share = 0.5`, two refits).  \"keeps\" is the filter's rule on the "
             "first seed's row, true / false; a cell is the winner's inliers after the refit, ‖R − R₀‖ and the winning seed's rank.", "",
             "| set (m, share, seed) | true | the filter's seed is true | the filter keeps true / false | best of the first S seeds |",
             "|---|---|---|---|---|"]
    if a.no_table:
        lines = []
    for case in [] if a.no_table else THIN_SETS + README_SETS:
        lines.append(statement_row(case))
        print(lines[-1], flush=True)
    if a.device:
        version, rows = device_rows()
        lines += ["", f"## The device's fits against the statement ({version})", "",
                  "64 seeds a set.  The sums (Σa, Σb and the centred cross-covariance of each consensus set) are held to size × 2⁻⁵² "
                  "relative to the sums of absolute terms, the transforms to 64 × 2⁻⁵² × s1 / gap (× (1 + ‖ā‖) for t); the columns "
                  "are the worst measured multiples of size × 2⁻⁵² and of 2⁻⁵² × s1 / gap.", "",
                  "| set | fits | status and size exact | sums | R | t |", "|---|---|---|---|---|---|"] + rows
        for r in rows:
            print(r)
    else:
        lines += ["", "No device figures: the tool was run without `--device`."]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
