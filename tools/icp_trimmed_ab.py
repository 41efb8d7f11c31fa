#!/usr/bin/env python3
"""Same-box A/B of the EXISTING ICP entry points between this tree and a copy of another commit's (built in place, e.g. under
abl_libs/other_tree as tools/ab_tree.sh describes): alternating, --rounds (3) rounds, in every round tools/bench_icp_robust.py of
each tree with its defaults (a 10^5-point scan against a 10^6-point reference, 21 repeats after 3 warm-up rounds), every run a
process of its own.  Compared: the one-iteration host-to-host median of sf_icp_accumulate / sf_icp_accumulate_gicp ("plain") and of
sf_icp_accumulate_robust without a loss and with Cauchy.  The yardstick is the other tree's spread (max - min) over its rounds.
Writes a markdown table.  Needs an MI355X.

    python tools/icp_trimmed_ab.py abl_libs/other_tree [--rounds 3] [--out profiles/icp_trimmed_ab.md]
A later change to the kernel family names itself with --title and --change (K19: profiles/icp_symmetric_ab.md).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("plain", "none", "cauchy")
TITLE = "Trimmed ICP (K18)"
CHANGE = ("K18 gave `k_icp_sums` one more argument, a nullable pointer to the cut, which the three existing entry points pass as null, "
          "and moved the residual into a function it shares with the key pass")


def run(tree):
    p = subprocess.run([sys.executable, os.path.join("tools", "bench_icp_robust.py")], cwd=tree, capture_output=True, text=True, timeout=600)
    if p.returncode:
        raise SystemExit(f"{tree}: tools/bench_icp_robust.py failed ({p.returncode})\n{p.stderr[-2000:]}")
    return json.loads(p.stdout[p.stdout.index("{"):])


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("other")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_trimmed_ab.md"))
    ap.add_argument("--title", default=TITLE, help="what the new tree adds, for the heading")
    ap.add_argument("--change", default=CHANGE, help="what it changed in the code the existing calls run, for the text")
    a = ap.parse_args()
    trees = {"parent": os.path.abspath(a.other), "new": ROOT}
    runs = {name: [] for name in trees}
    for r in range(a.rounds):
        for name, tree in trees.items():
            runs[name].append(run(tree))
            print(f"round {r + 1} {name}: " + ", ".join(f"{m} {v['plain']['one_iteration_host_to_host_ms_median']:.3f}"
                                                        for m, v in runs[name][-1]["modes"].items()), flush=True)
    out = [f"# {a.title}: the existing ICP calls against the parent commit, same box", "",
           f"Written by `tools/icp_trimmed_ab.py` from one call on one MI355X: the parent commit's tree (its own library, Python and tools)",
           f"and this tree, alternating, {a.rounds} rounds; in every round `tools/bench_icp_robust.py` with its defaults (a 10^5-point scan against",
           "a 10^6-point reference, 21 repeats after 3 warm-up rounds), every run a process of its own.  The figure is the one-iteration",
           f"host-to-host median in ms.  {a.change}; the bar is the parent's own",
           "spread (max - min) over its rounds: the new median passes where it lies within that spread of the parent's median, or below it.", "",
           f"libraries: parent `{runs['parent'][0]['library']}`, new `{runs['new'][0]['library']}`", "",
           "| mode | call | parent, rounds | parent median | parent spread | new, rounds | new median | new - parent | within the spread |",
           "|---|---|---|---|---|---|---|---|---|"]
    worst = None
    for mode in runs["new"][0]["modes"]:
        for row in ROWS:
            v = {name: [r["modes"][mode][row]["one_iteration_host_to_host_ms_median"] for r in runs[name]] for name in trees}
            pm, nm = statistics.median(v["parent"]), statistics.median(v["new"])
            spread = max(v["parent"]) - min(v["parent"])
            ok = nm - pm <= spread
            worst = (nm - pm - spread) if worst is None else max(worst, nm - pm - spread)
            call = {"plain": "plain entry point", "none": "`_robust`, no loss", "cauchy": "`_robust`, Cauchy"}[row]
            out.append(f"| {mode} | {call} | " + " / ".join(f"{x:.3f}" for x in v["parent"]) + f" | {pm:.3f} | {spread:.3f} | "
                       + " / ".join(f"{x:.3f}" for x in v["new"]) + f" | {nm:.3f} | {nm - pm:+.3f} | {'yes' if ok else 'NO'} |")
    out += ["", "### The sums kernels of one plain call, µs (HIP events around the named launches, median of 5 per run; the rounds)", "",
            "| mode | library | launches: µs per round |", "|---|---|---|"]
    for mode in runs["new"][0]["modes"]:
        for name in trees:
            names = sorted(runs[name][0]["modes"][mode]["plain"]["sums_kernels"])
            cells = []
            for n in names:
                k = [r["modes"][mode]["plain"]["sums_kernels"][n] for r in runs[name]]
                cells.append(f"`{n} x {k[0]['launches']}` " + " / ".join(f"{x['ms'] * 1e3:.1f}" for x in k))
            out.append(f"| {mode} | {name} | " + "; ".join(cells) + " |")
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
