"""tests/golden/plumbing_pin.npz: what the calls of tests/plumbing_cases.py return, how often each waits for the stream and
which timer names it launches under, as the build it is run on has them.  Taken on the build BEFORE the entry points' host
plumbing (the two-phase rocPRIM calls, the host / device staging, the maps between the caller's and the cell-sorted order) was
folded into one definition each: tests/test_hip_plumbing_pin.py holds every later build to this record.

The cases and the recording are tests/plumbing_cases.py's, which the test runs too; nothing is written unless two recordings
agree.  The library's build id goes into the file.
Run on the GPU box: python tools/gen_golden_plumbing_pin.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import plumbing_cases as P
    from shot_fpfh_amd import _ffi

    first = {name: P.run_group(name) for name in P.GROUPS}
    second = {name: P.run_group(name) for name in P.GROUPS}
    differ = [(g, c) for g in first for c in first[g] if first[g][c] != second[g].get(c)]
    if differ:
        raise SystemExit(f"two recordings differ in {differ}: nothing written")
    for g, rows in first.items():
        for c, row in rows.items():
            print(g, c, row["syncs"], row["launches"], [s[:8] for s in row["sha256"]])
    build = _ffi.load().sf_version().decode()
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "plumbing_pin.npz")
    np.savez_compressed(dst, build=np.array(build), **{g: np.array(json.dumps(rows, sort_keys=True)) for g, rows in first.items()})
    print("wrote", dst, build, sum(len(r) for r in first.values()), "calls")


if __name__ == "__main__":
    main()
