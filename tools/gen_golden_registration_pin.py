"""tests/golden/registration_sums_pin.npz: what sf_ransac_refit_sums, sf_ransac_hypotheses, sf_fgr_sums, sf_sc2_seed_fits,
sf_icp_accumulate_robust (Cauchy) and sf_icp_accumulate_trimmed (trim 0.8) return, as the build it is run on returns them.  Taken
on the build BEFORE the four-wave block sums, the Kabsch tails and the refit sums of ransac.hip, fgr.hip, consistency.hip and
icp.hip were folded into one definition each: tests/test_hip_registration_pin.py holds every later build to these bits.

The inputs, the cases and the recording are that test's (`matched`, `draws_of`, `sc2_case`, `record`): exact integer arithmetic,
formed again by whoever needs them, so only the results are stored.  The conditions the test places on them are asserted here
(`stored_conditions`), and nothing is written unless two recordings agree byte for byte.
Run on the GPU box: python tools/gen_golden_registration_pin.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import test_hip_registration_pin as P
    from shot_fpfh_amd.engine import default_engine

    eng = default_engine()
    first, second = P.record(eng), P.record(eng)
    differ = [k for k in first if first[k].tobytes() != second[k].tobytes()]
    if differ or set(first) != set(second):
        raise SystemExit(f"two recordings differ in {differ}: a run is not reproducible bit for bit here, nothing written")
    for size in P.DRAW_SIZES:
        print("draw size", size, "status", first[f"hyp_status_{size}"].tolist())
    for m in P.SC2_M:
        print("sc2 m", m, "status", first[f"sc2_status_{m}"].tolist(), "size", first[f"sc2_size_{m}"].tolist())
    print("refit kept", [int(first[f"refit_{m}"][0]) for m in P.REFIT_M], "trimmed used", first["icp_trimmed"][..., 0].tolist())
    P.stored_conditions(first)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", P.PIN)
    np.savez(dst, **first)
    print("wrote", dst, eng.lib.sf_version().decode(), {k: v.shape for k, v in first.items()})


if __name__ == "__main__":
    main()
