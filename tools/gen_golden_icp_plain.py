"""tests/golden/icp_plain_sums.npz: the 40 numbers of the plain ICP entry points (sf_icp_accumulate in modes 0 and 1,
sf_icp_accumulate_gicp at epsilon 1e-3) on a small input set, as the build it is run on returns them, with the inputs.  Taken on
the build BEFORE the unweighted sums kernels of these two calls were deleted in favour of the weighted family of K17:
tests/test_hip_icp_robust.py holds every later build to these bits.

The inputs follow the recipe of tests/test_hip_gicp.py::one_pass_set at reduced size: 500 reference points and 600 scan rows with
unit normals, the three states (identity, true motion, 0.3 rad away), d_max = 0.05, all rows and a selection of 150 with repeats.
The conditions the test places on them are asserted here without a device (tests/test_icp_robust_host.py repeats them on the
file), and nothing is written unless two recordings, each from a `_Registration` of its own, agree byte for byte.
Run on the GPU box: python tools/gen_golden_icp_plain.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_REF, N_SCAN, N_SEL, SEED, SEL_SEED, D_MAX, EPSILON = 500, 600, 150, 2009, 5, 0.05, 1e-3


def inputs() -> dict:
    import gicp_numpy as G
    from test_hip_gicp import _unit

    rng = np.random.default_rng(SEED)
    ref, nref = rng.random((N_REF, 3)), _unit(rng.standard_normal((N_REF, 3)))
    world = ref[rng.integers(0, N_REF, N_SCAN)] + 0.03 * rng.standard_normal((N_SCAN, 3))
    r0, t0 = G.true_motion()
    scan, na = (world - t0) @ r0, _unit(rng.standard_normal((N_SCAN, 3)))
    away = G.rodrigues(0.3 * np.array([1.0, 2.0, -2.0]) / 3.0) @ r0
    return dict(ref=ref, ref_normals=nref, scan=scan, scan_normals=na,
                selection=np.random.default_rng(SEL_SEED).integers(0, N_SCAN, N_SEL),
                rotations=np.stack([np.eye(3), r0, away]), translations=np.stack([np.zeros(3), t0, t0]),  # state 0: no transform
                d_max=np.float64(D_MAX), epsilon=np.float64(EPSILON))


def main() -> None:
    import test_hip_icp_robust as H
    from shot_fpfh_amd.engine import default_engine

    g = inputs()
    kept = H.plain_golden_input_conditions(g)  # unambiguous, the kept counts of the test, every one at least 30
    print("kept pairs per (state, rows):", kept)
    eng = default_engine()
    first, second = H.plain_golden_sums(eng, g), H.plain_golden_sums(eng, g)
    if first.tobytes() != second.tobytes():
        raise SystemExit(f"two recordings differ at {np.argwhere(first != second).tolist()}: a run is not reproducible bit for "
                         "bit here, nothing written")
    assert first[..., 0].tolist() == [kept] * 3 and not first[..., 7].any()
    g["sums"] = first
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "icp_plain_sums.npz")
    np.savez(dst, **g)
    print("wrote", dst, eng.lib.sf_version().decode(), {k: v.shape for k, v in g.items()})


if __name__ == "__main__":
    main()
