"""tests/golden/normals_radius_sums.npz: compute_normals(radius=) of a small cloud at two radii, as the build it is run on
returns them.  Taken on the build BEFORE sf_wave_sum8 / sf_wave_sum4 moved their lane^32 and lane^16 exchanges onto the
lane-swap instructions (device_util.h): tests/test_k7_moments.py holds every later build to these bits -- the radius sweep
reduces its barycentre with sf_wave_sum4 and its covariance with sf_wave_sum8, and the normal is the covariance's
eigenvector, so a sum that paired other operands would show.  Run on the GPU box: python tools/gen_golden_k7_moments.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, SEED, RADII = 2000, 29, (0.08, 0.2)


def main() -> None:
    import shot_fpfh_amd as s
    from conftest import synth_cloud

    p, _, _ = synth_cloud(N, SEED)
    out = {"radii": np.array(RADII)}
    for i, r in enumerate(RADII):
        out[f"normals_{i}"] = s.compute_normals(p, p, radius=r)
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "normals_radius_sums.npz")
    np.savez(dst, **out)
    print("wrote", dst, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
