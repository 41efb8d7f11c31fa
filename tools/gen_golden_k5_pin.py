"""tests/golden/k5_rows_pin.npz: the rows and frames every form of K5 (the SHOT descriptor) returns, as the build it is run on returns
them.  Taken on the build BEFORE the pieces the four bodies of shot.hip / shot_bins.hip share were given one definition each in
shot_core.h: tests/test_hip_k5_pin.py holds every later build to these bits.

The clouds, the cases and the recording are that test's (`record`): only hashes, launch names and 16 rows per case are stored.
What the cases were chosen for is asserted while recording and again on the result (`stored_conditions`); nothing is written
unless two recordings agree byte for byte, and the file must stay under 1 MiB.
Run on the GPU box: python tools/gen_golden_k5_pin.py [destination]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main() -> None:
    import test_hip_k5_pin as P
    from shot_fpfh_amd.engine import default_engine

    eng = default_engine()
    first, second = P.record(eng), P.record(eng)
    differ = [k for k in first if k not in second or first[k].tobytes() != second[k].tobytes()]
    if differ or set(first) != set(second):
        raise SystemExit(f"two recordings differ in {differ}: a run is not reproducible bit for bit here, nothing written")
    for k in sorted(first):
        if k.endswith("__launches"):
            c = k[: -len("__launches")]
            print(c, "longest", first[f"{c}__longest"].tolist(), "zero rows", first[f"{c}__zero_rows"].tolist(), first[k].tolist())
    print("chunk edges among the external queries", first["index__edge_lengths"].tolist())
    P.stored_conditions(_AsFile(first))
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", P.PIN)
    np.savez_compressed(dst, **first)
    size = os.path.getsize(dst)
    if size >= 1 << 20:
        os.remove(dst)
        raise SystemExit(f"{dst} would be {size} bytes: over the 1 MiB a committed file may have, removed")
    P.stored_conditions(np.load(dst, allow_pickle=False))
    print("wrote", dst, size, "bytes", eng.lib.sf_version().decode(), len(first), "arrays")


class _AsFile(dict):
    """A recording with the `files` of a loaded .npz."""

    @property
    def files(self):
        return list(self)


if __name__ == "__main__":
    main()
