#!/usr/bin/env python3
"""Generate tests/golden/shot_ties.npz by IMPORTING the reference (aubin-tchoi/shot-fpfh): compute_single_shot_descriptor
(shot.py:175-306) on neighbourhoods of lattice clouds, where neighbours tie in distance in every list and the reference's row
depends on what its `np.argsort(rho)` (shot.py:218) makes of the ties.

Runs only in the build container, where /root/reference exists:

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_shot_ties.py

Stores only data.  The clouds are those of tests/shot_ties_cases.py.  Per neighbourhood c (`cases` lists their names):
  <c>_ijk      the neighbours as int16 lattice coordinates, in ascending index of the caller's cloud (<c>_index), the keypoint
               included; <c>_pitch, <c>_point (the keypoint's lattice coordinates), <c>_radius, <c>_min_nb
  <c>_normals  the neighbours' normals, <c>_frame the local reference frame handed in (3 x 3)
  <c>_row1 / <c>_row0   the reference's row with normalize True / False
  <c>_order    np.argsort(rho) as this NumPy produced it for that call: the same expression on the same array
What the file is for is asserted here and again by tests/test_shot_ties_host.py: replaying <c>_order through
tests/shot_ties_numpy.py gives the reference's row bit for bit; turning the ties round moves at least half of the rows of every
cloud and length class by more than 1e-6; no bin-deciding quantity is within 1e-9 of an edge (the identity-frame case apart).
"""
from __future__ import annotations

import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from shot_fpfh.descriptors.shot import compute_single_shot_descriptor  # noqa: E402

import shot_ties_cases as C  # noqa: E402
import shot_ties_numpy as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "shot_ties.npz")
PER_CLASS = 4


def neighbourhood(out, name, ijk, pitch, normals, row, index, radius, frame, min_nb):
    pts = ijk[index].astype(np.float64) * pitch
    point = ijk[row].astype(np.float64) * pitch
    nrm = np.ascontiguousarray(normals[index])
    rows = [compute_single_shot_descriptor((point, pts, nrm, radius, frame, bool(n), min_nb)) for n in (0, 1)]
    rho = np.linalg.norm(pts - point, axis=1)
    rho = rho[rho > 0]
    order = np.argsort(rho)
    for n in (0, 1):
        again = T.shot_row(point, pts, nrm, radius, frame, bool(n), min_nb, T.recorded(order), index)
        assert np.array_equal(again, rows[n]), (name, n, np.abs(again - rows[n]).max())
    assert len(np.unique(rho)) < len(rho), name  # (a tie in the list)
    out[f"{name}_ijk"], out[f"{name}_index"] = ijk[index].astype(np.int16), index.astype(np.int32)
    out[f"{name}_pitch"], out[f"{name}_point"] = np.array([pitch]), ijk[row].astype(np.int16)
    out[f"{name}_radius"], out[f"{name}_min_nb"] = np.array([radius]), np.array([min_nb], dtype=np.int64)
    out[f"{name}_normals"], out[f"{name}_frame"] = nrm, np.ascontiguousarray(frame)
    out[f"{name}_row0"], out[f"{name}_row1"], out[f"{name}_order"] = rows[0], rows[1], order.astype(np.int32)


def estimate(points):
    from oracle import oracle as O

    return O.compute_normals(points, points, radius=3.3 * C.PITCH)


def main():
    out, names = {}, []
    ijk, _ = C.thinned_lattice()
    for kind in C.NORMAL_KINDS:
        normals = C.thin_normals(kind, estimate)
        for cls in C.GOLDEN_CLASSES:
            x = C.CLASSES[cls][0]
            kp = C.thin_keypoints(x)[:: max(1, C.MAX_KEYPOINTS // PER_CLASS)][:PER_CLASS]
            off, idx = C.thin_lists(x, kp)
            frames = C.rotations(len(kp), 100 + len(names))
            for i, row in enumerate(kp):
                name = f"thin_{kind}_{cls}_{i}"
                neighbourhood(out, name, ijk, C.PITCH, normals, row, idx[off[i]:off[i + 1]], C.check_radius(x), frames[i], 5)
                names.append(name)
    g, _, nr, row, radius = C.full_lattice()
    off, idx = C.brute_lists(g, np.array([row]), C.FULL_X)
    neighbourhood(out, "full_identity", g, C.PITCH, nr, row, idx, radius, np.eye(3), 5)
    names.append("full_identity")
    d, _, nr, radius = C.duplicated_points()
    rows = np.array([0, 301, 602])
    off, idx = C.brute_lists(d, rows, radius / C.DUP_PITCH)
    for i, row in enumerate(rows):
        neighbourhood(out, f"dup_{i}", d, C.DUP_PITCH, nr, row, idx[off[i]:off[i + 1]], radius, C.rotations(3, 7)[i], 5)
        names.append(f"dup_{i}")
    out["cases"] = np.array(names)
    out["versions"] = np.array([f"numpy {np.__version__}"])
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_shot_ties_host as H

    H.check_conditions(out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(names), "neighbourhoods")


if __name__ == "__main__":
    main()
