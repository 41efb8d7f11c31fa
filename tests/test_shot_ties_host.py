"""SHOT rows of lists that hold neighbours at equal distance: the contract, checked without a device.

The contract (tests/shot_ties_numpy.py): the ten statements see the neighbours in ONE order, ascending rho and
among bit-equal rho ascending index in the caller's cloud.  Here:
  * the NumPy statement of the reference, given the permutation the reference's own np.argsort(rho) produced
    (tests/golden/shot_ties.npz, tools/gen_golden_shot_ties.py), reproduces the reference's row bit for bit: it treats a tie as
    the reference does once an order is given;
  * with `contract_order` it equals the C oracle (O.shot_single / O.shot), to the tolerance test_oracle_golden.py holds the
    oracle's SHOT rows to;
  * the rows the GPU tests compare DEPEND on the tie order: with the ties turned round at least half of them move by more
    than 1e-6, in every cloud, kind of normals and length class;
  * nothing else is on trial: every bin-deciding quantity of every compared neighbour stays clear of its edge by more than 1e-9
    (the identity-frame case apart: its edges are the reference's exact rules, which shot_boundary.npz covers)."""
import numpy as np
import pytest

import shot_ties_cases as C
import shot_ties_numpy as T
from conftest import load_golden

GOLDEN = "shot_ties.npz"
TOL = 1e-12  # test_oracle_golden.py's: oracle vs reference, same arithmetic up to summation order
MOVED, CLEAR = 1e-6, 1e-9


def _case(g, name):
    pitch = float(g[f"{name}_pitch"][0])
    return dict(point=g[f"{name}_point"].astype(np.float64) * pitch, pts=g[f"{name}_ijk"].astype(np.float64) * pitch,
                nrm=g[f"{name}_normals"], radius=float(g[f"{name}_radius"][0]), frame=g[f"{name}_frame"],
                min_nb=int(g[f"{name}_min_nb"][0]), index=g[f"{name}_index"], order=g[f"{name}_order"])


def _row(c, normalize, order_fn, details=None):
    return T.shot_row(c["point"], c["pts"], c["nrm"], c["radius"], c["frame"], normalize, c["min_nb"], order_fn, c["index"], details)


def check_conditions(g):
    """What the golden file is for (the generator asserts it while recording, the test on the file)."""
    names = [str(n) for n in g["cases"]]
    assert 36 <= len(names) <= 48 and "full_identity" in names
    groups = {}
    for name in names:
        c = _case(g, name)
        for n in (0, 1):
            assert np.array_equal(_row(c, bool(n), T.recorded(c["order"])), g[f"{name}_row{n}"]), (name, n)
        det = {}
        a, b = _row(c, True, T.contract_order, det), _row(c, True, T.reversed_ties)
        groups.setdefault(name.rsplit("_", 1)[0] if name != "full_identity" else name, []).append(np.abs(a - b).max())
        if name != "full_identity":
            assert T.edge_margin(det, c["radius"]) > CLEAR, (name, T.edge_margin(det, c["radius"]))
    for grp, moved in groups.items():
        assert 2 * sum(m > MOVED for m in moved) >= len(moved), (grp, moved)


def test_transcription_reproduces_the_reference_and_the_golden_is_what_it_is_for():
    check_conditions(load_golden(GOLDEN))


def test_oracle_agrees_with_the_contract_on_the_golden_neighbourhoods():
    from oracle import oracle as O

    g = load_golden(GOLDEN)
    for name in (str(n) for n in g["cases"]):
        c = _case(g, name)
        for normalize in (True, False):
            want = _row(c, normalize, T.contract_order)
            got = O.shot_single(c["point"], c["pts"], c["nrm"], c["radius"], c["frame"], normalize, c["min_nb"])
            assert want.any() and np.abs(got - want).max() < TOL, (name, normalize, np.abs(got - want).max())


def estimated_normals(points):
    from oracle import oracle as O

    return O.compute_normals(points, points, radius=3.3 * C.PITCH)


def lattice_margin(points, normals, kp, off, idx, frames, radius):
    """edge_margin of shot_ties_numpy over the lists of many keypoints at once (the same quantities, vectorised)."""
    owner = np.repeat(np.arange(len(kp)), np.diff(off))
    d = points[idx] - points[kp][owner]
    rho = np.linalg.norm(d, axis=1)
    keep = rho > 0
    loc = np.einsum("ni,nij->nj", d, frames[owner])[keep]
    cpos = (np.clip(np.einsum("ni,ni->n", normals[idx], frames[owner][:, :, 2]), -1, 1)[keep] + 1.0) * 11 / 2.0 - 0.5
    geo = np.minimum.reduce([np.abs(loc[:, 0]), np.abs(loc[:, 1]), np.abs(loc[:, 2]), np.abs(np.abs(loc[:, 0]) - np.abs(loc[:, 1])),
                             np.abs(rho[keep] - radius / 2)]) / radius
    return float(min(geo.min(), np.abs(cpos - np.floor(cpos) - 0.5).min()))


def reversed_rows(O, points, normals, kp, off, idx, radius, frames, normalize, min_nb):
    """The oracle with every list handed over in DESCENDING index: it breaks ties by list position, so this is the contract
    with the ties turned round."""
    rev = np.concatenate([idx[off[i]:off[i + 1]][::-1] for i in range(len(kp))]) if len(kp) else idx
    return O.shot_lists(points, normals, points[kp], off, rev, radius, frames, normalize, min_nb)


@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_lattice_classes_have_the_lists_they_are_named_for(cls):
    x, lo, hi, _ = C.CLASSES[cls]
    cnt = C.thin_counts(x)
    assert lo <= cnt.max() <= hi, (cls, cnt.max())
    kp = C.thin_keypoints(x)
    assert 0 < len(kp) <= C.MAX_KEYPOINTS and cnt[kp].min() > 20
    if cls == "mid":
        assert 0 < (cnt > 64).mean() <= 0.02


@pytest.mark.parametrize("kind", C.NORMAL_KINDS)
@pytest.mark.parametrize("cls", list(C.CLASSES))
def test_compared_rows_depend_on_the_tie_order_and_on_nothing_else(cls, kind):
    from oracle import oracle as O

    x = C.CLASSES[cls][0]
    radius = C.check_radius(x)
    _, p = C.thinned_lattice()
    nr = C.thin_normals(kind, estimated_normals)
    kp = C.thin_keypoints(x)
    off, idx = C.thin_lists(x, kp)
    frames = C.rotations(len(kp), 1000 + int(100 * x))
    assert lattice_margin(p, nr, kp, off, idx, frames, radius) > CLEAR
    a = O.shot_lists(p, nr, p[kp], off, idx, radius, frames, True, 5)
    b = reversed_rows(O, p, nr, kp, off, idx, radius, frames, True, 5)
    moved = np.abs(a - b).max(axis=1)
    assert 2 * (moved > MOVED).sum() >= len(kp), (cls, kind, int((moved > MOVED).sum()), len(kp), float(np.median(moved)))
    # the oracle is the contract on these lists too (a few keypoints: the NumPy form walks a list in milliseconds)
    for i in range(0, len(kp), max(1, len(kp) // 4)):
        sl = idx[off[i]:off[i + 1]]
        want = T.shot_row(p[kp[i]], p[sl], nr[sl], radius, frames[i], True, 5, T.contract_order, sl)
        assert np.abs(a[i] - want).max() < TOL, (cls, kind, i, np.abs(a[i] - want).max())


def test_full_lattice_and_duplicated_points_depend_on_the_tie_order():
    from oracle import oracle as O

    g, p, nr, row, radius = C.full_lattice()
    off, idx = C.brute_lists(g, np.array([row]), C.FULL_X)
    eye = np.eye(3)[None]
    a = O.shot_lists(p, nr, p[[row]], off, idx, radius, eye, True, 5)
    b = reversed_rows(O, p, nr, np.array([row]), off, idx, radius, eye, True, 5)
    assert np.abs(a - b).max() > MOVED
    d, p, nr, radius = C.duplicated_points()
    kp = np.arange(len(p))
    off, idx = C.brute_lists(d, kp, radius / C.DUP_PITCH)
    frames = C.rotations(len(kp), 77)
    assert lattice_margin(p, nr, kp, off, idx, frames, radius) > CLEAR
    a = O.shot_lists(p, nr, p[kp], off, idx, radius, frames, True, 5)
    b = reversed_rows(O, p, nr, kp, off, idx, radius, frames, True, 5)
    assert 2 * (np.abs(a - b).max(axis=1) > MOVED).sum() >= len(kp)
