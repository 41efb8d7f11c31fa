"""K5 on lists that hold neighbours at equal distance (lattice clouds: tests/shot_ties_cases.py), against the contract: the ten
statements see the neighbours in ONE order, ascending rho and among bit-equal rho ascending index in the caller's cloud
(tests/shot_ties_numpy.py; the C oracle breaks its ties the same way, tests/test_shot_ties_host.py).  No row is left out of the
unfused comparison; where the engine computes the frame itself, the rows whose weighted covariance has two eigenvalues closer
than 1e-6 relative are (their frame is LAPACK's rounding), at most 5 % of them.  The same host module shows that the rows compared
here move by more than 1e-6 when the ties are turned round, and that nothing but the tie order is within 1e-9 of a decision."""
import functools

import numpy as np
import pytest

import shot_ties_cases as C
import shot_ties_numpy as T

pytestmark = pytest.mark.gpu

TOL = 1e-9  # the project's SHOT tolerance
GAP, GAP_SHARE = 1e-6, 0.05
K5_NAMES = ("k5_shot", "k5_shot_mid", "k5_shot_tail", "k5_shot_tail_stream", "k5_shot_bins")
ALL_CLASSES = list(C.CLASSES) + list(C.IMPORT_CLASSES)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as orc

    return orc


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


@functools.lru_cache(maxsize=None)
def _normals(kind):
    from oracle import oracle as orc

    return C.thin_normals(kind, lambda p: orc.compute_normals(p, p, radius=3.3 * C.PITCH))


def _x(cls):
    return C.CLASSES[cls][0] if cls in C.CLASSES else C.IMPORT_CLASSES[cls]


@functools.lru_cache(maxsize=None)
def _lists(cls):
    """keypoints (rows of the thinned lattice), CSR lists in ascending index, radius, one frame per cloud point"""
    x = _x(cls)
    kp = C.thin_keypoints(x)
    off, idx = C.thin_lists(x, kp)
    return kp, off, idx, C.check_radius(x), C.rotations(C.thinned_lattice()[1].shape[0], 2000 + int(100 * x))


def _launched(eng, fn):
    eng.profile(True)
    eng.profile_reset()
    try:
        res = fn()
        rep = eng.profile_report()
    finally:
        eng.profile(False)
    return res, tuple(sorted(n for n, (launches, _) in rep.items() if n in K5_NAMES and launches > 0))


def _search(cloud, cls, p, kp, off, idx, r):
    """The class's keypoints as external queries -- or, for the import classes, their lists handed in."""
    if cls in C.IMPORT_CLASSES:
        return cloud.import_neighbors(p[kp], [idx[off[i]:off[i + 1]] for i in range(len(kp))], r)
    return cloud.radius_search(p[kp], r)


def _gates(off):
    """A gate every list passes and one that the median list fails."""
    return 5, int(np.median(np.diff(off)))


def _worst(got, want):
    err = np.abs(got - want).max(axis=1)
    return float(err.max()), int((err >= TOL).sum()), int(err.argmax())


@pytest.mark.parametrize("cls", ALL_CLASSES)
def test_unfused_rows_are_the_contracts_and_the_same_bits_however_served(eng, O, cls):
    """nb.shot on frames handed in (seeded rotations) against the oracle on the same lists and frames: every kind of normals, both
    normalize values, a gate that passes and one that fails, every row.  Then, array_equal: the call five times over, and the
    class's keypoints served by a self search of the whole cloud (whose launches are asserted) against external queries."""
    _, p = C.thinned_lattice()
    kp, off, idx, r, frames = _lists(cls)
    for kind in C.NORMAL_KINDS:
        nr = _normals(kind)
        cloud, nb = eng.cloud(p, nr), None
        try:
            nb = _search(cloud, cls, p, kp, off, idx, r)
            assert np.array_equal(nb.counts(), np.diff(off)), cls
            for normalize in (True, False):
                for gate in _gates(off):
                    want = O.shot_lists(p, nr, p[kp], off, idx, r, frames[kp], normalize, gate)
                    (got, names) = _launched(eng, lambda: np.array(nb.shot(frames[kp], normalize, gate)))
                    zero = int((~want.any(axis=1)).sum())
                    print(cls, kind, normalize, gate, names, "zero rows", zero, "worst", _worst(got, want))
                    assert (zero == 0) if gate == 5 else (0 < zero < len(kp))
                    assert np.abs(got - want).max() < TOL, (cls, kind, normalize, gate, _worst(got, want))
                    if cls in C.IMPORT_CLASSES:
                        assert names == ("k5_shot",) and (nb.max_count > 256) == (cls == "import450"), (names, nb.max_count)
            first = np.array(nb.shot(frames[kp], True, 5))
            for _ in range(4):
                assert np.array_equal(np.array(nb.shot(frames[kp], True, 5)), first), (cls, kind)
            if cls in C.CLASSES and kind == "random":
                nb.free()
                nb = cloud.radius_search_self(r)
                perm = cloud.perm()
                assert np.array_equal(nb.counts(), C.thin_counts(_x(cls))[perm])
                rows, names = _launched(eng, lambda: np.array(nb.shot(frames[perm], True, 5)))
                assert names == C.CLASSES[cls][3], (cls, names)
                assert np.array_equal(rows[np.argsort(perm)[kp]], first), cls
        finally:
            if nb is not None:
                nb.free()
            cloud.free()


def _eigen_gaps(p, kp, off, idx, r):
    """Smallest relative gap between two eigenvalues of every keypoint's weighted covariance (shot.py:27-36)."""
    gaps = np.zeros(len(kp))
    for i, row in enumerate(kp):
        d = p[idx[off[i]:off[i + 1]]] - p[row]
        w = r - np.linalg.norm(d, axis=1)
        ev = np.linalg.eigvalsh(d.T @ (d * w[:, None]) / w.sum())
        gaps[i] = np.diff(ev).min() / ev[2]
    return gaps


def _fused(eng, nb, normalize, min_nb):
    d_rows, d_lrf = eng.empty((max(nb.m, 1), 352)), eng.empty((max(nb.m, 1), 9))
    try:
        nb.shot_single_scale(normalize, min_nb, out=d_rows, lrf_out=d_lrf)
        return d_rows.to_host()[: nb.m].copy(), d_lrf.to_host()[: nb.m].copy().reshape(-1, 3, 3)
    finally:
        d_rows.free()
        d_lrf.free()


@pytest.mark.parametrize("cls", ALL_CLASSES)
def test_fused_rows_are_the_contracts_on_the_frames_the_call_returned(eng, O, cls):
    _, p = C.thinned_lattice()
    kp, off, idx, r, _ = _lists(cls)
    ok = _eigen_gaps(p, kp, off, idx, r) >= GAP
    assert (~ok).mean() <= GAP_SHARE, (cls, int((~ok).sum()))
    want_lrf = O.shot_lrf_lists(p, p[kp], off, idx, r)
    for kind in C.NORMAL_KINDS:
        nr = _normals(kind)
        cloud, nb = eng.cloud(p, nr), None
        try:
            nb = _search(cloud, cls, p, kp, off, idx, r)
            for normalize in (True, False):
                rows, lrf = _fused(eng, nb, normalize, 5)
                assert np.abs(lrf - want_lrf)[ok].max() < TOL, (cls, kind, np.abs(lrf - want_lrf)[ok].max())
                want = O.shot_lists(p, nr, p[kp], off, idx, r, lrf, normalize, 5)
                print(cls, kind, normalize, "excluded", int((~ok).sum()), "worst", _worst(rows[ok], want[ok]))
                assert np.abs(rows - want)[ok].max() < TOL, (cls, kind, normalize, _worst(rows[ok], want[ok]))
                again, lrf2 = _fused(eng, nb, normalize, 5)
                assert np.array_equal(again, rows) and np.array_equal(lrf2, lrf), (cls, kind)
        finally:
            if nb is not None:
                nb.free()
            cloud.free()


def _serial_frames(O, p, kp, off, idx, r):
    """The serial variant's frames (shot.py:361-372): on the neighbours at non-zero distance only."""
    keep = np.ones(len(idx), dtype=bool)
    owner = np.repeat(np.arange(len(kp)), np.diff(off))
    keep &= ~(p[idx] == p[kp][owner]).all(axis=1)
    off2 = np.concatenate([[0], np.cumsum(np.bincount(owner[keep], minlength=len(kp)))]).astype(np.int64)
    return O.shot_lrf_lists(p, p[kp], off2, idx[keep], r)


@pytest.mark.parametrize("cls", ["c64", "c255", "team4"])
def test_serial_shot_at_11_and_12_bins(eng, O, cls):
    """shot_serial: the fixed form against O.compute_shot_descriptor, k_shot_bins at 11 and at 12 bins against the contract's
    statements with n bins on the serial variant's frames."""
    _, p = C.thinned_lattice()
    kp, off, idx, r, _ = _lists(cls)
    ok = _eigen_gaps(p, kp, off, idx, r) >= GAP
    assert (~ok).mean() <= GAP_SHARE
    nr = _normals("random")
    frames = _serial_frames(O, p, kp, off, idx, r)
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search(p[kp], r)
        want = O.compute_shot_descriptor(p[kp], p, nr, r, 5)
        (got, names) = _launched(eng, lambda: np.array(nb.shot_serial(5)))
        assert "k5_shot_bins" not in names and np.abs(got - want)[ok].max() < TOL, (cls, names, _worst(got[ok], want[ok]))
        for n in (11, 12):
            (got, names) = _launched(eng, lambda: np.array(nb.shot_serial(5, n_cosine_bins=n)))
            assert names == ("k5_shot_bins",) and got.shape == (len(kp), 32 * n)
            rows = np.flatnonzero(ok)[:: max(1, int(ok.sum()) // 24)]
            for i in rows:
                sl = idx[off[i]:off[i + 1]]
                one = T.shot_row(p[kp[i]], p[sl], nr[sl], r, frames[i], True, 5, T.contract_order, sl, n=n)
                assert np.abs(got[i] - one).max() < TOL, (cls, n, i, np.abs(got[i] - one).max())
            if n == 11:
                assert np.abs(got - want)[ok].max() < TOL, (cls, _worst(got[ok], want[ok]))
            assert np.array_equal(np.array(nb.shot_serial(5, n_cosine_bins=n)), got)
    finally:
        if nb is not None:
            nb.free()
        cloud.free()


def test_full_lattice_with_the_identity_frame(eng, O):
    """Every neighbour on a bin boundary, ties up to 48-fold: every point a keypoint, the identity handed in."""
    g, p, nr, _, r = C.full_lattice()
    cloud, nb = eng.cloud(p, nr), None
    try:
        nb = cloud.radius_search_self(r)
        perm = cloud.perm()
        eye = np.tile(np.eye(3), (len(p), 1, 1))
        assert 128 < nb.max_count <= 192
        for normalize in (True, False):
            want = O.shot(p, nr, p, r, eye, normalize, 5)
            got = np.array(nb.shot(eye, normalize, 5))[np.argsort(perm)]
            print("full lattice", normalize, _worst(got, want))
            assert want.any(axis=1).all() and np.abs(got - want).max() < TOL, _worst(got, want)
    finally:
        if nb is not None:
            nb.free()
        cloud.free()


def test_drop_ins_on_duplicated_points(O):
    from shot_fpfh_amd.descriptors import ShotMultiprocessor
    from shot_fpfh_amd.descriptors.shot import compute_shot_descriptor

    _, p, nr, r = C.duplicated_points()
    with ShotMultiprocessor(normalize=True, min_neighborhood_size=5, verbose=False) as sm:
        d = sm.compute_descriptor_single_scale(p, nr, p, r)
    want = O.shot_single_scale(p, nr, p, r, True, 5)
    assert want.any(axis=1).all() and np.abs(d - want).max() < TOL, _worst(d, want)
    d = compute_shot_descriptor(p, p, nr, r, min_neighborhood_size=5)
    want = O.compute_shot_descriptor(p, p, nr, r, 5)
    assert want.any(axis=1).all() and np.abs(d - want).max() < TOL, _worst(d, want)


def test_sharded_job_gives_the_unsharded_bits_on_the_thinned_lattice(eng):
    """DescriptorJob in neighbour mode at world 2 against the unsharded pass: array_equal."""
    from shot_fpfh_amd.sharding import DescriptorJob

    _, p = C.thinned_lattice()
    nr, r = _normals("random"), C.check_radius(C.CLASSES["c128"][0])
    one = DescriptorJob(eng, p, nr, r, n_bins=5, min_neighborhood_size=5)
    one.step()
    s1, l1, rows1 = one.shot_out.to_host(), one.lrf_out.to_host(), one.block_original_indices()
    one.close()
    assert s1.any(axis=1).all()
    for rank in range(2):
        job = DescriptorJob(eng, p, nr, r, n_bins=5, min_neighborhood_size=5, world=2, rank=rank, spfh_exchange="neighbor",
                            emulate_peers=True)
        job.step()
        b, e = job.plan.block()
        assert np.array_equal(job.block_original_indices(), rows1[b:e])
        assert np.array_equal(job.shot_out.to_host(), s1[b:e]) and np.array_equal(job.lrf_out.to_host(), l1[b:e])
        job.close()
