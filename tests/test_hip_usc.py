"""Unique Shape Context on the MI355X (K21) against its NumPy statement (tests/usc_numpy.py).

The statement is fed what the device itself produced in front of the kernel under test -- its frames (Neighbors.shot_lrf), its
exported lists, its weights -- and the library's own tables; the weights are checked on their own against 1.0 / c with c from the
statement's KDTree.  Unnormalised rows are then a matter of integer bin decisions and of one exactly rounded sum per bin:
they are compared by EXACT equality.  Normalised rows: within D 2^-53 relative (the norm is a sum of D non-negative terms in
another order)."""

import numpy as np
import pytest

import usc_numpy as U
from conftest import config1_cloud, family, synth_cloud
from shot_fpfh_amd import ShotFpfhError, _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from shot_fpfh_amd import default_engine

    return default_engine()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(engine, pts, kp, R, shape=(14, 14, 10), density=None, min_radius=None, frames=None, lists=None, normalize=False,
        min_nb=0, weights=None):
    """(device rows, frames used, lists in the caller's numbering, weights used) of one layered call: weights FIRST (the pass
    rebuilds the grid), then the search (or the import of `lists`), the frames, the rows."""
    L, K, J = shape
    cloud = engine.cloud(pts)
    try:
        w = cloud.usc_weights(R / 5 if density is None else density) if weights is None else weights
        nb = cloud.radius_search(kp, R) if lists is None else cloud.import_neighbors(kp, lists, R)
        try:
            lrf = nb.shot_lrf() if frames is None else np.ascontiguousarray(frames, dtype=np.float64)
            rows = np.array(nb.usc(w, R / 10 if min_radius is None else min_radius, lrf=lrf, azimuth_bins=L, elevation_bins=K,
                                   radius_bins=J, normalize=normalize, min_neighborhood_size=min_nb))
            off, idx = nb.export()
        finally:
            nb.free()
    finally:
        cloud.free()
    return rows, lrf.reshape(-1, 3, 3), [idx[off[i]:off[i + 1]] for i in range(kp.shape[0])], w


def check_exact(engine, pts, kp, R, shape=(14, 14, 10), **kw):
    rows, lrf, lists, w = run(engine, pts, kp, R, shape, **kw)
    L, K, J = shape
    want = U.rows(pts, kp, lists, lrf, w, R, kw.get("min_radius"), L, K, J, min_neighborhood_size=kw.get("min_nb", 0))
    assert rows.shape == want.shape == (kp.shape[0], L * K * J)
    wrong = np.flatnonzero((bits(rows) != bits(want)).any(axis=1))
    assert wrong.size == 0, (wrong[:5], [len(lists[i]) for i in wrong[:5]])
    return rows, lists, w


def _pick(pts, m, seed=3):
    return pts[np.sort(np.random.default_rng(seed).choice(pts.shape[0], min(m, pts.shape[0]), replace=False))]


# ---- the families -------------------------------------------------------------------------------------------------------------
FAMILY = {
    # name: (points, radius)
    "uniform": (lambda: family("uniform", 5000, np.random.default_rng(1))[0], 0.1),
    "noisy_sphere": (lambda: config1_cloud(5000, 2)[0], 0.12),
    "clustered": (lambda: family("clustered", 5000, np.random.default_rng(1))[0], 0.06),
    "duplicates": (lambda: family("duplicates", 5000, np.random.default_rng(1))[0], 0.1),
    "far_origin": (lambda: family("far_origin", 5000, np.random.default_rng(1))[0], 0.1),
    "three_points": (lambda: synth_cloud(3, 7)[0], 2.0),
}


@pytest.mark.parametrize("name", list(FAMILY))
def test_rows_equal_the_statement_bit_for_bit(engine, name):
    make, R = FAMILY[name]
    pts = make()
    kp = _pick(pts, 300)
    rows, lists, w = check_exact(engine, pts, kp, R)
    sizes = np.array([len(a) for a in lists])
    assert rows.any() and np.isfinite(rows).all() and (rows >= 0).all()
    if name == "clustered":
        assert (sizes > 255).sum() >= 20 and (sizes <= 64).sum() >= 5  # several steps of 128, and single ones
    if name == "duplicates":  # r2 == 0 skipped: a keypoint's duplicates carry no mass
        dup = [i for i, a in enumerate(lists) if ((pts[a] - kp[i]) ** 2).sum(axis=1).tolist().count(0.0) > 1]
        assert len(dup) >= 20
    if name == "three_points":
        assert sizes.tolist() == [3, 3, 3] and (np.count_nonzero(rows, axis=1) <= 2).all()


def test_lattice_with_identity_frames_meets_every_tie_rule(engine):
    """Spacing 1/16 and the identity frame: offsets along the axes and in the coordinate planes, so lx = 0, ly = 0, lz = 0, the
    azimuth edges at 0 and pi and the equator all occur, together with neighbours exactly on the radius."""
    pts = family("lattice", 4096, np.random.default_rng(1))[0]
    kp = _pick(pts, 200)
    R = 0.125  # two spacings, on-radius points included
    frames = np.tile(np.eye(3).reshape(1, 9), (kp.shape[0], 1))
    rows, lists, w = check_exact(engine, pts, kp, R, frames=frames)
    d = np.vstack([pts[a] - kp[i] for i, a in enumerate(lists)])
    r2 = (d ** 2).sum(axis=1)
    assert (r2 == R * R).any() and (r2 == 0).any()
    for axis in range(3):
        assert ((d[:, axis] == 0) & (r2 > 0)).any()
    assert ((d[:, 1] == 0) & (d[:, 0] < 0)).any() and ((d[:, 0] == 0) & (d[:, 1] == 0) & (r2 > 0)).any()
    check_exact(engine, pts, kp[:50], R, shape=(4, 2, 1), frames=frames[:50])  # (edges ON the axes: pi / 2, pi, the equator)


def test_keypoints_outside_the_cloud_get_rows_of_zeros(engine):
    pts = synth_cloud(2000, 5)[0]
    kp = np.vstack([pts[:5], pts[:20] + 10.0])
    rows, lists, w = check_exact(engine, pts, kp, 0.1)
    assert all(len(a) == 0 for a in lists[5:]) and not rows[5:].any() and rows[:5].any()


@pytest.mark.parametrize("min_nb", [0, 40, 10 ** 9, -5])
def test_the_gate_counts_neighbours_at_non_zero_distance(engine, min_nb):
    pts = synth_cloud(3000, 5)[0]
    kp = _pick(pts, 100)
    rows, lists, w = check_exact(engine, pts, kp, 0.15, min_nb=min_nb)
    sizes = np.array([len(a) - 1 for a in lists])  # (every keypoint is a cloud point without duplicates)
    assert np.array_equal(rows.any(axis=1), sizes > max(min_nb, 0))
    if min_nb == 40:
        assert 5 < (sizes > 40).sum() < 95


# ---- list lengths around the steps of 128 --------------------------------------------------------------------------------
def test_imported_lists_of_every_length_around_a_step(engine):
    lengths = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
    pts = synth_cloud(400, 9)[0]
    rng = np.random.default_rng(10)
    kp = pts[: len(lengths)] + 1e-3  # (off the cloud: every entry of a list is at non-zero distance)
    lists = [rng.permutation(400)[:n] for n in lengths]
    R = 0.6  # (what the tables are made for; some entries lie beyond it: last radial bin)
    rows, got_lists, w = check_exact(engine, pts, kp, R, lists=lists, density=0.15)
    assert [len(a) for a in got_lists] == lengths
    assert not rows[0].any() and np.count_nonzero(rows[1]) == 1
    far = [(((pts[a] - kp[i]) ** 2).sum(axis=1) > R * R).sum() for i, a in enumerate(got_lists)]
    assert max(far) > 10


# ---- neighbours exactly on the radial edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(14, 14, 10), (12, 11, 15)])
def test_neighbours_on_the_radial_edges(engine, shape):
    """d = (e[j], 0, 0) from a keypoint at the origin, identity frame: r2 == e2[j] exactly (sqrt(x x) = |x|), so the point belongs
    to radial bin j (>=), the one at r = R to the last bin; its neighbour one ulp nearer to bin j - 1."""
    L, K, J = shape
    R, r0 = 0.5, 0.05
    e2 = U.tables(R, r0, L, K, J)[0]
    e = np.sqrt(e2)
    assert np.array_equal(e * e, e2) and e[J] == R
    on = np.column_stack([e, np.zeros(J + 1), np.zeros(J + 1)])
    below = np.column_stack([np.nextafter(e, 0.0), np.full(J + 1, 0.0), np.zeros(J + 1)])
    filler = synth_cloud(200, 3)[0] - 0.5
    pts = np.vstack([np.zeros((1, 3)), on, below, filler])
    kp = np.zeros((1, 3))
    lists = [np.arange(1, 2 * (J + 1) + 1)]
    weights = np.ones(pts.shape[0])
    rows, _, _ = check_exact(engine, pts, kp, R, shape=shape, min_radius=r0, frames=np.eye(3).reshape(1, 9), lists=lists, weights=weights)
    vol = U.tables(R, r0, L, K, J)[4]
    k_eq = sum(1 for i in range(1, K) if 0.0 <= U.tables(R, r0, L, K, J)[3][i])  # lz = 0: k = #{q[i] >= 0}
    mass = np.zeros(J)
    for j in range(J + 1):
        mass[min(j, J - 1)] += 1  # on the edge: bin j (the last edge: the last bin)
        mass[min(max(j - 1, 0), J - 1)] += 1  # one ulp below: bin j - 1 (below r0: bin 0)
    want = np.zeros(L * K * J)
    want[(0 * K + k_eq) * J + np.arange(J)] = mass * vol[(0 * K + k_eq) * J + np.arange(J)]
    assert np.array_equal(bits(rows[0]), bits(want))
    check_exact(engine, pts, _pick(pts, 50), R, shape=shape, min_radius=r0, density=0.1)  # (and the same cloud searched)


# ---- bin shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(14, 14, 10), (12, 11, 15), (2, 1, 1), (4, 2, 1), (16, 16, 16)])
def test_bin_shapes(engine, shape):
    pts = config1_cloud(4000, 4)[0]
    kp = _pick(pts, 150)
    rows, lists, w = check_exact(engine, pts, kp, 0.15, shape=shape)
    assert np.count_nonzero(rows.any(axis=0)) > 0.3 * rows.shape[1] or shape[0] * shape[1] * shape[2] > 1000


def test_shapes_above_the_cap_and_bad_arguments_are_refused(engine):
    pts = synth_cloud(500, 1)[0]
    cloud = engine.cloud(pts)
    try:
        w = cloud.usc_weights(0.05)
        nb = cloud.radius_search(pts[:10], 0.2)
        try:
            for L, K, J in ((16, 16, 17), (4098, 1, 1), (13, 14, 10), (0, 1, 1), (2, 0, 1), (2, 1, 0)):
                with pytest.raises(ValueError):
                    nb.usc(w, 0.02, azimuth_bins=L, elevation_bins=K, radius_bins=J)
                out = np.zeros(10 * 5000)
                rc = engine.lib.sf_usc(engine.h, cloud.h, nb.h, None, w.ctypes.data, 0.02, L, K, J, 0, 0, out.ctypes.data, 0)
                assert rc == -1 and "sf_usc:" in _ffi.last_error()
            for r0 in (0.0, 0.2, 0.3, -1.0, float("nan")):
                with pytest.raises(ShotFpfhError, match=r"\(-1\)"):
                    nb.usc(w, r0)
            with pytest.raises(ValueError):
                nb.usc(w[:-1], 0.02)
            with pytest.raises(ValueError):
                nb.usc(w, 0.02, lrf=np.zeros((9, 3, 3)))
            assert nb.usc(w, 0.02).shape == (10, 1960)
            stale = cloud.usc_weights(0.05)  # rebuilds the grid: the lists of before are refused
            with pytest.raises(ShotFpfhError, match=r"\(-5\)"):
                nb.usc(stale, 0.02)
        finally:
            nb.free()
    finally:
        cloud.free()


# ---- the weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, radius", [("uniform", 0.05), ("lattice", 0.125), ("far_origin", 0.04), ("duplicates", 0.03),
                                          ("clustered", 0.02)])
def test_weights_are_exactly_one_over_the_ball_count(engine, name, radius):
    pts = family(name, 4096 if name == "lattice" else 5000, np.random.default_rng(1))[0]
    cloud = engine.cloud(pts)
    try:
        w = cloud.usc_weights(radius)
        dev = engine.empty((cloud.n,))
        try:
            assert np.array_equal(bits(cloud.usc_weights(radius, out=dev).to_host()), bits(w))
        finally:
            dev.free()
    finally:
        cloud.free()
    want = U.density_weights(pts, radius)
    assert w.shape == want.shape and np.array_equal(bits(w), bits(want))
    assert w.max() <= 1.0 and w.min() > 0.0
    if name == "duplicates":  # (the first fifth occurs three times)
        assert (w[: pts.shape[0] // 5] <= 1.0 / 3.0).all()


def test_a_weight_out_of_range_is_an_argument_error(engine):
    pts = synth_cloud(1000, 2)[0]
    cloud = engine.cloud(pts)
    try:
        w = cloud.usc_weights(0.05)
        nb = cloud.radius_search(pts, 0.2)  # (point 17 lies in dozens of lists)
        try:
            for bad in (2.0, 0.0, -0.25, 2.0 ** -23, float("nan"), float("inf")):
                wb = w.copy()
                wb[17] = bad
                with pytest.raises(ShotFpfhError, match=r"\(-1\).*weight"):
                    nb.usc(wb, 0.01)
            wb = w.copy()
            wb[17], wb[18] = 1.0, 2.0 ** -22  # the ends of the range are weights
            assert np.isfinite(nb.usc(wb, 0.01)).all()
        finally:
            nb.free()
    finally:
        cloud.free()


# ---- normalised rows, repeatability, the public function ------------------------------------------------------------------------
def test_normalised_rows(engine):
    pts = config1_cloud(5000, 2)[0]
    kp = np.vstack([_pick(pts, 200), pts[:3] + 5.0])
    D = 1960
    rows, lrf, lists, w = run(engine, pts, kp, 0.12, normalize=True)
    want = U.rows(pts, kp, lists, lrf, w, 0.12, normalize=True)
    err = np.abs(rows - want)
    print("largest relative error of a normalised entry: %.3g (bound %.3g)" % ((err[want > 0] / want[want > 0]).max(), D * 2.0 ** -53))
    assert (err <= D * 2.0 ** -53 * np.abs(want)).all()
    assert np.array_equal(rows == 0, want == 0) and not rows[-3:].any()
    assert np.allclose(np.linalg.norm(rows[:-3], axis=1), 1.0, rtol=1e-13, atol=0)


def test_a_call_repeats_and_a_shuffled_cloud_gives_the_same_bits(engine):
    pts = family("clustered", 5000, np.random.default_rng(1))[0]
    kp = _pick(pts, 200)
    first, lrf, lists, w = run(engine, pts, kp, 0.06)
    again, _, _, _ = run(engine, pts, kp, 0.06, frames=lrf)
    assert np.array_equal(bits(first), bits(again))
    order = np.random.default_rng(8).permutation(pts.shape[0])
    shuffled, _, lists2, w2 = run(engine, pts[order], kp, 0.06, frames=lrf)
    assert np.array_equal(bits(w2), bits(w[order]))
    assert np.array_equal(bits(first), bits(shuffled))


def test_public_function_equals_the_layered_calls(engine):
    from shot_fpfh_amd.descriptors import compute_usc_descriptor

    pts = config1_cloud(5000, 2)[0]
    kp = _pick(pts, 200)
    R = 0.12
    rows, _, _, _ = run(engine, pts, kp, R)
    assert np.array_equal(bits(compute_usc_descriptor(pts, kp, R)), bits(rows))
    # every parameter, the frames from lists at another radius
    cloud = engine.cloud(pts)
    try:
        support = cloud.radius_search(kp, 0.2)
        lrf = support.shot_lrf()
        support.free()
    finally:
        cloud.free()
    layered, _, _, _ = run(engine, pts, kp, R, shape=(12, 11, 15), density=0.03, min_radius=0.02, frames=lrf, normalize=True, min_nb=30)
    public = compute_usc_descriptor(pts, kp, R, min_radius=0.02, density_radius=0.03, azimuth_bins=12, elevation_bins=11,
                                    radius_bins=15, local_rf_radius=0.2, normalize=True, min_neighborhood_size=30)
    assert public.shape == (200, 12 * 11 * 15) and np.array_equal(bits(public), bits(layered))
    assert compute_usc_descriptor(pts, np.zeros((0, 3)), R).shape == (0, 1960)
    assert compute_usc_descriptor(np.zeros((0, 3)), kp[:4], R).shape == (4, 1960)


def test_pipeline_choice_usc_and_matching_at_1960(engine):
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    p, n = config1_cloud(6000, 5)
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(6)
    pipe = RegistrationPipeline(scan=p @ rot.T, scan_normals=n @ rot.T, ref=p, ref_normals=n)
    pipe.scan_keypoints = np.sort(rng.choice(6000, 300, replace=False))
    pipe.ref_keypoints = np.sort(rng.choice(6000, 300, replace=False))
    with pytest.raises(ValueError):
        pipe.compute_descriptors(0.2, descriptor_choice="nope")
    pipe.compute_descriptors(0.2, descriptor_choice="usc")
    sd, rd = pipe.scan_descriptors, pipe.ref_descriptors
    assert sd.shape == rd.shape == (300, 1960) and sd.any(axis=1).all() and rd.any(axis=1).all()
    from shot_fpfh_amd.descriptors import compute_usc_descriptor

    assert np.array_equal(bits(rd), bits(compute_usc_descriptor(p, p[pipe.ref_keypoints], 0.2)))
    pipe.find_descriptors_matches("simple", reject_threshold=0.8, threshold_multiplier=10)
    best = np.array([np.argmin(((rd - row) ** 2).sum(axis=1)) for row in sd])
    assert np.array_equal(pipe.matches[0], np.arange(300)) and np.array_equal(pipe.matches[1], best)
