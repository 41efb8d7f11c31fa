"""Point Feature Histograms on the MI355X (K22) against their NumPy statement (tests/pfh_numpy.py).

The statement is fed the lists the device itself exported (or the ones it was given) and the library's own tables.  A row is then
a matter of integer bin decisions, one exact product and one correctly rounded division: rows are compared by EXACT equality."""

import numpy as np
import pytest

import pfh_numpy as P
from conftest import config1_cloud, family, synth_cloud
from shot_fpfh_amd import ShotFpfhError, _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from shot_fpfh_amd import default_engine

    return default_engine()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(engine, pts, nrm, kp, R, S=5, lists=None):
    """(device rows, lists in the caller's numbering) of one layered call: the search (or the import of `lists`), the rows."""
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(kp, R) if lists is None else cloud.import_neighbors(kp, lists, R)
        try:
            rows = np.array(nb.pfh(S))
            off, idx = nb.export()
        finally:
            nb.free()
    finally:
        cloud.free()
    return rows, [idx[off[i]:off[i + 1]] for i in range(kp.shape[0])]


def check_exact(engine, pts, nrm, kp, R, S=5, lists=None):
    rows, got_lists = run(engine, pts, nrm, kp, R, S, lists)
    want = P.rows(pts, nrm, got_lists, S)
    assert rows.shape == want.shape == (kp.shape[0], S ** 3)
    wrong = np.flatnonzero((bits(rows) != bits(want)).any(axis=1))
    assert wrong.size == 0, (wrong[:5], [len(got_lists[i]) for i in wrong[:5]])
    return rows, got_lists


def _pick(pts, m, seed=3):
    return pts[np.sort(np.random.default_rng(seed).choice(pts.shape[0], min(m, pts.shape[0]), replace=False))]


def _lattice():
    pts = family("lattice", 4096, np.random.default_rng(1))[0]
    return pts, np.tile(np.array([1.0, 2.0, 2.0]) / 3.0, (pts.shape[0], 1))  # one tilted normal: every source is a tie


# ---- the families -------------------------------------------------------------------------------------------------------------
FAMILY = {
    # name: (points and normals, radius)
    "uniform": (lambda: family("uniform", 5000, np.random.default_rng(1))[:2], 0.14),
    "noisy_sphere": (lambda: config1_cloud(5000, 2), 0.12),
    "clustered": (lambda: family("clustered", 5000, np.random.default_rng(1))[:2], 0.03),
    "lattice_tilted_normal": (_lattice, 0.125),
    "duplicates": (lambda: family("duplicates", 5000, np.random.default_rng(1))[:2], 0.14),
    "far_origin": (lambda: family("far_origin", 5000, np.random.default_rng(1))[:2], 0.14),
    "three_points": (lambda: synth_cloud(3, 7)[:2], 2.0),
}


@pytest.mark.parametrize("name", list(FAMILY))
def test_rows_equal_the_statement_bit_for_bit(engine, name):
    make, R = FAMILY[name]
    pts, nrm = make()
    kp = _pick(pts, 200)
    rows, lists = check_exact(engine, pts, nrm, kp, R)
    sizes = np.array([len(a) for a in lists])
    print(name, "list lengths: min %d, median %d, max %d" % (sizes.min(), np.median(sizes), sizes.max()))
    assert rows.any() and np.isfinite(rows).all() and (rows >= 0).all() and (rows.sum(axis=1) <= 100.0 + 1e-9).all()
    if name == "clustered":
        assert (sizes > 128).sum() >= 10 and (sizes <= 64).sum() >= 5  # the streaming form, and single chunks
    elif name != "three_points":
        assert 30 <= np.median(sizes) <= 100
    if name == "lattice_tilted_normal":
        f = P.list_pairs(pts, nrm, lists[np.argmax(sizes)])
        assert (f["branch"] > 0).all() and (f["branch"] == 1).any() and (f["branch"] == 2).any() and (~f["keep"]).any()
    if name == "duplicates":  # d2 == 0 skipped, counted in P
        skipped = [int((~P.list_pairs(pts, nrm, a)["keep"]).sum()) for a in lists[:40]]
        assert sum(1 for s in skipped if s > 0) >= 10
    if name == "three_points":
        assert sizes.tolist() == [3, 3, 3] and np.array_equal(bits(rows[0]), bits(rows[1])) and abs(rows[0].sum() - 100.0) < 1e-9


def test_keypoints_outside_the_cloud_get_rows_of_zeros(engine):
    pts, nrm, _ = synth_cloud(2000, 5)
    kp = np.vstack([pts[:5], pts[:20] + 10.0])
    rows, lists = check_exact(engine, pts, nrm, kp, 0.2)
    assert all(len(a) == 0 for a in lists[5:]) and not rows[5:].any() and rows[:5].any()


# ---- list lengths around the chunk of 64, the stage of 128 and the tiles of 64 ---------------------------------------------------
def test_imported_lists_of_every_length_around_a_chunk_a_stage_and_a_tile(engine):
    lengths = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 300, 1000]
    pts, nrm, _ = synth_cloud(1200, 9)
    rng = np.random.default_rng(10)
    kp = pts[: len(lengths)] + 1e-3
    lists = [rng.permutation(1200)[:n] for n in lengths]
    rows, got = check_exact(engine, pts, nrm, kp, 0.6, lists=lists)
    assert [len(a) for a in got] == lengths
    assert not rows[0].any() and not rows[1].any() and np.count_nonzero(rows[2]) == 1 and rows[2].max() == 100.0
    assert (np.abs(rows[2:].sum(axis=1) - 100.0) < 1e-9).all()  # (no pair of distinct random points is skipped)


def test_repeated_entries_in_a_list_are_skipped_pairs(engine):
    pts, nrm, _ = synth_cloud(300, 11)
    lists = [np.r_[np.arange(150), np.arange(100)], np.full(70, 5), np.r_[np.arange(200), np.arange(200)]]
    rows, _ = check_exact(engine, pts, nrm, pts[:3], 0.5, lists=lists)
    assert not rows[1].any() and rows[0].any() and rows[0].sum() < 100.0


# ---- bin counts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 8, 11, 16])
def test_bin_counts(engine, S):
    pts, nrm = config1_cloud(4000, 4)
    kp = _pick(pts, 150)
    rows, lists = check_exact(engine, pts, nrm, kp, 0.15, S=S)
    assert rows.any(axis=1).all()
    if S == 1:
        assert (rows == 100.0).all()


def test_bin_counts_out_of_range_and_a_cloud_without_normals_are_refused(engine):
    pts, nrm, _ = synth_cloud(500, 1)
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(pts[:10], 0.2)
        try:
            out = np.zeros(10 * 17 ** 3)
            for S in (0, 17, -2):
                with pytest.raises(ValueError):
                    nb.pfh(S)
                assert engine.lib.sf_pfh(engine.h, cloud.h, nb.h, S, out.ctypes.data, 0) == -1 and "sf_pfh:" in _ffi.last_error()
            assert engine.lib.sf_pfh(engine.h, cloud.h, nb.h, 5, None, 0) == -1
            assert nb.pfh().shape == (10, 125) and nb.pfh(16).shape == (10, 4096)
        finally:
            nb.free()
    finally:
        cloud.free()
    bare = engine.cloud(pts)
    try:
        nb = bare.radius_search(pts[:10], 0.2)
        try:
            with pytest.raises(ShotFpfhError, match=r"\(-5\).*normals"):
                nb.pfh()
        finally:
            nb.free()
    finally:
        bare.free()


def test_a_list_of_65536_entries_is_refused(engine):
    """Through an imported list of repeated indices: the kernel does not walk it (it raises the error word), so the call
    takes as long as the import.  The longest list that is served, 65 535 entries, is 2 x 10^9 pairs on one wave and is not run."""
    pts, nrm, _ = synth_cloud(300, 12)
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.import_neighbors(pts[:2], [np.arange(40), np.arange(P.MAX_LIST) % 300], 0.5)
        try:
            with pytest.raises(ShotFpfhError, match=r"\(-1\).*entries"):
                nb.pfh()
        finally:
            nb.free()
    finally:
        cloud.free()


# ---- pairs exactly on edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 4, 5, 8, 16])
def test_pairs_exactly_on_edges(engine, S):
    pts, nrm, lists, want = P.near_edge_fixture(S)
    kp = pts[0::2]
    rows, _ = check_exact(engine, pts, nrm, kp, 2.0, S=S, lists=lists)
    got = np.argmax(rows, axis=1)
    assert (rows.max(axis=1) == 100.0).all() and (np.count_nonzero(rows, axis=1) == 1).all()
    for i, w in enumerate(want):
        b = (got[i] % S, got[i] // S % S, got[i] // (S * S))
        assert all(e is None or h == e for h, e in zip(b, w)), (i, b, w)
    check_exact(engine, pts, nrm, kp, 1.5, S=S)  # (and the same cloud searched: the pairs alone in their balls)


# ---- repeatability, the public function, device output, the pipeline ----------------------------------------------------------------
def test_a_call_repeats_and_a_shuffled_cloud_gives_the_same_bits(engine):
    pts, nrm = family("clustered", 5000, np.random.default_rng(1))[:2]
    kp = _pick(pts, 200)
    first, _ = run(engine, pts, nrm, kp, 0.02)
    again, _ = run(engine, pts, nrm, kp, 0.02)
    assert np.array_equal(bits(first), bits(again))
    order = np.random.default_rng(8).permutation(pts.shape[0])
    shuffled, _ = run(engine, pts[order], nrm[order], kp, 0.02)
    assert np.array_equal(bits(first), bits(shuffled))


def test_public_function_equals_the_layered_calls(engine):
    from shot_fpfh_amd.descriptors import compute_pfh_descriptor

    pts, nrm = config1_cloud(5000, 2)
    idx = np.sort(np.random.default_rng(3).choice(5000, 200, replace=False))
    R = 0.12
    rows, _ = run(engine, pts, nrm, pts[idx], R)
    assert np.array_equal(bits(compute_pfh_descriptor(idx, pts, nrm, R)), bits(rows))
    mask = np.zeros(5000, dtype=bool)
    mask[idx] = True
    assert np.array_equal(bits(compute_pfh_descriptor(mask, pts, nrm, R, 5, engine=engine)), bits(rows))
    rows8, _ = run(engine, pts, nrm, pts[idx[:50]], R, S=8)
    assert np.array_equal(bits(compute_pfh_descriptor(idx[:50], pts, nrm, radius=R, n_bins=8)), bits(rows8))


def test_device_output_equals_host_output(engine):
    pts, nrm = config1_cloud(3000, 6)
    kp = _pick(pts, 100)
    cloud = engine.cloud(pts, nrm)
    try:
        nb = cloud.radius_search(kp, 0.15)
        try:
            host = np.array(nb.pfh())
            dev = engine.empty((100, 125))
            try:
                assert nb.pfh(out=dev) is dev
                assert np.array_equal(bits(dev.to_host()), bits(host))
                with pytest.raises(ValueError):
                    nb.pfh(8, out=dev)
            finally:
                dev.free()
        finally:
            nb.free()
    finally:
        cloud.free()


def test_pipeline_choice_pfh_and_matching_at_125(engine):
    from shot_fpfh_amd.descriptors import compute_pfh_descriptor
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    p, n = config1_cloud(6000, 5)
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(6)
    pipe = RegistrationPipeline(scan=p @ rot.T, scan_normals=n @ rot.T, ref=p, ref_normals=n)
    pipe.scan_keypoints = np.sort(rng.choice(6000, 300, replace=False))
    pipe.ref_keypoints = np.sort(rng.choice(6000, 300, replace=False))
    pipe.compute_descriptors(0.12, descriptor_choice="pfh")
    sd, rd = pipe.scan_descriptors, pipe.ref_descriptors
    assert sd.shape == rd.shape == (300, 125) and sd.any(axis=1).all() and rd.any(axis=1).all()
    assert np.array_equal(bits(rd), bits(compute_pfh_descriptor(pipe.ref_keypoints, p, n, 0.12)))
    pipe.find_descriptors_matches("simple", reject_threshold=0.8, threshold_multiplier=10)
    best = np.array([np.argmin(((rd - row) ** 2).sum(axis=1)) for row in sd])
    assert np.array_equal(pipe.matches[0], np.arange(300)) and np.array_equal(pipe.matches[1], best)
    pipe.compute_descriptors(0.12, descriptor_choice="pfh", pfh_n_bins=3, force_recompute=True)
    assert pipe.scan_descriptors.shape == (300, 27)
