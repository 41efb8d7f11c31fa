"""The serial compute_shot_descriptor (shot.py:310-499) with any number of cosine bins n (1 .. 64): the kernel of
shot_bins.hip (sf_shot_serial_bins) against the reference's rows in tests/golden/shot_cosine_bins.npz
(tools/gen_golden_shot_bins.py), and at n = 11 against the tuned K5 (sf_shot_serial) on large clouds.

  (a) every golden row within the parity tolerance, and within 1e-12 absolute (a flipped bin decision is far above it);
  (b) the z = 0 planes: normals +z raise IndexError for even n (the cosine bin rounds to n), as the reference does; 0 and -1
      raise what the reference raised; the +x planes (cosine 0: ties for every even n) match the goldens;
  (c) n = 11 on a 200 000-point cloud and on a clustered one with lists above 255 and above 3 072 points: the same zero
      pattern as sf_shot_serial and at most 1e-15 apart (only the reduction order of the norm differs);
  (d) two calls give the same bits;  (e) SF_OUT_DEVICE gives the rows of the host output.
"""
import numpy as np
import pytest

from conftest import load_golden, synth_cloud

pytestmark = pytest.mark.gpu

TOL = 1e-5


def close(a, b, tol=TOL):
    return np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))


@pytest.fixture(scope="module")
def g():
    return load_golden("shot_cosine_bins.npz")


def _case(g, case):
    f = lambda k: g[f"{case}_{k}"]  # noqa: E731
    return (f("points").astype(np.float64), f("normals").astype(np.float64), f("kp").astype(np.float64),
            float(f("radius")), int(f("min_nb")), [int(n) for n in f("ns")])


CASES = ["random", "dups", "cluster", "plane_x", "plane_z"]


@pytest.mark.parametrize("case", CASES)
def test_rows_match_the_reference(g, case):
    """(a), and the +x / odd-n planes of (b): (M, 32 n) float64 rows equal to the reference's."""
    from shot_fpfh_amd.descriptors.shot import compute_shot_descriptor

    p, nr, kp, r, mn, ns = _case(g, case)
    checked = 0
    stored = [n for n in ns if f"{case}_rows_{n}" in g.files]
    for n in ns:
        if f"{case}_rows_{n}" not in g.files:
            continue
        want, sel = g[f"{case}_rows_{n}"], g[f"{case}_sel_{n}"]
        got = compute_shot_descriptor(kp[sel], p, nr, r, min_neighborhood_size=mn, n_cosine_bins=n)
        assert got.shape == want.shape and got.dtype == np.float64, (n, got.shape, want.shape)
        assert np.all(close(got, want)), (case, n, np.abs(got - want).max())
        assert np.abs(got - want).max() <= 1e-12, (case, n, np.abs(got - want).max())
        assert np.array_equal(got.any(axis=1), want.any(axis=1)), (case, n)
        checked += 1
    assert checked == len(stored) >= 2


@pytest.mark.parametrize("case", ["plane_x", "plane_z"])
def test_planes_raise_what_the_reference_raises(g, case):
    """(b): normals +z put every neighbour at cosine +1 -- bin n for even n, IndexError for the whole call; n = 0 IndexError
    (keypoints pass the gate), n = -1 ValueError."""
    from shot_fpfh_amd.descriptors.shot import compute_shot_descriptor

    p, nr, kp, r, mn, ns = _case(g, case)
    raised = [n for n in ns if f"{case}_raises_{n}" in g.files]
    assert 0 in raised and -1 in raised
    if case == "plane_z":
        assert {2, 4, 8, 16} <= set(raised)
    for n in raised:
        exc = {"IndexError": IndexError, "ValueError": ValueError}[str(g[f"{case}_raises_{n}"])]
        with pytest.raises(exc):
            compute_shot_descriptor(kp, p, nr, r, min_neighborhood_size=mn, n_cosine_bins=n)


def test_zero_bins_without_a_passing_keypoint_gives_empty_rows(g):
    """n = 0 when no keypoint passes the gate: the reference returns (M, 0) rows."""
    from shot_fpfh_amd.descriptors.shot import compute_shot_descriptor

    p, nr, kp, r, _, _ = _case(g, "random")
    d = compute_shot_descriptor(kp, p, nr, r, min_neighborhood_size=100000, n_cosine_bins=0)
    assert d.shape == (len(kp), 0)


def _serial_pair(p, nr, kp, r, mn):
    """sf_shot_serial (the tuned K5) and sf_shot_serial_bins at n = 11 on the same lists."""
    import shot_fpfh_amd as s
    from shot_fpfh_amd.engine import Cloud

    cloud = Cloud(s.default_engine(), p, nr)
    try:
        nb = cloud.radius_search(kp, r)
        try:
            return nb.shot_serial(mn), nb.shot_serial(mn, n_cosine_bins=11)
        finally:
            nb.free()
    finally:
        cloud.free()


def _same_rows(tuned, new):
    assert new.shape == tuned.shape == (tuned.shape[0], 352)
    assert np.array_equal(new == 0.0, tuned == 0.0)
    assert np.abs(new - tuned).max() <= 1e-15, np.abs(new - tuned).max()


def test_eleven_bins_match_the_tuned_kernel_on_a_large_cloud():
    """(c) on 200 000 points (the register-cached K5 form, lists up to ~160 points)."""
    p, nr, rng = synth_cloud(200_000, 811)
    kp = np.vstack([p[rng.choice(len(p), 40_000, replace=False)], rng.random((2000, 3))])
    tuned, new = _serial_pair(p, nr, kp, 0.05, 10)
    assert tuned.any(axis=1).sum() > 35_000
    _same_rows(tuned, new)


def test_eleven_bins_match_the_tuned_kernel_on_long_lists():
    """(c) on a clustered cloud: lists of 256 .. 3 072 points (the team form) and above (the streaming form)."""
    p, nr, rng = synth_cloud(20_000, 812)
    c = 0.5 + 0.07 * rng.standard_normal((12_000, 3))
    cn = rng.standard_normal((12_000, 3))
    cn /= np.linalg.norm(cn, axis=1)[:, None]
    p, nr = np.vstack([p, c]), np.vstack([nr, cn])
    kp = np.vstack([c[:600], p[:2000], p[-50:]])  # (cluster, background, duplicates of cluster points)
    p, nr = np.vstack([p, p[-50:]]), np.vstack([nr, nr[-50:]])
    from sklearn.neighbors import KDTree

    counts = KDTree(p).query_radius(kp, 0.12, count_only=True)
    assert (counts > 3072).sum() > 100 and ((counts > 255) & (counts <= 3072)).sum() > 100
    tuned, new = _serial_pair(p, nr, kp, 0.12, 10)
    _same_rows(tuned, new)


def test_two_calls_give_the_same_bits_and_device_output_equals_host_output(g):
    """(d) and (e), at a few bin counts, on the clustered golden case (long lists: the most atomics per slot)."""
    import shot_fpfh_amd as s
    from shot_fpfh_amd.engine import Cloud

    p, nr, kp, r, mn, _ = _case(g, "cluster")
    eng = s.default_engine()
    cloud = Cloud(eng, p, nr)
    try:
        nb = cloud.radius_search(kp, r)
        try:
            for n in (5, 11, 16, 64):
                a = nb.shot_serial(mn, n_cosine_bins=n)
                b = nb.shot_serial(mn, n_cosine_bins=n)
                assert a.shape == (len(kp), 32 * n)
                assert a.tobytes() == b.tobytes(), n
                out = eng.empty((len(kp), 32 * n))
                try:
                    nb.shot_serial(mn, n_cosine_bins=n, out=out)
                    assert out.to_host().tobytes() == a.tobytes(), n
                finally:
                    out.free()
        finally:
            nb.free()
    finally:
        cloud.free()
