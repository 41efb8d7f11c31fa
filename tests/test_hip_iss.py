"""ISS keypoints on the MI355X (K10) against the NumPy statement of the definition (tests/iss_numpy.py: float64,
KDTree.query_radius balls, numpy.linalg.eigvalsh).

The check is split where the definition leaves a choice to the implementation.  Points with the same neighbour set have
saliencies that are equal up to the rounding of a sum, and which of them wins the suppression follows that rounding -- so the
saliency is compared with NumPy's under a bound (1e-9 e1: Weyl's bound for a covariance error of k 2^-53 |C| is ~1e-13 e1),
and the suppression is compared EXACTLY, on the device's own saliency array, where it is nothing but comparisons of identical
float64 values and exact ball membership."""
import numpy as np
import pytest

import iss_numpy as N
from conftest import config1_cloud, family, synth_cloud
from shot_fpfh_amd.keypoint_selection import cloud_resolution, iss_saliency, select_keypoints_iss

pytestmark = pytest.mark.gpu


def _family(name):
    return family(name, 5000, np.random.default_rng(1))[0]


# name -> (points, r_s, r_n); the counts the NumPy statement gives are recomputed by the tests, not stored
CLOUDS = {
    "uniform": (lambda: synth_cloud(20000, 7)[0], 0.06, 0.04),
    "sphere": (lambda: config1_cloud(35947, 1)[0], 0.03, 0.02),
    "bumpy": (lambda: N.bumpy_sphere(30000, 5), 0.03, 0.02),  # (this builder's generator: 29 844 salient, 1 165 keypoints in NumPy)
    "lattice": (lambda: family("lattice", 4096, np.random.default_rng(1))[0], 0.13, 0.09),
    "duplicates": (lambda: _family("duplicates"), 0.1, 0.07),
    "plane": (lambda: _family("plane"), 0.05, 0.03),
    "rough_plane": (lambda: _family("rough_plane"), 0.05, 0.03),
    "slab": (lambda: _family("slab"), 0.05, 0.03),
    "far_origin": (lambda: _family("far_origin"), 0.1, 0.07),
    "clustered": (lambda: _family("clustered"), 0.05, 0.03),
    "uniform_rn_3rs": (lambda: synth_cloud(20000, 7)[0], 0.03, 0.09),  # r_n > r_s: the suppression needs another grid
    "uniform_rs_3rn": (lambda: synth_cloud(20000, 7)[0], 0.09, 0.03),  # r_s / r_n = 3: the saliency grid is too coarse to keep
    # a wave serves four points: last waves of one, two and three points (35 947 above: three), balls of up to several hundred
    "last_wave_of_1": (lambda: synth_cloud(2001, 7)[0], 0.4, 0.15),
    "last_wave_of_2": (lambda: synth_cloud(2002, 7)[0], 0.15, 0.4),
    "three_points": (lambda: synth_cloud(3, 7)[0], 2.0, 2.0),  # ... and a wave that is the whole launch
}

_cache = {}


def _case(name, engine):
    """points, radii, the NumPy side (counts, eigenvalues) and the device side (saliency, counts) of one cloud"""
    if name not in _cache:
        make, r_s, r_n = CLOUDS[name]
        p = make()
        counts, e = N.ball_eigenvalues(p, r_s)
        cloud = engine.cloud(p)
        try:
            sal, cnt = cloud.iss_saliency(r_s, return_counts=True)
        finally:
            cloud.free()
        _cache[name] = (p, r_s, r_n, counts, e, sal, cnt)
    return _cache[name]


@pytest.fixture(scope="module")
def engine():
    from shot_fpfh_amd import default_engine

    return default_engine()


@pytest.mark.parametrize("name", list(CLOUDS))
def test_saliency_against_numpy(name, engine):
    p, r_s, _, counts, e, sal, cnt = _case(name, engine)
    assert sal.dtype == np.float64 and sal.shape == (p.shape[0],)
    assert np.array_equal(cnt, counts), "ball sizes differ"  # the project's neighbour-set rule: 100 %
    ref = N.saliency_from(counts, e)
    both = (sal > 0) & (ref > 0)
    gap = np.abs(sal[both] - e[both, 2]) / e[both, 0]
    worst = float(gap.max(initial=0.0))
    differ = (sal > 0) != (ref > 0)
    excepted = differ & N.near_a_threshold(e)
    print(f"ISS_PARITY {name} n={p.shape[0]} r_s={r_s} salient_numpy={int((ref > 0).sum())} salient_device={int((sal > 0).sum())} "
          f"max_gap_over_e1={worst:.3e} decisions_differ={int(differ.sum())} near_threshold={int(N.near_a_threshold(e).sum())}")
    assert np.all((sal > 0) | (sal == -1.0))
    assert worst <= 1e-9
    assert not np.any(differ & ~excepted), np.flatnonzero(differ & ~excepted)[:10]
    assert excepted.sum() <= 1e-3 * p.shape[0]


@pytest.mark.parametrize("name", list(CLOUDS))
def test_suppression_is_exact_on_the_devices_own_saliency(name, engine):
    p, _, r_n, _, _, sal, _ = _case(name, engine)
    cloud = engine.cloud(p)
    try:
        got = cloud.iss_select(sal, r_n)
        want = N.select(p, sal, r_n)
        print(f"ISS_SELECT {name} r_n={r_n} keypoints={want.size}")
        assert got.dtype == np.int64 and np.array_equal(got, want)
        # any score will do: many exact ties and negatives
        score = (np.arange(p.shape[0]) % 7 - 2).astype(np.float64)
        assert np.array_equal(cloud.iss_select(score, r_n), N.select(p, score, r_n))
        assert np.array_equal(cloud.iss_select(score, r_n, min_neighbors=1), N.select(p, score, r_n, min_neighbors=1))
        score = 1.0 + np.arange(p.shape[0]) % 5  # every point sweeps: no wave is skipped, ties everywhere
        assert np.array_equal(cloud.iss_select(score, r_n, min_neighbors=1), N.select(p, score, r_n, min_neighbors=1))
    finally:
        cloud.free()


@pytest.mark.parametrize("name", ["uniform", "sphere", "lattice", "duplicates", "uniform_rn_3rs", "uniform_rs_3rn"])
def test_end_to_end(name, engine):
    p, r_s, r_n, _, _, sal, _ = _case(name, engine)
    kp, s2 = select_keypoints_iss(p, r_s, r_n, return_saliency=True)
    assert kp.dtype == np.int64 and np.all(np.diff(kp) > 0)
    assert np.array_equal(s2, sal) and np.array_equal(iss_saliency(p, r_s), sal)  # bit for bit
    cloud = engine.cloud(p)
    try:
        assert np.array_equal(kp, cloud.iss_select(cloud.iss_saliency(r_s), r_n))
    finally:
        cloud.free()
    assert np.array_equal(kp, select_keypoints_iss(p, r_s, r_n))  # deterministic
    for other in (1.7 * r_s, 0.8 * r_n):  # the same Cloud, searched at another radius first: a grid the passes must not trust
        cloud = engine.cloud(p)
        try:
            cloud.radius_search(p[:64], other)
            k3, s3 = cloud.iss_keypoints(r_s, r_n, return_saliency=True)
            assert np.array_equal(s3, sal) and np.array_equal(k3, kp)
            cloud.radius_search(p[:64], other)
            assert np.array_equal(cloud.iss_select(sal, r_n), kp)
        finally:
            cloud.free()


def test_automatic_radii_and_resolution(engine):
    p = synth_cloud(20000, 7)[0]
    rho, ref = cloud_resolution(p), N.resolution(p)
    assert abs(rho - ref) <= 1e-12 * ref
    kp = select_keypoints_iss(p)
    assert np.array_equal(kp, select_keypoints_iss(p, 6.0 * rho, 4.0 * rho)) and kp.size
    assert np.array_equal(select_keypoints_iss(p, non_max_radius=4.0 * rho), kp)
    d = family("duplicates", 5000, np.random.default_rng(1))[0]
    assert abs(cloud_resolution(d) - N.resolution(d)) <= 1e-12 * N.resolution(d)
    twice = np.vstack([p[:500], p[:500]])  # every point has an exact duplicate: resolution 0
    assert cloud_resolution(twice) == 0.0
    with pytest.raises(ValueError):
        select_keypoints_iss(twice)
    assert select_keypoints_iss(twice, 0.2, 0.1).dtype == np.int64  # (explicit radii need no resolution)


def test_plane_has_no_keypoints(engine):
    p = _family("plane")
    kp, sal = select_keypoints_iss(p, 0.05, 0.03, return_saliency=True)
    assert kp.dtype == np.int64 and kp.size == 0 and np.all(sal == -1.0)


def test_pipeline_feeds_fpfh_and_shot(engine):
    from shot_fpfh_amd import RegistrationPipeline

    p, d = config1_cloud(35947, 1)
    q, dq = config1_cloud(20000, 2)
    pipe = RegistrationPipeline(scan=p, scan_normals=d, ref=q, ref_normals=dq)
    pipe.select_keypoints("iss", neighborhood_size=0.03, iss_non_max_radius=0.02)
    assert np.array_equal(pipe.scan_keypoints, select_keypoints_iss(p, 0.03, 0.02))
    assert pipe.scan_keypoints.dtype == np.int64 and 0 < pipe.scan_keypoints.size < p.shape[0] // 4
    pipe.compute_descriptors(radius=0.06, descriptor_choice="fpfh", disable_progress_bars=True, verbose=False)
    assert pipe.scan_descriptors.shape == (pipe.scan_keypoints.size, 125) and np.isfinite(pipe.scan_descriptors).all()
    pipe.compute_descriptors(radius=0.06, descriptor_choice="shot_single_scale", subsample_support=False, min_neighborhood_size=10,
                             disable_progress_bars=True, verbose=False, force_recompute=True)
    assert pipe.ref_descriptors.shape == (pipe.ref_keypoints.size, 352) and np.isfinite(pipe.ref_descriptors).all()
    pipe.select_keypoints("iss", min_n_neighbors=8, force_recompute=True)  # automatic radii
    assert np.array_equal(pipe.ref_keypoints, select_keypoints_iss(q, min_neighbors=8))
