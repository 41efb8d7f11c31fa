"""Outlier removal on the MI355X (K20) against the NumPy statement of the two filters (tests/outliers_numpy.py: float64,
KDTree.query / KDTree.query_radius, math.fsum).

The statistical check is split where the definition leaves the implementation a choice, the order of a sum:
1. the mean distances against the statement's under (k + 4) 2^-52 relative -- correctly rounded square roots of d2 values formed
   by the same three operations on both sides, a sum of k + 1 non-negative terms in any order, one division;
2. mu and sigma against math.fsum over the DEVICE's own mean array under n 2^-52 relative (any order of a sum of non-negative
   terms), the threshold within 2 ulp of mu + std_ratio sigma formed from the device's own mu and sigma;
3. the kept indices EXACTLY, on the device's own numbers: flatnonzero(mean_dev <= threshold_dev);
4. the kept indices against the statement's: a decision may differ only where the statement has |mean - threshold| <= 1e-9
   threshold, and no point of these inputs is that close (smallest gap of the statement: 2.4e-5 threshold, far_origin; 2.9e-5
   at n = 2001, k = 64), so the sets are equal.
The radius filter is integers: counts and kept sets are compared exactly."""
import ctypes as C
import math

import numpy as np
import pytest

import outliers_numpy as O
from conftest import config1_cloud, family, synth_cloud
from shot_fpfh_amd import _ffi
from shot_fpfh_amd.outlier_removal import remove_radius_outliers, remove_statistical_outliers

pytestmark = pytest.mark.gpu

U = 2.0 ** -52


def _family(name, n):
    return family(name, n, np.random.default_rng(1))[0]


def _twice():
    p = synth_cloud(20000, 7)[0]
    return np.vstack([p[:500], p[:500]])  # every point has an exact duplicate: mean == 0 == threshold


# name -> (points, k, std_ratio)
STATISTICAL = {
    "uniform": (lambda: synth_cloud(20000, 7)[0], 20, 2.0),
    "sphere_k20": (lambda: O.contaminated_sphere(20000, 400, 1), 20, 2.0),
    "sphere_k8": (lambda: O.contaminated_sphere(20000, 400, 1), 8, 1.0),
    "clustered": (lambda: _family("clustered", 5000), 16, 1.0),
    "lattice": (lambda: _family("lattice", 4096), 6, 1.0),
    "duplicates": (lambda: _family("duplicates", 5000), 10, 2.0),
    "far_origin": (lambda: _family("far_origin", 5000), 10, 2.0),
    "slab": (lambda: _family("slab", 5000), 10, 2.0),
    "last_wave_of_1": (lambda: synth_cloud(2001, 7)[0], 30, 2.0),  # a wave serves four points
    "k63": (lambda: synth_cloud(2001, 7)[0], 63, 2.0),  # k + 1 = 64: the last list length of the fast k-NN kernel
    "k64": (lambda: synth_cloud(2001, 7)[0], 64, 2.0),  # the other k-NN kernel; a list longer than a wave
    "k100": (lambda: synth_cloud(2001, 7)[0], 100, 2.0),
    "n70_k64": (lambda: synth_cloud(70, 7)[0], 64, 1.0),
    "three_points": (lambda: synth_cloud(3, 7)[0], 2, 1.0),  # one wave is the whole launch
    "all_duplicates": (_twice, 1, 2.0),
}
# removed points, from the statement (recomputed by the tests: these only say that the cases are what they were chosen to be)
REMOVED = {"uniform": 752, "sphere_k20": 346, "sphere_k8": 371, "clustered": 954, "lattice": 1352, "duplicates": 158,
           "far_origin": 169, "slab": 156, "last_wave_of_1": 95, "n70_k64": 12, "three_points": 1, "all_duplicates": 0}

_cache = {}


@pytest.fixture(scope="module")
def engine():
    from shot_fpfh_amd import default_engine

    return default_engine()


def _case(name, engine):
    """points, parameters, the statement's side and the device's side (one public call with everything returned) of one case"""
    if name not in _cache:
        make, k, ratio = STATISTICAL[name]
        p = make()
        kept_np, mean_np, st_np = O.statistical(p, k, ratio)
        cloud = engine.cloud(p)
        try:
            kept, mean, st = cloud.statistical_outliers(k, ratio, return_stats=True)
        finally:
            cloud.free()
        _cache[name] = (p, k, ratio, kept_np, mean_np, st_np, kept, mean, st)
    return _cache[name]


@pytest.mark.parametrize("name", list(STATISTICAL))
def test_statistical_against_the_statement(name, engine):
    p, k, ratio, kept_np, mean_np, st_np, kept, mean, st = _case(name, engine)
    n = p.shape[0]
    if name in REMOVED:
        assert n - kept_np.size == REMOVED[name]
    # 1. the mean distances
    assert mean.dtype == np.float64 and mean.shape == (n,)
    err = np.abs(mean - mean_np)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio_to_bound = np.where(mean_np > 0, err / ((k + 4) * U * mean_np), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio_to_bound.max())
    # 2. mu, sigma, threshold on the device's own mean array
    mu, sigma, threshold = (float(v) for v in st)
    mu_f, sigma_f, _ = O.stats(mean, ratio)
    mu_err = abs(mu - mu_f) / mu_f if mu_f else abs(mu)
    sigma_err = abs(sigma - sigma_f) / sigma_f if sigma_f else abs(sigma)
    thr_ulps = abs(threshold - (mu + ratio * sigma)) / np.spacing(abs(mu + ratio * sigma)) if threshold else 0.0
    # 4. decisions against the statement's
    in_np, in_dev = np.zeros(n, bool), np.zeros(n, bool)
    in_np[kept_np], in_dev[kept] = True, True
    near = np.abs(mean_np - st_np[2]) <= 1e-9 * st_np[2]
    differ = in_np != in_dev
    gap = float((np.abs(mean_np - st_np[2]) / st_np[2]).min()) if st_np[2] else 0.0
    print(f"OUTLIERS_PARITY {name} n={n} k={k} std_ratio={ratio} removed_numpy={n - kept_np.size} removed_device={n - kept.size} "
          f"mean_err_over_bound={worst:.3f} mu_rel={mu_err:.2e} sigma_rel={sigma_err:.2e} threshold_ulps={thr_ulps:.1f} "
          f"statement_gap={gap:.2e} near={int(near.sum())} decisions_differ={int(differ.sum())}")
    assert np.all(err <= (k + 4) * U * mean_np), np.flatnonzero(err > (k + 4) * U * mean_np)[:10]
    assert mu_err <= n * U and sigma_err <= n * U
    assert thr_ulps <= 2.0
    # 3. the mask on the device's own numbers
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0)
    assert np.array_equal(kept, np.flatnonzero(mean <= threshold))
    assert not np.any(differ & ~near), np.flatnonzero(differ & ~near)[:10]
    if name == "all_duplicates":  # threshold 0: every point sits ON it, and every decision is `0 <= 0`
        assert threshold == 0.0 and np.all(mean == 0.0) and kept.size == n
    else:
        assert near.sum() == 0
    assert np.array_equal(kept, kept_np)


def _block_sum(v):
    """sf_block_sum4_stage + sf_block_sum4_at of 256 per-thread values: the xor ladder 32 .. 1 inside each wave, then the four
    waves in order"""
    w = v.reshape(4, 64).copy()
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lanes ^ off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def _fixed_order_sum(terms):
    """The device's sum of n terms (outliers.hip): B = clamp(ceil(n / 1024), 1, 1024) blocks of 256 threads, thread t of block b
    adds terms (b + j B) 256 + t for j = 0, 1, .. in that order; a block sum each; then one block whose thread t adds the
    partials t, t + 256, .. and a last block sum."""
    n = terms.shape[0]
    nb = min(max(-(-n // 1024), 1), 1024)
    rounds = -(-n // (nb * 256))
    padded = np.zeros(rounds * nb * 256)
    padded[:n] = terms
    acc = np.zeros((nb, 256))
    for chunk in padded.reshape(rounds, nb, 256):
        acc = acc + chunk
    partial = np.array([_block_sum(a) for a in acc])
    fold = np.zeros(256)
    for j in range(0, nb, 256):
        part = partial[j: j + 256]
        fold[: part.size] = fold[: part.size] + part
    return _block_sum(fold)


def _device_stats(mean):
    """(mu, sigma) as the two passes of the device form them from a mean-distance array"""
    n = mean.shape[0]
    mu = _fixed_order_sum(mean) / n
    d = mean - mu
    return mu, math.sqrt(_fixed_order_sum(d * d) / (n - 1))


def _raw_statistical(engine, cloud, k, ratio):
    n = cloud.n
    mean, stats, sel, kept = np.zeros(n), np.zeros(3), np.zeros(n, dtype=np.int64), C.c_int64(0)
    _ffi.check(engine.lib.sf_outliers_statistical(engine.h, cloud.h, k, ratio, mean.ctypes.data, stats.ctypes.data, sel.ctypes.data,
                                                 C.byref(kept), _ffi.SF_HOST), "sf_outliers_statistical")
    return sel[: kept.value].copy(), mean, stats


@pytest.mark.parametrize("name", ["sphere_k20", "lattice", "duplicates", "k64", "three_points"])
def test_one_call_equals_its_steps_and_repeats_bit_for_bit(name, engine):
    p, k, ratio, _, _, _, kept, mean, st = _case(name, engine)
    n = p.shape[0]
    cloud = engine.cloud(p)
    try:
        # the steps: the mean distances alone; the statistics, a pure function of that array (the fixed order of the two sums,
        # re-enacted in NumPy: bit for bit); the select on the stored threshold
        assert np.array_equal(cloud.knn_mean_distance(k), mean)
        assert _device_stats(mean) == (st[0], st[1])
        assert np.array_equal(np.flatnonzero(mean <= st[2]), kept)
        # the same entry point with its outputs left on the device
        dmean = engine.empty((n,)).from_host(mean)
        dsel = engine.empty((n,), np.int64)
        try:
            stats, num = np.zeros(3), C.c_int64(0)
            _ffi.check(engine.lib.sf_outliers_statistical(engine.h, cloud.h, k, ratio, dmean.ptr, stats.ctypes.data, dsel.ptr,
                                                         C.byref(num), _ffi.SF_OUT_DEVICE), "sf_outliers_statistical")
            assert np.array_equal(stats, st) and num.value == kept.size
            assert np.array_equal(dsel.to_host()[: num.value], kept) and np.array_equal(dmean.to_host(), mean)
        finally:
            dmean.free()
            dsel.free()
        # a second call, and the entry point without the optional outputs
        k2, m2, s2 = _raw_statistical(engine, cloud, k, ratio)
        assert np.array_equal(k2, kept) and np.array_equal(m2, mean) and np.array_equal(s2, st)
        assert np.array_equal(cloud.statistical_outliers(k, ratio), kept)
    finally:
        cloud.free()
    assert np.array_equal(remove_statistical_outliers(p, k, ratio), kept)  # the public function, a fresh Cloud
    r = remove_statistical_outliers(p, k, ratio, return_stats=True)
    assert np.array_equal(r[0], kept) and np.array_equal(r[1], mean) and np.array_equal(r[2], st)
    for other in (0.03, 0.11):  # the same Cloud, searched at other radii first: grids the pass must not inherit anything from
        cloud = engine.cloud(p)
        try:
            cloud.radius_search(p[:64], other)
            k3, m3, s3 = cloud.statistical_outliers(k, ratio, return_stats=True)
            assert np.array_equal(m3, mean) and np.array_equal(s3, st) and np.array_equal(k3, kept)
            cloud.radius_search(p[:64], 1.7 * other)
            assert np.array_equal(cloud.knn_mean_distance(k), mean)
        finally:
            cloud.free()


# name -> (points, radius, min_neighbors, kept by the statement or None)
RADIUS = {
    "uniform": (lambda: synth_cloud(20000, 7)[0], 0.06, 6, 19867),
    "sphere": (lambda: O.contaminated_sphere(20000, 400, 1), 0.03, 6, 19997),
    "lattice": (lambda: _family("lattice", 4096), 0.125, 6, 4096),  # points exactly on the radius
    "three_points": (lambda: synth_cloud(3, 7)[0], 2.0, 2, None),
}


@pytest.mark.parametrize("name", list(RADIUS))
def test_radius_against_the_statement(name, engine):
    make, radius, min_neighbors, expect = RADIUS[name]
    p = make()
    n = p.shape[0]
    kept_np, counts_np = O.radius(p, radius, min_neighbors)
    if expect is not None:
        assert kept_np.size == expect
    cloud = engine.cloud(p)
    try:
        counts = cloud.ball_counts(radius)
        assert counts.dtype == np.int32 and np.array_equal(counts, counts_np)
        kept, c2 = cloud.radius_outliers(radius, min_neighbors, return_counts=True)
        print(f"OUTLIERS_RADIUS {name} n={n} radius={radius} min_neighbors={min_neighbors} kept={kept.size} "
              f"counts={counts.min()}..{counts.max()}")
        assert kept.dtype == np.int64 and np.array_equal(kept, kept_np) and np.array_equal(c2, counts)
        assert np.array_equal(cloud.radius_outliers(radius, min_neighbors), kept)  # again, without the counts
        assert np.array_equal(cloud.radius_outliers(radius, 0), np.arange(n))  # every point has itself
        top = int(counts_np.max())
        assert np.array_equal(cloud.radius_outliers(radius, top - 1), np.flatnonzero(counts_np == top))
        assert cloud.radius_outliers(radius, top).size == 0
    finally:
        cloud.free()
    assert np.array_equal(remove_radius_outliers(p, radius, min_neighbors), kept)
    for other in (1.7 * radius, 0.6 * radius):  # a Cloud that carries another grid (one that would serve `radius`, one too fine)
        cloud = engine.cloud(p)
        try:
            cloud.radius_search(p[:64], other)
            k3, c3 = cloud.radius_outliers(radius, min_neighbors, return_counts=True)
            assert np.array_equal(k3, kept) and np.array_equal(c3, counts)
            cloud.radius_search(p[:64], other)
            assert np.array_equal(cloud.ball_counts(radius), counts)
        finally:
            cloud.free()


def test_bad_arguments_are_sf_err_arg_with_a_message(engine):
    p = synth_cloud(100, 7)[0]
    cloud = engine.cloud(p)
    one = engine.cloud(p[:1])
    try:
        lib, h = engine.lib, engine.h
        mean, stats, sel, cnt, num = np.zeros(100), np.zeros(3), np.zeros(100, dtype=np.int64), np.zeros(100, dtype=np.int32), C.c_int64(0)
        ptr = lambda a: a.ctypes.data  # noqa: E731
        calls = [
            lambda: lib.sf_knn_mean_distance(h, cloud.h, 0, ptr(mean), 0),
            lambda: lib.sf_knn_mean_distance(h, cloud.h, 100, ptr(mean), 0),
            lambda: lib.sf_knn_mean_distance(h, one.h, 1, ptr(mean), 0),
            lambda: lib.sf_knn_mean_distance(h, cloud.h, 5, None, 0),
            lambda: lib.sf_outliers_statistical(h, cloud.h, 100, 2.0, None, ptr(stats), ptr(sel), C.byref(num), 0),
            lambda: lib.sf_outliers_statistical(h, cloud.h, 5, float("nan"), None, ptr(stats), ptr(sel), C.byref(num), 0),
            lambda: lib.sf_outliers_statistical(h, cloud.h, 5, float("inf"), None, ptr(stats), ptr(sel), C.byref(num), 0),
            lambda: lib.sf_outliers_statistical(h, cloud.h, 5, 2.0, None, ptr(stats), None, C.byref(num), 0),
            lambda: lib.sf_ball_counts(h, cloud.h, 0.0, ptr(cnt), 0),
            lambda: lib.sf_ball_counts(h, cloud.h, float("nan"), ptr(cnt), 0),
            lambda: lib.sf_outliers_radius(h, cloud.h, -1.0, 2, None, ptr(sel), C.byref(num), 0),
            lambda: lib.sf_outliers_radius(h, cloud.h, 0.1, -1, None, ptr(sel), C.byref(num), 0),
        ]
        for i, call in enumerate(calls):
            assert call() == -1, i  # SF_ERR_ARG
            assert _ffi.last_error(), i
        with pytest.raises(ValueError):
            cloud.knn_mean_distance(100)
        with pytest.raises(ValueError):
            cloud.statistical_outliers(5, float("nan"))
    finally:
        cloud.free()
        one.free()


def test_pipeline_removes_outliers_in_front_of_iss_and_fpfh(engine):
    from shot_fpfh_amd import RegistrationPipeline

    scan, ref = O.contaminated_sphere(20000, 400, 1), O.contaminated_sphere(12000, 240, 2)
    sn = np.vstack([config1_cloud(20000, 1)[1], np.tile([0.0, 0.0, 1.0], (400, 1))])
    rn = np.vstack([config1_cloud(12000, 2)[1], np.tile([0.0, 0.0, 1.0], (240, 1))])
    pipe = RegistrationPipeline(scan=scan, scan_normals=sn, ref=ref, ref_normals=rn)
    pipe.remove_outliers("statistical")
    kept = remove_statistical_outliers(scan)
    assert np.array_equal(pipe.scan_kept, kept) and np.array_equal(pipe.ref_kept, remove_statistical_outliers(ref))
    assert kept.size == 20400 - 346 and np.all(kept[:20000] == np.arange(20000))  # the surface stays whole
    assert np.array_equal(pipe.scan, scan[kept]) and np.array_equal(pipe.scan_normals, sn[kept])
    assert np.array_equal(pipe.ref, ref[pipe.ref_kept]) and np.array_equal(pipe.ref_normals, rn[pipe.ref_kept])
    pipe.select_keypoints("iss", neighborhood_size=0.04, iss_non_max_radius=0.03)
    assert 0 < pipe.scan_keypoints.size < pipe.scan.shape[0] // 4
    pipe.compute_descriptors(radius=0.08, descriptor_choice="fpfh", disable_progress_bars=True, verbose=False)
    assert pipe.scan_descriptors.shape == (pipe.scan_keypoints.size, 125) and np.isfinite(pipe.scan_descriptors).all()
    assert pipe.ref_descriptors.shape == (pipe.ref_keypoints.size, 125) and np.isfinite(pipe.ref_descriptors).all()
    with pytest.raises(ValueError):
        pipe.remove_outliers("radius", radius=0.03, min_neighbors=6)
    pipe.remove_outliers("radius", radius=0.03, min_neighbors=6, force_recompute=True)
    assert pipe.scan_keypoints is None and pipe.scan_descriptors is None
    assert np.array_equal(pipe.scan_kept, remove_radius_outliers(scan[kept], 0.03, 6))


def test_cli_filters_both_clouds_before_the_normals(engine, tmp_path):
    """scripts/register_point_clouds.py --outliers statistical on the pair of test_hip_parity's script test with strays added to
    both files (the scan without stored normals, the reference with): the written scan is the KEPT points, moved by the motion
    that generated the scan."""
    import importlib.util
    import os

    from conftest import ROOT, load_golden
    from shot_fpfh_amd.helpers import read_ply, write_ply

    g = load_golden("icp_3500.npz")
    rng = np.random.default_rng(5)
    lo, hi = g["ref"].min(axis=0) - 0.3, g["ref"].max(axis=0) + 0.3
    strays = lambda m: (lo + (hi - lo) * rng.random((m, 3))).astype(np.float32).astype(np.float64)  # noqa: E731
    scan = np.vstack([g["scan"], strays(60)])
    ref, ref_normals = np.vstack([g["ref"], strays(60)]), np.vstack([g["ref_normals"], np.tile([0.0, 0.0, 1.0], (60, 1))])
    scan_file, ref_file = str(tmp_path / "scan.ply"), str(tmp_path / "ref.ply")
    write_ply(scan_file, [scan], ["x", "y", "z"])
    write_ply(ref_file, [ref, ref_normals], ["x", "y", "z", "nx", "ny", "nz"])
    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "aligned")
    rc = mod.main([scan_file, ref_file, "--outliers", "statistical", "--outlier-neighbors", "10", "--outlier-std-ratio", "2.0",
                   "--radius", "0.2", "--keypoints", "subsampling", "--keypoint-size", "0.05", "--min-neighborhood-size", "10",
                   "--ransac-draws", "2000", "--ransac-threshold", "0.02", "--icp", "point_to_plane", "--icp-dmax", "0.05",
                   "--icp-voxel", "0.04", "--icp-rms", "1e-9", "--metric-threshold", "0.01", "--write", out])
    assert rc == 0
    scan_on_disk = np.vstack([read_ply(scan_file)[c] for c in "xyz"]).T.astype(np.float64)
    ref_on_disk = np.vstack([read_ply(ref_file)[c] for c in "xyz"]).T.astype(np.float64)
    kept, ref_kept = remove_statistical_outliers(scan_on_disk, 10, 2.0), remove_statistical_outliers(ref_on_disk, 10, 2.0)
    n_scan = g["scan"].shape[0]
    assert kept.size < scan.shape[0] and (kept >= n_scan).sum() < 30  # most strays went
    merged = read_ply(out + "_icp.ply")
    assert merged.shape[0] == kept.size + ref_kept.size and merged["is_scan"][: kept.size].all() and not merged["is_scan"][kept.size:].any()
    moved = np.vstack((merged["x"], merged["y"], merged["z"])).T[: kept.size]
    surface = kept < n_scan
    truth = g["scan"][kept[surface]] @ g["true_rotation"].T + g["true_translation"]
    assert np.abs(moved[surface] - truth).max() < 2e-3  # the script found the generating motion
