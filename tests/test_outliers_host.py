"""Outlier removal (K20), the part that needs no GPU: the NumPy statement of the two filters (tests/outliers_numpy.py) on
clouds whose answers were recorded once with sklearn's KDTree, the argument errors, the public surface, the pipeline's
bookkeeping and the compiler's resource listing of the new kernels."""
import glob
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import outliers_numpy as O
from conftest import ROOT, family, synth_cloud
from shot_fpfh_amd import outlier_removal
from shot_fpfh_amd.outlier_removal import remove_radius_outliers, remove_statistical_outliers


def _pts(n=50, seed=0):
    return np.random.default_rng(seed).random((n, 3))


# ---- the statement on recorded cases ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, std_ratio, strays_removed", [(20, 2.0, 346), (8, 1.0, 371)])
def test_statement_on_the_contaminated_sphere(k, std_ratio, strays_removed):
    p = O.contaminated_sphere(20000, 400, 1)
    assert p.shape == (20400, 3)
    kept, mean, (mu, sigma, threshold) = O.statistical(p, k, std_ratio)
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0)
    removed = np.setdiff1d(np.arange(p.shape[0]), kept)
    assert int((removed >= 20000).sum()) == strays_removed
    assert int((removed < 20000).sum()) == 0  # no point of the surface goes
    assert threshold == mu + std_ratio * sigma and np.array_equal(kept, np.flatnonzero(mean <= threshold))


def test_statement_keeps_a_cloud_of_exact_duplicates():
    p = synth_cloud(20000, 7)[0]
    twice = np.vstack([p[:500], p[:500]])
    kept, mean, st = O.statistical(twice, 1, 2.0)
    assert np.all(mean == 0.0) and st == (0.0, 0.0, 0.0)  # mean == 0 == threshold: `<=` keeps everything
    assert np.array_equal(kept, np.arange(1000))


def test_statement_radius_rule_with_points_exactly_on_the_radius():
    p = family("lattice", 4096, np.random.default_rng(1))[0]  # spacing 1/16: two cells away is exactly 0.125
    kept, counts = O.radius(p, 0.125, 6)
    assert counts.min() == 11 and counts.max() == 33  # corner: 1 + 3 + 3 + 1 + 3; inside: 1 + 6 + 12 + 8 + 6
    assert np.array_equal(kept, np.arange(4096))
    assert O.radius(p, 0.125, 11)[0].size < 4096  # the corners have ten other points
    assert np.array_equal(O.radius(p, 0.125, 0)[0], np.arange(4096))


# ---- argument errors (all raised before a device is asked for) ----------------------------------------------------------------
@pytest.mark.parametrize("k", [0, -1, 50, 51, 2.5])
def test_nb_neighbors_must_lie_in_1_to_n_minus_1(k):
    with pytest.raises(ValueError):
        remove_statistical_outliers(_pts(50), k)


@pytest.mark.parametrize("n", [0, 1])
def test_the_statistical_filter_needs_two_points(n):
    with pytest.raises(ValueError):
        remove_statistical_outliers(np.zeros((n, 3)), 1)


@pytest.mark.parametrize("ratio", [float("nan"), float("inf"), float("-inf")])
def test_std_ratio_must_be_finite(ratio):
    with pytest.raises(ValueError):
        remove_statistical_outliers(_pts(), 5, ratio)


@pytest.mark.parametrize("radius", [0.0, -0.1, float("nan"), float("inf")])
def test_radius_must_be_positive_and_finite(radius):
    with pytest.raises(ValueError):
        remove_radius_outliers(_pts(), radius)


@pytest.mark.parametrize("m", [-1, -5, 1.5])
def test_min_neighbors_must_not_be_negative(m):
    with pytest.raises(ValueError):
        remove_radius_outliers(_pts(), 0.1, m)


def test_points_must_be_n_by_3():
    with pytest.raises(ValueError):
        remove_statistical_outliers(np.zeros((10, 2)), 3)
    with pytest.raises(ValueError):
        remove_radius_outliers(np.zeros(9), 0.1)


def test_the_radius_filter_of_an_empty_cloud_is_empty():
    idx = remove_radius_outliers(np.zeros((0, 3)), 0.1)
    assert idx.dtype == np.int64 and idx.shape == (0,)
    idx, cnt = remove_radius_outliers(np.zeros((0, 3)), 0.1, return_counts=True)
    assert idx.shape == (0,) and cnt.dtype == np.int32 and cnt.shape == (0,)


# ---- the public surface -----------------------------------------------------------------------------------------------------
def test_signatures_exports_and_prototypes():
    import shot_fpfh_amd
    from shot_fpfh_amd import Cloud, _ffi

    for name in ("remove_statistical_outliers", "remove_radius_outliers"):
        assert name in outlier_removal.__all__ and name in shot_fpfh_amd.__all__
        assert getattr(shot_fpfh_amd, name) is getattr(outlier_removal, name)
    p = inspect.signature(remove_statistical_outliers).parameters
    assert list(p) == ["points", "nb_neighbors", "std_ratio", "return_stats", "engine"]
    assert [p[k].default for k in list(p)[1:]] == [20, 2.0, False, None]
    assert p["return_stats"].kind is inspect.Parameter.KEYWORD_ONLY and p["engine"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(remove_radius_outliers).parameters
    assert list(p) == ["points", "radius", "min_neighbors", "return_counts", "engine"]
    assert p["radius"].default is inspect.Parameter.empty and [p[k].default for k in list(p)[2:]] == [2, False, None]
    assert p["return_counts"].kind is inspect.Parameter.KEYWORD_ONLY and p["engine"].kind is inspect.Parameter.KEYWORD_ONLY
    for method in ("knn_mean_distance", "statistical_outliers", "ball_counts", "radius_outliers"):
        assert callable(getattr(Cloud, method))
    text = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name in ("sf_knn_mean_distance", "sf_outliers_statistical", "sf_ball_counts", "sf_outliers_radius"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _ffi.SIGNATURES
        assert hasattr(_ffi.load(), name)


def test_cli_takes_the_outlier_options():
    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["a.ply", "b.ply", "--radius", "0.1"])
    assert (a.outliers, a.outlier_neighbors, a.outlier_std_ratio, a.outlier_radius, a.outlier_min_neighbors) == ("none", 20, 2.0, None, 2)
    a = mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--outliers", "statistical", "--outlier-neighbors", "8",
                        "--outlier-std-ratio", "1.0"])
    assert (a.outliers, a.outlier_neighbors, a.outlier_std_ratio) == ("statistical", 8, 1.0)
    a = mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--outliers", "radius", "--outlier-radius", "0.03",
                        "--outlier-min-neighbors", "6"])
    assert (a.outliers, a.outlier_radius, a.outlier_min_neighbors) == ("radius", 0.03, 6)
    with pytest.raises(SystemExit):
        mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--outliers", "radius"])  # no --outlier-radius


# ---- the pipeline's bookkeeping (the filters replaced by the statement: no device) -----------------------------------------
def test_pipeline_remove_outliers_filters_clouds_and_guards_what_indexes_them(monkeypatch):
    import dataclasses

    from shot_fpfh_amd import RegistrationPipeline, pipeline

    names = [f.name for f in dataclasses.fields(RegistrationPipeline)]
    assert names[-2:] == ["scan_kept", "ref_kept"] and names[:4] == ["scan", "scan_normals", "ref", "ref_normals"]
    p = inspect.signature(RegistrationPipeline.remove_outliers).parameters
    assert list(p) == ["self", "method", "nb_neighbors", "std_ratio", "radius", "min_neighbors", "force_recompute"]
    assert [p[k].default for k in list(p)[2:]] == [20, 2.0, None, 2, False]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[2:])

    calls = []

    def stat(points, nb_neighbors=20, std_ratio=2.0):
        calls.append(("statistical", nb_neighbors, std_ratio))
        return O.statistical(points, nb_neighbors, std_ratio)[0]

    def rad(points, radius, min_neighbors=2):
        calls.append(("radius", radius, min_neighbors))
        return O.radius(points, radius, min_neighbors)[0]

    monkeypatch.setattr(pipeline, "remove_statistical_outliers", stat)
    monkeypatch.setattr(pipeline, "remove_radius_outliers", rad)
    scan, ref = O.contaminated_sphere(2000, 40, 1), O.contaminated_sphere(1500, 30, 2)
    sn, rn = np.arange(scan.size, dtype=np.float64).reshape(-1, 3), -np.arange(ref.size, dtype=np.float64).reshape(-1, 3)
    pipe = RegistrationPipeline(scan=scan, scan_normals=sn, ref=ref, ref_normals=rn)
    assert pipe.scan_kept is None and pipe.ref_kept is None
    pipe.remove_outliers("statistical", nb_neighbors=8, std_ratio=1.0)
    assert calls == [("statistical", 8, 1.0)] * 2
    want = O.statistical(scan, 8, 1.0)[0]
    assert 0 < want.size < scan.shape[0]
    assert np.array_equal(pipe.scan_kept, want) and np.array_equal(pipe.scan, scan[want]) and np.array_equal(pipe.scan_normals, sn[want])
    want = O.statistical(ref, 8, 1.0)[0]
    assert np.array_equal(pipe.ref_kept, want) and np.array_equal(pipe.ref, ref[want]) and np.array_equal(pipe.ref_normals, rn[want])

    # keypoints index into the clouds: the stage refuses to pull the clouds from under them ...
    pipe.scan_keypoints, pipe.ref_keypoints = np.arange(10), np.arange(10)
    before = pipe.scan.copy()
    with pytest.raises(ValueError, match="scan_keypoints"):
        pipe.remove_outliers("radius", radius=0.05, min_neighbors=3)
    assert np.array_equal(pipe.scan, before) and pipe.scan_keypoints is not None
    # ... unless told to, and then clears them (descriptors and matches with them)
    pipe.scan_descriptors, pipe.matches = np.zeros((10, 4)), (np.arange(3), np.arange(3))
    pipe.remove_outliers("radius", radius=0.05, min_neighbors=3, force_recompute=True)
    assert calls[-1] == ("radius", 0.05, 3)
    assert pipe.scan_keypoints is None and pipe.ref_keypoints is None and pipe.scan_descriptors is None and pipe.matches is None
    assert np.array_equal(pipe.scan, before[pipe.scan_kept]) and np.array_equal(pipe.scan_kept, O.radius(before, 0.05, 3)[0])

    with pytest.raises(ValueError, match="Incorrect outlier removal"):
        pipe.remove_outliers("median")
    with pytest.raises(ValueError, match="radius"):
        pipe.remove_outliers("radius")


# ---- the build ----------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_do_not_spill():
    """From the compiler's resource remarks of the build (csrc/build/outliers.remarks), as tests/test_abi.py reads them: no kernel
    of K20 spills a register or uses scratch memory, and the mean-distance pass stays within 32 VGPRs (30)."""
    files = glob.glob(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "build", "outliers.remarks"))
    if not files:
        pytest.skip("no build/outliers.remarks (the library was not built by its Makefile here)")
    res, cur = {}, None
    for ln in open(files[0], errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", ln)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    for kernel, count in (("k_knn_mean_distance", 1), ("k_outlier_stats", 2), ("k_outlier_fold", 2), ("k_perm_scatter", 1)):
        # (k_perm_scatter: search_util.h's map to the caller's order, which the radius filter's counts take since k_outlier_scatter left)
        mine = [r for name, r in res.items() if re.search(r"\b" + kernel + r"\b", name)]
        assert len(mine) == count, (kernel, list(res))
        for r in mine:
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (kernel, r)
    mean = [r for name, r in res.items() if "k_knn_mean_distance" in name][0]
    assert mean["VGPRs"] <= 32, mean
