"""Harris 3D keypoints without a GPU: the NumPy statement of the definition (tests/harris_numpy.py) on hand-made cases, the
argument checks of the public functions (each raised before an engine is touched), and the way from the pipeline and the
registration script down to select_keypoints_harris."""
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import harris_numpy as H
from conftest import ROOT, synth_cloud
from shot_fpfh_amd import keypoint_selection as ks
from shot_fpfh_amd.keypoint_selection import harris_response, select_keypoints_harris


class NoEngine:
    """an engine that must not be reached: every argument check comes first"""

    def cloud(self, *a, **k):
        raise AssertionError("the engine was reached before the arguments were checked")


# ---- the statement on hand-made cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), tuple(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0))])
def test_a_plane_with_one_common_normal_has_no_keypoints(normal):
    rng = np.random.default_rng(3)
    p = np.column_stack([rng.random((1500, 2)), np.full(1500, 0.25)])
    nr = np.tile(np.array(normal), (1500, 1))
    counts, C, _ = H.tensor(p, nr, 0.08)
    assert counts.min() >= 1 and counts.max() > 20
    assert np.all(np.abs(H.det(C)) <= 1e-15 * H.trace(C) ** 3) and np.all(H.lambda_min(C) <= 1e-15 * H.trace(C))
    for method in H.TENSOR_METHODS:
        assert np.all(H.response_from(method, counts, C=C) == -1.0), method
        assert H.keypoints(p, nr, 0.08, method=method).size == 0


def _octant_corner(m=12, h=1.0 / 16):
    """three orthogonal faces of (m x m) points each, half a step away from the edges they meet at, with their exact face
    normals, and the corner point itself (normal of the z face) as point 0"""
    g = (np.arange(m) + 0.5) * h
    a, b = [v.ravel() for v in np.meshgrid(g, g, indexing="ij")]
    zero = np.zeros_like(a)
    p = np.vstack([np.zeros((1, 3)), np.column_stack([zero, a, b]), np.column_stack([a, zero, b]), np.column_stack([a, b, zero])])
    nr = np.vstack([[[0.0, 0.0, 1.0]], np.tile([1.0, 0.0, 0.0], (m * m, 1)), np.tile([0.0, 1.0, 0.0], (m * m, 1)),
                    np.tile([0.0, 0.0, 1.0], (m * m, 1))])
    return p, nr


def test_an_octant_corner_has_its_maximum_response_at_the_corner_point():
    p, nr = _octant_corner()
    r = 0.26
    counts, C, _ = H.tensor(p, nr, r)
    # by hand: the corner's ball holds na, nb, nc points of the three faces (the corner itself among the z face's), the normals
    # are unit vectors along the axes, so C = diag(na, nb, nc) / k and det C = na nb nc / k^3
    inside = (p ** 2).sum(axis=1) <= r * r
    na, nb, nc = (int((inside & (nr[:, a] == 1.0)).sum()) for a in range(3))
    k = na + nb + nc
    assert counts[0] == k and na == nb and nc == na + 1 and na > 10
    assert np.array_equal(C[0], [na / k, 0.0, 0.0, nb / k, 0.0, nc / k])
    by_hand = na * nb * nc / k ** 3
    assert abs(H.det(C)[0] - by_hand) <= 4 * H.U * by_hand
    assert abs(by_hand - 1.0 / 27.0) < 1e-3  # three balanced faces: close to the largest determinant a unit-trace matrix has
    for method in H.TENSOR_METHODS:
        res = H.response_from(method, counts, C=C)
        assert res[0] > 0 and int(np.argmax(res)) == 0 and np.all(res[1:] < res[0]), method
        assert 0 in H.keypoints(p, nr, r, method=method)


def test_harris_noble_and_lowe_agree_for_unit_normals_and_part_for_scaled_ones():
    p, nr, _ = synth_cloud(600, 11)
    counts, C, _ = H.tensor(p, nr, 0.25)
    v = {m: H.value_and_rank(m, C)[0] for m in ("harris", "noble", "lowe")}
    tr = H.trace(C)
    assert np.all(np.abs(tr - 1.0) <= 1e-13)  # unit normals: trace 1, so the three are det C
    for m in ("noble", "lowe"):
        assert np.all(np.abs(v[m] - v["harris"]) <= 1e-13), m
    for s in (2.0, 0.5):  # C -> s^2 C: harris 0.04 + s^6 det - 0.04 s^4, noble s^4 det, lowe s^2 det
        _, Cs, _ = H.tensor(p, s * nr, 0.25)
        assert np.array_equal(Cs, s * s * C)  # (a power of two: exact)
        w = {m: H.value_and_rank(m, Cs)[0] for m in ("harris", "noble", "lowe")}
        d = H.det(C)
        assert np.allclose(w["noble"], s ** 4 * d, rtol=1e-12, atol=0) and np.allclose(w["lowe"], s ** 2 * d, rtol=1e-12, atol=0)
        assert np.allclose(w["harris"], 0.04 + s ** 6 * d - 0.04 * s ** 4, rtol=0, atol=1e-13)
        assert np.all(np.abs(w["noble"] - w["lowe"]) > 1e-3 * np.abs(w["lowe"])) and np.all(np.abs(w["harris"] - w["lowe"]) > 1e-3 * np.abs(w["lowe"]))
    # normals scaled per point: two points the methods rank differently
    _, Cm, _ = H.tensor(p, nr * np.linspace(0.5, 2.0, 600)[:, None], 0.25)
    w = {m: H.value_and_rank(m, Cm)[0] for m in ("harris", "noble", "lowe")}
    assert not np.array_equal(np.argsort(w["harris"]), np.argsort(w["lowe"]))
    assert not np.array_equal(np.argsort(w["noble"]), np.argsort(w["lowe"]))


def test_the_sign_of_a_normal_does_not_reach_the_tensor():
    p, nr, rng = synth_cloud(500, 13)
    flip = np.where(rng.random(500) < 0.5, -1.0, 1.0)[:, None]
    a, b = H.tensor(p, nr, 0.2), H.tensor(p, nr * flip, 0.2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for method in H.TENSOR_METHODS:
        assert np.array_equal(H.keypoints(p, nr, 0.2, method=method), H.keypoints(p, nr * flip, 0.2, method=method))


def test_rejections_of_the_statement():
    p, nr, _ = synth_cloud(400, 17)
    counts, C, _ = H.tensor(p, nr, 0.15)
    for method in H.TENSOR_METHODS:
        res = H.response_from(method, counts, C=C, min_neighbors=8)
        assert np.all(res[counts < 8] == -1.0) and np.all((res > 0) | (res == -1.0))
        med = float(np.median(res[res > 0]))
        half = H.response_from(method, counts, C=C, threshold=med, min_neighbors=8)
        assert (half > 0).sum() == (res > med).sum() and abs(2 * (half > 0).sum() - (res > 0).sum()) <= 1
    zero = np.zeros_like(nr)  # no normals at all: trace 0, rejected, and near no threshold
    counts, C0, _ = H.tensor(p, zero, 0.15)
    for method in H.TENSOR_METHODS:
        assert np.all(H.response_from(method, counts, C=C0, min_neighbors=1) == -1.0)
        assert not H.near_a_threshold(method, C=C0).any()
    with pytest.raises(ValueError):
        H.response_from("harris", counts, C=C, threshold=-0.1)
    cur = H.response(p, None, 0.15, "curvature")
    assert np.all((cur == -1.0) | ((cur > 0) & (cur <= 1.0 / 3.0 + 1e-12))) and (cur > 0).sum() > 100


# ---- the public functions: every check before an engine is needed -----------------------------------------------------
def test_arguments_are_checked_before_anything_is_uploaded():
    p, nr, _ = synth_cloud(50, 19)
    eng = NoEngine()
    bad = nr.copy()
    bad[7, 1] = np.nan
    inf = nr.copy()
    inf[0, 0] = np.inf
    for call in (lambda **kw: select_keypoints_harris(p, kw.pop("normals", nr), 0.2, engine=eng, **kw),
                 lambda **kw: harris_response(p, kw.pop("normals", nr), 0.2, engine=eng, **kw)):
        with pytest.raises(ValueError, match="threshold"):
            call(threshold=-1e-9)
        with pytest.raises(ValueError, match="threshold"):
            call(threshold=float("nan"))
        with pytest.raises(ValueError, match="unknown Harris response method"):
            call(method="shi")
        with pytest.raises(ValueError, match="non-finite"):
            call(normals=bad)
        with pytest.raises(ValueError, match="non-finite"):
            call(normals=inf)
        for method in H.TENSOR_METHODS:
            with pytest.raises(ValueError, match="normals"):
                call(normals=None, method=method)
        with pytest.raises(ValueError, match="min_neighbors"):
            call(min_neighbors=0)
        with pytest.raises(ValueError, match="shape"):
            call(normals=nr[:10])
        with pytest.raises(AssertionError, match="engine was reached"):  # (everything in order: the call goes on to the engine)
            call(normals=None, method="curvature")
    with pytest.raises(ValueError, match="radius"):
        select_keypoints_harris(p, nr, -0.1, engine=eng)
    with pytest.raises(ValueError, match="non_max_radius"):
        select_keypoints_harris(p, nr, 0.1, float("inf"), engine=eng)
    with pytest.raises(ValueError, match="radius"):
        harris_response(p, nr, 0.0, engine=eng)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        select_keypoints_harris(p[:, :2], nr, 0.1, engine=eng)
    with pytest.raises(ValueError, match="two points"):
        select_keypoints_harris(p[:1], nr[:1], engine=eng)


def test_an_empty_cloud_gives_empty_arrays():
    e = np.zeros((0, 3))
    idx = select_keypoints_harris(e, e, 0.1, engine=NoEngine())
    assert idx.dtype == np.int64 and idx.shape == (0,)
    idx, res = select_keypoints_harris(e, None, method="curvature", return_response=True, engine=NoEngine())
    assert idx.shape == (0,) and res.dtype == np.float64 and res.shape == (0,)
    assert harris_response(e, e, 0.1, engine=NoEngine()).shape == (0,)


class StatementCloud:
    """the calls the public functions make on a Cloud, answered by the statement"""

    def __init__(self, log, points, normals):
        self.log, self.p, self.nr, self.n = log, points, normals, points.shape[0]

    def resolution(self, points):
        return H.N.resolution(points)

    def harris_response(self, radius, method, threshold, min_neighbors):
        self.log.append(("response", radius, method, threshold, min_neighbors))
        return H.response(self.p, self.nr, radius, method, threshold, min_neighbors)

    def harris_keypoints(self, radius, non_max_radius, method, threshold, min_neighbors, return_response):
        self.log.append(("keypoints", radius, non_max_radius, method, threshold, min_neighbors, return_response))
        res = H.response(self.p, self.nr, radius, method, threshold, min_neighbors)
        idx = H.N.select(self.p, res, radius if non_max_radius is None else non_max_radius, min_neighbors)
        return (idx, res) if return_response else idx

    def free(self):
        self.log.append("free")


class StatementEngine:
    def __init__(self):
        self.log = []

    def cloud(self, points, normals=None):
        return StatementCloud(self.log, points, normals)


def test_the_public_functions_hand_their_arguments_down():
    p, nr, _ = synth_cloud(300, 23)
    eng = StatementEngine()
    idx, res = select_keypoints_harris(p, nr, 0.2, 0.3, method="tomasi", threshold=0.01, min_neighbors=4, return_response=True, engine=eng)
    assert eng.log == [("keypoints", 0.2, 0.3, "tomasi", 0.01, 4, True), "free"]
    assert np.array_equal(idx, H.keypoints(p, nr, 0.2, 0.3, "tomasi", 0.01, 4)) and res.shape == (300,)
    eng.log.clear()
    idx = select_keypoints_harris(p, nr, engine=eng)  # automatic radius: 6 x the resolution; one radius for both passes
    assert eng.log[0][:3] == ("keypoints", 6.0 * H.N.resolution(p), None) and eng.log[0][3:] == ("harris", 0.0, 5, False)
    assert np.array_equal(idx, H.keypoints(p, nr, 6.0 * H.N.resolution(p)))
    eng.log.clear()
    res = harris_response(p, None, 0.2, method="curvature", engine=eng)
    assert eng.log == [("response", 0.2, "curvature", 0.0, 5), "free"] and np.array_equal(res, H.response(p, None, 0.2, "curvature"))
    twice = np.vstack([p[:50], p[:50]])
    with pytest.raises(ValueError, match="resolution"):
        select_keypoints_harris(twice, np.vstack([nr[:50], nr[:50]]), engine=eng)
    assert eng.log[-1] == "free"


# ---- the public surface ------------------------------------------------------------------------------------------------
def test_all_signatures_and_choices():
    for name in ("harris_response", "select_keypoints_harris"):
        assert name in ks.__all__
    q = inspect.signature(select_keypoints_harris).parameters
    assert list(q) == ["points", "normals", "radius", "non_max_radius", "method", "threshold", "min_neighbors", "return_response", "engine"]
    assert [q[k].default for k in list(q)[1:]] == [None, None, None, "harris", 0.0, 5, False, None]
    assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(q)[4:])
    q = inspect.signature(harris_response).parameters
    assert list(q) == ["points", "normals", "radius", "method", "threshold", "min_neighbors", "engine"]
    assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(q)[3:])

    from shot_fpfh_amd import Cloud
    from shot_fpfh_amd.engine import HARRIS_METHODS, harris_method_id

    assert HARRIS_METHODS == H.METHODS and [harris_method_id(m) for m in H.METHODS] == [0, 1, 2, 3, 4]
    q = inspect.signature(Cloud.harris_response).parameters
    assert list(q) == ["self", "radius", "method", "threshold", "min_neighbors", "return_counts", "return_tensor"]
    q = inspect.signature(Cloud.harris_keypoints).parameters
    assert list(q) == ["self", "radius", "non_max_radius", "method", "threshold", "min_neighbors", "return_response"]
    assert q["non_max_radius"].default is None


def test_the_pipeline_reaches_select_keypoints_harris(monkeypatch):
    from shot_fpfh_amd import RegistrationPipeline

    calls = []

    def record(points, normals=None, radius=None, non_max_radius=None, **kw):
        calls.append((points, normals, radius, non_max_radius, kw))
        return np.arange(2, dtype=np.int64)

    monkeypatch.setattr(ks, "select_keypoints_harris", record)
    p, nr, _ = synth_cloud(40, 29)
    q, nq, _ = synth_cloud(30, 31)
    pipe = RegistrationPipeline(scan=p, scan_normals=nr, ref=q, ref_normals=nq)
    pipe.select_keypoints("harris", neighborhood_size=0.03)
    assert [c[0] is x and c[1] is y for c, (x, y) in zip(calls, ((p, nr), (q, nq)))] == [True, True]
    assert calls[0][2:] == (0.03, None, {"method": "harris", "threshold": 0.0, "min_neighbors": 5})
    assert np.array_equal(pipe.scan_keypoints, [0, 1]) and np.array_equal(pipe.ref_keypoints, [0, 1])
    calls.clear()
    pipe.select_keypoints("harris", neighborhood_size=0.05, min_n_neighbors=9, harris_method="lowe", harris_threshold=0.002,
                          harris_non_max_radius=0.07, force_recompute=True)
    assert calls[1][2:] == (0.05, 0.07, {"method": "lowe", "threshold": 0.002, "min_neighbors": 9}) and calls[1][1] is nq
    calls.clear()
    pipe.select_keypoints("harris", harris_method="curvature", force_recompute=True)  # needs no normals and gets none
    assert calls[0][1] is None and calls[0][2] is None and calls[0][4]["method"] == "curvature"
    bare = RegistrationPipeline(scan=p, scan_normals=nr, ref=q, ref_normals=None)
    calls.clear()
    with pytest.raises(ValueError, match="ref_normals is None"):
        bare.select_keypoints("harris", neighborhood_size=0.03, harris_method="tomasi")
    assert not calls and bare.scan_keypoints is None
    bare.select_keypoints("harris", neighborhood_size=0.03, harris_method="curvature")
    assert len(calls) == 2
    q = inspect.signature(RegistrationPipeline.select_keypoints).parameters
    for name, default in (("harris_method", "harris"), ("harris_threshold", 0.0), ("harris_non_max_radius", None)):
        assert q[name].kind is inspect.Parameter.KEYWORD_ONLY and q[name].default == default


def _cli():
    import importlib.util

    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_takes_harris_and_reaches_select_keypoints_harris(monkeypatch):
    mod = _cli()
    a = mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--keypoints", "harris"])
    assert (a.keypoints, a.harris_method, a.harris_threshold, a.harris_non_max_radius, a.keypoint_size) == ("harris", "harris", 0.0, None, None)
    argv = ["a.ply", "b.ply", "--radius", "0.1", "--keypoints", "harris", "--keypoint-size", "0.04", "--harris-method", "noble",
            "--harris-threshold", "0.001", "--harris-non-max-radius", "0.06", "--min-n-neighbors", "7"]
    a = mod.parse_args(argv)
    assert (a.harris_method, a.harris_threshold, a.harris_non_max_radius, a.keypoint_size) == ("noble", 0.001, 0.06, 0.04)
    for bad in (["--harris-method", "shi"], ["--harris-threshold", "-0.1"]):
        with pytest.raises(SystemExit):
            mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--keypoints", "harris"] + bad)

    class Reached(Exception):
        pass

    calls = []

    def record(points, normals=None, radius=None, non_max_radius=None, **kw):
        calls.append((normals is not None, radius, non_max_radius, kw))
        if len(calls) == 2:
            raise Reached
        return np.arange(2, dtype=np.int64)

    clouds = {"a.ply": synth_cloud(40, 29)[:2], "b.ply": synth_cloud(30, 31)[:2]}
    monkeypatch.setattr(mod, "get_data", lambda path, **kw: clouds[path])
    monkeypatch.setattr(ks, "select_keypoints_harris", record)
    with pytest.raises(Reached):
        mod.main(argv)
    assert calls == [(True, 0.04, 0.06, {"method": "noble", "threshold": 0.001, "min_neighbors": 7})] * 2


def test_header_and_prototype_table_carry_the_two_entry_points():
    from shot_fpfh_amd import _ffi

    text = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name in ("sf_harris_response", "sf_harris_keypoints"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _ffi.SIGNATURES
        assert hasattr(_ffi.load(), name)
    assert [int(v) for v in re.search(r"SF_HARRIS_HARRIS = (\d), SF_HARRIS_NOBLE = (\d), SF_HARRIS_LOWE = (\d), SF_HARRIS_TOMASI = (\d), "
                                      r"SF_HARRIS_CURVATURE = (\d)", text).groups()] == [0, 1, 2, 3, 4]
    assert "serves both detectors" in text  # (the suppression of an existing score array stays sf_iss_select)


def test_the_new_kernels_do_not_spill():
    """From the compiler's resource remarks of the build (csrc/build/harris.remarks), as tests/test_abi.py reads them for the
    hot kernels: none of k_harris_tensor (the sweep), k_harris_response (one eigen-solve per lane at most) and
    k_harris_normals_soa spills a register or uses scratch memory, and the sweep keeps eight waves per SIMD."""
    files = glob.glob(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "build", "harris.remarks"))
    assert files, "no csrc/build/harris.remarks: the build that made the library this file loads writes it"
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
    for kernel in ("k_harris_tensor", "k_harris_response", "k_harris_normals_soa"):
        mine = [r for name, r in res.items() if kernel + "(" in name]
        assert len(mine) == 1, (kernel, list(res))
        assert mine[0]["VGPRs Spill"] == 0 and mine[0]["SGPRs Spill"] == 0 and mine[0]["ScratchSize"] == 0, (kernel, mine[0])
    sweep = [r for name, r in res.items() if "k_harris_tensor(" in name][0]
    assert sweep["Occupancy"] == 8 and sweep["LDS Size"] == 6144, sweep
