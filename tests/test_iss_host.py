"""ISS keypoints, the part that needs no GPU: argument errors, the public surface, the compiler's resource listing of the
two new kernels, and the NumPy statement of the definition (tests/iss_numpy.py) on hand-made cases."""
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import iss_numpy as N
from conftest import ROOT
from shot_fpfh_amd import keypoint_selection as ks
from shot_fpfh_amd.keypoint_selection import cloud_resolution, iss_saliency, select_keypoints_iss


def _pts(n=50, seed=0):
    return np.random.default_rng(seed).random((n, 3))


# ---- argument errors (all raised before a device is asked for) ---------------------------------------------------------
@pytest.mark.parametrize("radius", [0.0, -0.1, float("nan"), float("inf")])
def test_radii_must_be_positive_and_finite(radius):
    with pytest.raises(ValueError):
        iss_saliency(_pts(), radius)
    with pytest.raises(ValueError):
        select_keypoints_iss(_pts(), radius, 0.1)
    with pytest.raises(ValueError):
        select_keypoints_iss(_pts(), 0.1, radius)


@pytest.mark.parametrize("gamma", [0.0, -0.5, 1.0000001, float("nan")])
def test_gammas_must_lie_in_0_1(gamma):
    with pytest.raises(ValueError):
        iss_saliency(_pts(), 0.1, gamma_21=gamma)
    with pytest.raises(ValueError):
        iss_saliency(_pts(), 0.1, gamma_32=gamma)
    with pytest.raises(ValueError):
        select_keypoints_iss(_pts(), 0.1, 0.1, gamma, 0.9)
    with pytest.raises(ValueError):
        select_keypoints_iss(_pts(), 0.1, 0.1, 0.9, gamma)


def test_min_neighbors_must_be_at_least_one():
    with pytest.raises(ValueError):
        iss_saliency(_pts(), 0.1, min_neighbors=0)
    with pytest.raises(ValueError):
        select_keypoints_iss(_pts(), 0.1, 0.1, min_neighbors=0)


def test_points_must_be_n_by_3():
    with pytest.raises(ValueError):
        select_keypoints_iss(np.zeros((10, 2)), 0.1, 0.1)
    with pytest.raises(ValueError):
        cloud_resolution(np.zeros(9))


def test_automatic_radii_need_two_points():
    for kwargs in ({}, {"salient_radius": 0.1}, {"non_max_radius": 0.1}):
        with pytest.raises(ValueError):
            select_keypoints_iss(np.zeros((1, 3)), **kwargs)
    with pytest.raises(ValueError):
        cloud_resolution(np.zeros((1, 3)))


def test_an_empty_cloud_gives_an_empty_int64_array():
    idx = select_keypoints_iss(np.zeros((0, 3)), 0.1, 0.1)
    assert idx.dtype == np.int64 and idx.shape == (0,)
    idx = select_keypoints_iss(np.zeros((0, 3)))  # (nothing to take a resolution of, nothing to raise about)
    assert idx.dtype == np.int64 and idx.shape == (0,)
    idx, sal = select_keypoints_iss(np.zeros((0, 3)), 0.1, 0.1, return_saliency=True)
    assert idx.shape == (0,) and sal.dtype == np.float64 and sal.shape == (0,)
    assert iss_saliency(np.zeros((0, 3)), 0.1).shape == (0,)


# ---- the public surface -----------------------------------------------------------------------------------------------
def test_all_signatures_and_choices():
    for name in ("cloud_resolution", "iss_saliency", "select_keypoints_iss"):
        assert name in ks.__all__
    p = inspect.signature(select_keypoints_iss).parameters
    assert list(p) == ["points", "salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors", "return_saliency", "engine"]
    assert [p[k].default for k in list(p)[1:]] == [None, None, 0.975, 0.975, 5, False, None]
    assert p["return_saliency"].kind is inspect.Parameter.KEYWORD_ONLY and p["engine"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(iss_saliency).parameters
    assert list(p) == ["points", "salient_radius", "gamma_21", "gamma_32", "min_neighbors", "engine"]
    assert p["engine"].kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(cloud_resolution).parameters
    assert list(p) == ["points", "engine"] and p["engine"].kind is inspect.Parameter.KEYWORD_ONLY

    from shot_fpfh_amd import Cloud, RegistrationPipeline

    for method in ("resolution", "iss_saliency", "iss_select", "iss_keypoints"):
        assert callable(getattr(Cloud, method))
    src = inspect.getsource(RegistrationPipeline.select_keypoints)
    assert '"iss"' in src
    one = np.zeros((1, 3))
    pipe = RegistrationPipeline(scan=one, scan_normals=one, ref=one, ref_normals=one)
    with pytest.raises(ValueError):  # "iss" is a known choice: what fails is the single point's missing resolution
        pipe.select_keypoints("iss")
    with pytest.raises(ValueError, match="Incorrect keypoint selection"):
        pipe.select_keypoints("isss")


def test_cli_takes_iss():
    import importlib.util

    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--keypoints", "iss", "--iss-non-max-radius", "0.02",
                        "--iss-gamma21", "0.9", "--iss-gamma32", "0.8"])
    assert (a.keypoints, a.iss_non_max_radius, a.iss_gamma21, a.iss_gamma32, a.keypoint_size) == ("iss", 0.02, 0.9, 0.8, None)
    a = mod.parse_args(["a.ply", "b.ply", "--radius", "0.1", "--keypoints", "iss"])
    assert (a.iss_non_max_radius, a.iss_gamma21, a.iss_gamma32) == (None, 0.975, 0.975)


def test_header_and_prototype_table_carry_the_three_entry_points():
    from shot_fpfh_amd import _ffi

    text = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name in ("sf_iss_saliency", "sf_iss_select", "sf_iss_keypoints"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _ffi.SIGNATURES
        assert hasattr(_ffi.load(), name)


def test_the_new_kernels_do_not_spill():
    """From the compiler's resource remarks of the build (csrc/build/iss.remarks), as tests/test_abi.py reads them for the
    hot kernels: neither k_iss_saliency (one 3 x 3 eigen-solve per lane) nor k_iss_nms (the sweep) spills a register or
    uses scratch memory."""
    files = glob.glob(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "build", "iss.remarks"))
    if not files:
        pytest.skip("no build/iss.remarks (the library was not built by its Makefile here)")
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
    for kernel in ("k_iss_saliency", "k_iss_nms"):
        mine = [r for name, r in res.items() if kernel + "(" in name]
        assert len(mine) == 1, (kernel, list(res))
        assert mine[0]["VGPRs Spill"] == 0 and mine[0]["SGPRs Spill"] == 0 and mine[0]["ScratchSize"] == 0, (kernel, mine[0])


# ---- the NumPy statement on hand-made cases ------------------------------------------------------------------------------
def _corner(spacings=(0.05, 0.04, 0.03)):
    """A cube corner at the origin sampled on its three faces (point 0 is the corner).  The axes are sampled at three
    different spacings: a corner sampled alike on all three faces has e1 == e2 by symmetry, which the rule rejects."""
    gx, gy, gz = [np.arange(0, int(0.5 / s) + 1) * s for s in spacings]

    def face(u, v):
        return [w.reshape(-1) for w in np.meshgrid(u, v, indexing="ij")]

    (a1, b1), (a2, b2), (a3, b3) = face(gx, gy), face(gx, gz), face(gy, gz)
    p = np.vstack([np.column_stack([a1, b1, 0 * a1]), np.column_stack([a2, 0 * a2, b2]), np.column_stack([0 * a3, a3, b3])])
    return np.unique(p, axis=0)  # (sorted: the origin comes first)


def test_numpy_statement_cube_corner_is_salient():
    p = _corner()
    assert np.array_equal(p[0], [0, 0, 0])
    counts, e = N.ball_eigenvalues(p, 0.16)
    sal = N.saliency_from(counts, e)
    assert sal[0] > 0 and sal[0] == e[0, 2] and e[0, 2] > 0.2 * e[0, 0]  # a genuinely three-dimensional ball
    face = np.flatnonzero((p[:, 2] == 0) & (p[:, 0] >= 0.2) & (p[:, 1] >= 0.2) & (p[:, 0] <= 0.3) & (p[:, 1] <= 0.3))
    assert face.size and np.all(sal[face] == -1.0)  # the inside of a face is flat
    kp = N.keypoints(p, 0.16, 0.11)
    assert kp.size and kp.dtype == np.int64 and np.all(np.diff(kp) > 0)
    assert np.all(np.sum(p[kp] == 0, axis=1) >= 1) and np.all(sal[kp] > 0)  # every keypoint lies on an edge or at the corner
    # the same corner sampled alike on all three faces: two equal eigenvalues, not salient
    sym = _corner((0.05, 0.05, 0.05))
    assert N.saliency(sym, 0.16)[0] == -1.0


def test_numpy_statement_flat_patch_and_line_are_not_salient():
    g = np.arange(20) / 16.0
    a, b = [v.reshape(-1) for v in np.meshgrid(g, g, indexing="ij")]
    plane = np.column_stack([a, b, np.full(a.size, 0.25)])
    counts, e = N.ball_eigenvalues(plane, 0.2)
    assert np.all(e[:, 2] <= N.FLOOR * e[:, 0])  # e3 = 0 up to rounding: under the floor
    assert np.all(N.saliency_from(counts, e) == -1.0)
    assert N.keypoints(plane, 0.2, 0.15).size == 0
    line = np.arange(40)[:, None] / 32.0 * np.array([[1.0, 0.5, 0.25]])
    assert np.all(N.saliency(line, 0.3) == -1.0)
    assert N.keypoints(line, 0.3, 0.2).size == 0


def test_numpy_statement_small_balls_and_gammas():
    rng = np.random.default_rng(3)
    p = rng.random((400, 3))
    counts, e = N.ball_eigenvalues(p, 0.12)
    sal = N.saliency_from(counts, e, min_neighbors=5)
    assert np.all(sal[counts < 5] == -1.0)
    assert np.all(N.saliency_from(counts, e, gamma_21=1e-6) == -1.0) and np.all(N.saliency_from(counts, e, gamma_32=1e-6) == -1.0)
    ok = sal > 0
    assert ok.any() and np.array_equal(sal[ok], e[ok, 2])


def test_numpy_statement_exact_duplicates_are_kept_or_dropped_together():
    rng = np.random.default_rng(4)
    base = rng.random((600, 3))
    p = np.vstack([base, base[:100]])  # point 600 + i duplicates point i
    sal = N.saliency(p, 0.15)
    assert np.array_equal(sal[:100], sal[600:])  # same ball -- but the sums run in another order only if the lists differ
    kp = set(N.select(p, sal, 0.1).tolist())
    assert kp
    for i in range(100):
        assert (i in kp) == (600 + i in kp)
    # a score with many exact ties and negatives: every maximum of a tie is kept
    score = (np.arange(p.shape[0]) % 7 - 2).astype(np.float64)
    kp = N.select(p, score, 0.1, min_neighbors=1)
    assert kp.size and np.all(score[kp] > 0)
    far = N.select(p, score, 10.0, min_neighbors=1)  # one ball holds everything: exactly the points of the top value
    assert np.array_equal(far, np.flatnonzero(score == 4))
