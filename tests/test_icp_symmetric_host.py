"""Symmetric point-to-plane ICP (K19) without a GPU: the NumPy statement (tests/icp_symmetric_numpy.py) against the cost it descends
and against the motions it must recover, its indifference to the sign of either cloud's normals, the layout of the header, the
binding and the reader, the argument checks of shot_fpfh_amd.icp.icp_symmetric, and the accuracy the mode is for."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

import gicp_numpy as G
import icp_symmetric_numpy as Y
from conftest import ROOT
from test_hip_gicp import D_MAX, one_pass_set

ULP = 2.0**-52


def pairs_at_the_true_motion(m=2000):
    s = one_pass_set()
    label, R, t = s["states"][1]
    return s, s["scan"][:m], s["na"][:m], R, t


# ---- the layout ---------------------------------------------------------------------------------------------------------------------
def test_layout_of_the_header_the_binding_and_the_reader():
    from shot_fpfh_amd import _ffi
    from shot_fpfh_amd.icp import _MODES, _PairSums, _SYMMETRIC

    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shotfpfh.h")).read(), flags=re.S)
    m = re.search(r"int\s+sf_icp_accumulate_symmetric\s*\(([^;]*)\)\s*;", code)
    assert m, "include/shotfpfh.h does not declare sf_icp_accumulate_symmetric"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 12 == len(_ffi.SIGNATURES["sf_icp_accumulate_symmetric"][1])
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "ref", "pts_dev", "nrm_dev", "sel_dev", "m", "Rt", "d_max", "loss",
                                                           "scale", "trim", "sums"]
    assert _SYMMETRIC not in _MODES.values() and _SYMMETRIC not in (0, 1, 2, 3) and len(_MODES) == 3  # 3 stays an error of the shared calls
    s, a, na, R, t = pairs_at_the_true_motion()
    want = Y.sums(2, 0.01, 0.8, a, na, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"])
    v = want["vec"]
    got = _PairSums(v, _SYMMETRIC)
    count, gtg, gth, abs_h, sq = Y.unpack(v)
    assert 0 < want["rank"] <= got.count == count < want["n0"] and (got.inside, got.rank, got.cut) == (want["n0"], want["rank"], want["cut"])
    assert got.sum_w == v[7] and got.sum_wr2 == v[46] and np.array_equal(got.sum_wp, v[40:43]) and np.array_equal(got.sum_wq, v[43:46])
    assert np.array_equal(got.sum_p, v[1:4]) and np.array_equal(got.sum_q, v[4:7])
    assert np.array_equal(got.gtg, gtg) and np.array_equal(got.gth, gth) and got.abs_h == abs_h > 0 and got.sq_dist == sq > 0
    assert not v[Y.UNUSED].any()


# ---- the terms against the cost -----------------------------------------------------------------------------------------------------
def test_right_hand_side_is_minus_half_the_gradient_and_the_matrix_is_definite():
    """Over FIXED pairs and fixed mean normals n the cost is E(x) = sum (h_i - g_i . x)^2 = sum h(x)^2 with
    h_i(x) = (b - p) . n - a~ . ((p + b) x n) - t~ . n, the paper's linearised residual: E is a quadratic, so central differences
    of it are exact up to rounding, 2^-53 E / e per component at the step e."""
    s, a, na, R, t = pairs_at_the_true_motion()
    p, b, n, d, d2, dot = Y.pairs(a, na, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"])
    assert p.shape[0] > 1000
    tm, mg, r2 = Y.terms(0, 1.0, a, na, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"])
    count, gtg, gth, abs_h, sq = Y.unpack(G.fsum_cols(tm))
    g = np.hstack([np.cross(p + b, n), n])
    h = np.einsum("ij,ij->i", b - p, n)
    assert np.allclose(g.T @ g, gtg, rtol=1e-12, atol=1e-12) and np.allclose(g.T @ h, gth, rtol=1e-12, atol=1e-12)
    assert np.array_equal(r2, tm[:, 35] * tm[:, 35]) and np.isclose(abs_h, np.abs(h).sum(), rtol=1e-12)

    def cost(x):
        return float(np.sum((h - g @ x) ** 2))

    e = 1e-4
    grad = np.array([(cost(e * u) - cost(-e * u)) / (2 * e) for u in np.eye(6)])
    assert np.allclose(-0.5 * grad, gth, rtol=0, atol=64 * 2.0**-53 * cost(np.zeros(6)) / e + 1e-9 * np.abs(gth).max())
    assert np.linalg.eigvalsh(gtg).min() > 1e-6 * np.linalg.eigvalsh(gtg).max() > 0


# ---- the step -------------------------------------------------------------------------------------------------------------------------
def _one_step_on_exact_pairs(angle, t0, seed=3, n=400):
    """the step from the identity on the pairs (p, R0 p + t0) with the normals of a common surface: na random unit rows, nb = R0 na"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) - 0.5
    na = rng.standard_normal((n, 3))
    na /= np.linalg.norm(na, axis=1)[:, None]
    R0 = G.rodrigues(angle * G.TRUE_AXIS)
    b, nb = p @ R0.T + t0, na @ R0.T
    nm, _dot = Y.mean_normal(nb, na)
    g = np.hstack([np.cross(p + b, nm), nm])
    h = np.einsum("ij,ij->i", b - p, nm)
    dR, dt = Y.step(np.linalg.solve(g.T @ g, g.T @ h))
    return R0, dR, dt


@pytest.mark.parametrize("angle", [1e-3, 0.12, 0.3, 0.5])
def test_one_step_recovers_an_exact_rotation_and_a_translation_across_its_axis(angle):
    """A pure rotation, and one with a translation across its axis: the cases in which b - p has no component along the axis and
    the paper's own step is exact too.  Rounding: a 6 x 6 solve of condition ~1e2 and two products of rotations."""
    axis = G.TRUE_AXIS
    across = np.cross(axis, [0.04, -0.03, 0.05])
    for t0 in (np.zeros(3), across):
        R0, dR, dt = _one_step_on_exact_pairs(angle, t0)
        assert np.abs(dR - R0).max() <= 1e3 * ULP and np.abs(dt - t0).max() <= 1e3 * ULP, (angle, t0)


@pytest.mark.parametrize("angle", [1e-3, 0.12, 0.3, 0.5])
def test_one_step_recovers_an_exact_rotation_and_translation(angle):
    """The same with the translation of the corner sets, (0.04, -0.03, 0.05), which has a component of 0.07 along the axis: the
    whole motion in one step, to rounding.  This is what leaving t~'s component along the axis unscaled is for: the linear system is
    exact -- b - p = a~ x (p + b) + t~ holds for b = C p + (I - [a~]x)^-1 t~ with C the Cayley rotation by 2 atan|a~| about a~ -- and
    (I - [a~]x)^-1 t~ is R_h (cos theta t~) across the axis but t~ itself along it.  With the paper's dt = R_h (cos theta t~) the
    translation came out short by (1 - cos(angle / 2)) (axis . t0) axis: 5.83e-9, 8.40e-5, 5.24e-4 and 1.45e-3 at the four angles."""
    t0 = np.array([0.04, -0.03, 0.05])
    R0, dR, dt = _one_step_on_exact_pairs(angle, t0)
    print(f"angle {angle}: max|dR - R0| = {np.abs(dR - R0).max():.2e}, max|dt - t0| = {np.abs(dt - t0).max():.2e}")
    assert np.abs(dR - R0).max() <= 1e3 * ULP
    assert np.abs(dt - t0).max() <= 1e3 * ULP


def test_identical_noise_free_clouds_at_the_true_motion_do_not_move():
    scan, ref, R0, t0 = G.corner_set(0, n=600, sigma=0.0)
    world = scan @ R0.T + t0
    nw = G.knn_normals(world)
    run = Y.refine(scan, nw @ R0, world, nw, 0.15, R=R0, t=t0, max_iter=3, rms_threshold=0.0, step_tolerance=1e-12)
    assert run["iterations"] == 1 and run["converged"] and run["counts"] == [600]
    assert run["steps"][0] < 1e-12 and run["rms"] < 1e-15
    assert np.abs(run["R"] - R0).max() < 1e-14 and np.abs(run["t"] - t0).max() < 1e-14


# ---- the sign of a normal -----------------------------------------------------------------------------------------------------------
def flipped(nrm, seed):
    out = nrm.copy()
    out[np.random.default_rng(seed).random(nrm.shape[0]) < 0.5] *= -1.0
    return out


def test_flipping_normals_of_either_cloud_changes_no_sum():
    s, a, na, R, t = pairs_at_the_true_motion()
    for label, R, t in s["states"]:
        for loss, k, trim in ((0, 1.0, 1.0), (2, 0.01, 0.8)):
            want = Y.sums(loss, k, trim, a, na, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"])
            assert want["count"] > 100
            for fa, fb in ((flipped(na, 1), s["nref"]), (na, flipped(s["nref"], 2)), (flipped(na, 3), flipped(s["nref"], 4))):
                got = Y.sums(loss, k, trim, a, fa, s["ref"], fb, R, t, D_MAX, tree=s["tree"])
                assert np.array_equal(got["vec"], want["vec"]), label


def test_zero_normal_rows():
    """a zero row on one side leaves n as half the other normal; on both sides the pair is counted and fits nothing"""
    s, a, na, R, t = pairs_at_the_true_motion(500)
    zero = np.zeros_like(na)
    p, b, n, d, d2, dot = Y.pairs(a, zero, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"])
    idx = s["tree"].query(p)[1]
    assert p.shape[0] > 100 and np.array_equal(n, 0.5 * s["nref"][idx])
    v = Y.sums(0, 1.0, 1.0, a, zero, s["ref"], np.zeros_like(s["nref"]), R, t, D_MAX, tree=s["tree"])["vec"]
    assert v[0] == p.shape[0] and v[7] == v[0] and not v[8:36].any() and v[36] > 0


# ---- the arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_upload(monkeypatch):
    import shot_fpfh_amd.icp as icp
    from shot_fpfh_amd.core import RigidTransform

    def no_device(*a, **kw):
        raise AssertionError("reached the device")

    monkeypatch.setattr(icp, "_Registration", no_device)
    monkeypatch.setattr(icp, "grid_subsampling", no_device)
    monkeypatch.setattr(icp, "compute_normals", no_device)
    pts = np.random.default_rng(1).random((50, 3))
    ok = dict(scan_normals=pts, ref_normals=pts, loss="cauchy", scale=0.01)
    for kw, word in ((dict(loss="l2"), "loss"), (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"),
                     (dict(scale=float("inf")), "scale"), (dict(scale=None), "scale"), (dict(scale_start=0.0), "scale_start"),
                     (dict(scale_start=float("inf")), "scale_start"), (dict(division_factor=1.0), "division_factor"),
                     (dict(division_factor=float("nan")), "division_factor"), (dict(overlap=0.0), "overlap"), (dict(overlap=1.5), "overlap"),
                     (dict(overlap=float("nan")), "overlap"), (dict(overlap=None), "overlap"), (dict(anneal_iterations=-1), "anneal_iterations"),
                     (dict(anneal_iterations=2.5), "anneal_iterations"), (dict(step_tolerance=-1.0), "step_tolerance"),
                     (dict(ref_normals=pts[:10]), "ref normals"), (dict(scan_normals=pts[:10]), "scan normals"),
                     (dict(ref_normals=None, k_normals=2), "k_normals"), (dict(scan_normals=None, k_normals=51), "k_normals")):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            icp.icp_symmetric(pts, pts, RigidTransform(), 0.1, **args)
    with pytest.raises(ValueError, match="scan"):
        icp.icp_symmetric(pts[:, :2], pts, RigidTransform(), 0.1, **ok)
    with pytest.raises(ValueError, match="ref"):
        icp.icp_symmetric(pts, pts[:, :2], RigidTransform(), 0.1, **ok)
    with pytest.raises(AssertionError, match="reached the device"):  # loss "none" needs no scale: the first thing it does is subsample
        icp.icp_symmetric(pts, pts, RigidTransform(), 0.1, scan_normals=pts, ref_normals=pts)


def test_the_function_is_exported_with_the_signature_set_down():
    import shot_fpfh_amd
    from shot_fpfh_amd import icp

    assert "icp_symmetric" in icp.__all__ and "icp_symmetric" in shot_fpfh_amd.__all__ and shot_fpfh_amd.icp_symmetric is icp.icp_symmetric
    got = {name: (p.kind, p.default) for name, p in inspect.signature(icp.icp_symmetric).parameters.items()}
    pos, kw, none = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    assert got == dict(scan=(pos, none), ref=(pos, none), transformation_init=(pos, none), d_max=(pos, none), scan_normals=(kw, None),
                       ref_normals=(kw, None), k_normals=(kw, 20), loss=(kw, "none"), scale=(kw, None), scale_start=(kw, None),
                       division_factor=(kw, 1.4), overlap=(kw, 1.0), anneal_iterations=(kw, 10), voxel_size=(kw, 0.2), max_iter=(kw, 50),
                       rms_threshold=(kw, 1e-2), step_tolerance=(kw, 1e-9))


def test_the_host_step_is_the_statements():
    from shot_fpfh_amd.icp import _PairSums, _SYMMETRIC, _symmetric_fit

    s, a, na, R, t = pairs_at_the_true_motion()
    for label, R, t in s["states"]:
        v = Y.sums(0, 1.0, 1.0, a, na, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"])["vec"]
        found = _PairSums(v, _SYMMETRIC)
        tf = _symmetric_fit(found)
        count, gtg, gth, abs_h, sq = Y.unpack(v)
        dR, dt = Y.step(np.linalg.solve(gtg, gth))
        assert np.array_equal(tf.rotation, dR) and np.array_equal(tf.translation, dt) and np.array_equal(found.step, np.linalg.solve(gtg, gth))
    with pytest.raises(np.linalg.LinAlgError, match="d_max"):
        _symmetric_fit(_PairSums(np.zeros(48), _SYMMETRIC))
    raw = np.zeros(48)
    raw[0] = raw[7] = 6.0
    raw[8:29] = np.eye(6)[np.triu_indices(6)]
    raw[32:35] = [0.1, 0.2, 0.3]  # no rotation: the identity and t~
    tf = _symmetric_fit(_PairSums(raw, _SYMMETRIC))
    assert np.array_equal(tf.rotation, np.eye(3)) and np.array_equal(tf.translation, [0.1, 0.2, 0.3])


def test_pipeline_and_script_know_the_method(monkeypatch):
    import shot_fpfh_amd.pipeline as pipeline
    from shot_fpfh_amd.core import RigidTransform

    calls = []
    monkeypatch.setattr(pipeline, "icp_symmetric", lambda *a, **kw: calls.append((a, kw)) or "result")
    pts, nrm = np.random.default_rng(2).random((50, 3)), np.random.default_rng(3).random((50, 3))
    pipe = pipeline.RegistrationPipeline(scan=pts, scan_normals=nrm, ref=pts, ref_normals=nrm)
    start = RigidTransform()
    assert pipe.run_icp("symmetric", start, d_max=0.1, voxel_size=0.05, max_iter=7, rms_threshold=1e-5, gicp_neighbors=12) == "result"
    assert pipe.run_icp("symmetric", start, d_max=0.1, robust_loss="tukey", robust_scale=0.012, robust_scale_start=0.05, trim_overlap=0.8,
                        trim_anneal_iterations=4) == "result"
    (a1, k1), (a2, k2) = calls
    assert a1[0] is pipe.scan and a1[1] is pipe.ref and a1[2] is start and a1[3] == 0.1
    assert k1 == dict(scan_normals=pipe.scan_normals, ref_normals=pipe.ref_normals, k_normals=12, loss="none", scale=None, scale_start=None,
                      overlap=1.0, anneal_iterations=10, voxel_size=0.05, max_iter=7, rms_threshold=1e-5)
    assert (k2["loss"], k2["scale"], k2["scale_start"], k2["overlap"], k2["anneal_iterations"]) == ("tukey", 0.012, 0.05, 0.8, 4)
    with pytest.raises(ValueError, match="robust_scale"):
        pipe.run_icp("symmetric", start, d_max=0.1, robust_loss="cauchy")
    with pytest.raises(ValueError, match="robust_loss"):
        pipe.run_icp("symmetric", start, d_max=0.1, robust_scale=0.01)
    with pytest.raises(ValueError, match="ICP type"):
        pipe.run_icp("symmetrical", start, d_max=0.1)
    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    base = ["scan.ply", "ref.ply", "--radius", "0.2"]
    args = script.parse_args(base + ["--icp", "symmetric", "--icp-loss", "cauchy", "--icp-loss-scale", "0.006", "--icp-overlap", "0.8"])
    assert (args.icp, args.icp_loss, args.icp_loss_scale, args.icp_overlap) == ("symmetric", "cauchy", 0.006, 0.8)
    with pytest.raises(SystemExit):
        script.parse_args(base + ["--icp", "symmetrical"])


# ---- what it is for -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_statement_is_no_worse_than_point_to_plane_on_the_corner_sets(seed):
    """1 500 + 1 500 points, sigma = 0.002, d_max = 0.15, from the identity, 0.12 rad off, 60 iterations allowed; the normals of both
    clouds from 20 neighbours.  No margin: the ratios are 0.49, 0.67, 0.99 and 0.47."""
    scan, ref, R0, t0 = G.corner_set(seed)
    na, nref = G.knn_normals(scan), G.knn_normals(ref)
    plane = G.icp_point_to_plane(scan, ref, nref, 0.15)
    sym = Y.refine(scan, na, ref, nref, 0.15, max_iter=60, rms_threshold=0.0)
    ep, es = G.rotation_error(plane["R"], R0), G.rotation_error(sym["R"], R0)
    print(f"seed {seed}: point-to-plane {ep:.4e} ({plane['iterations']}), symmetric {es:.4e} ({sym['iterations']}), ratio {es / ep:.2f}")
    assert sym["converged"] and sym["iterations"] < 60 and es <= ep
