"""Generalized ICP on the MI355X (K16: k_icp_sums<1, 2>, sf_icp_accumulate_gicp, csrc/icp.hip) against the NumPy statement of the
definition (tests/gicp_numpy.py).

The check is split where the definition leaves rounding to the implementation.  ONE pass is held to the math.fsum value of each
of its sums within C k 2^-53 sum|term|, with an equal pair count; the whole run amplifies rounding through its dependent steps,
so its bound is ten times the definition's own sensitivity to the order of its sums, measured on the NumPy statement alone; the
iteration count and the convergence flag are exact."""
import os
import sys

import numpy as np
import pytest
from scipy.spatial import cKDTree

import gicp_numpy as G
from conftest import ROOT, load_golden, run_program

pytestmark = pytest.mark.gpu

U = 2.0**-53
D_MAX = 0.05
# Roundings that enter one term as k_icp_sums<1, 2> forms it from the loaded coordinates, for the longest chain, the column of r^T M r:
# p = ((R0 x + R1 y) + R2 z) + t, 6 per component (18); m = (R0 nx + R1 ny) + R2 nz, 5 per component (15); c = 1 - eps (1);
# S: three diagonal entries 2 - c (nb nb + m m) of 5 and three off-diagonal ones of 4 (the negation is exact) (27); the adjugate,
# six entries of two products and a difference (18); det = (S00 a00 + S01 a01) + S02 a02 (5); 1 / det (1); M = adj inv (6);
# r = b - p (3); u = M r, (.. + ..) + .. per component (15); (r0 u0 + r1 u1) + r2 u2 (5): 114.  The NumPy statement forms every
# term by the same operations in the same order, so what really differs is the order of the k additions (k - 1 roundings, each
# relative to a partial sum of magnitude <= sum|term|): C k 2^-53 sum|term| covers both with room to spare.
C_ROUNDINGS = 114
M_MAX = 65537
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def one_pass_set():
    """2 000 reference points (random float64, unit normals) and 65 537 scan points: R0 scan + t0 lies within ~0.03 of a reference
    point, so at the true motion most pairs are kept at d_max = 0.05, at the identity and 0.3 rad away a part of them."""
    if "one" not in _cache:
        rng = np.random.default_rng(2009)
        ref, nref = rng.random((2000, 3)), _unit(rng.standard_normal((2000, 3)))
        world = ref[rng.integers(0, 2000, M_MAX)] + 0.03 * rng.standard_normal((M_MAX, 3))
        r0, t0 = G.true_motion()
        scan, na = (world - t0) @ r0, _unit(rng.standard_normal((M_MAX, 3)))
        away = G.rodrigues(0.3 * np.array([1.0, 2.0, -2.0]) / 3.0) @ r0
        states = [("identity", None, None), ("true", r0, t0), ("0.3 rad", away, t0)]
        _cache["one"] = dict(ref=ref, nref=nref, scan=scan, na=na, states=states, tree=cKDTree(ref))
    return _cache["one"]


def assert_unambiguous(s, a, R, t, d_max, label):
    """nearest and second-nearest distances differ, and no distance is within 1e-9 relative of d_max: the kept set is not a
    matter of rounding"""
    d = s["tree"].query(G.move(R, t, a), k=2)[0]
    assert np.all(d[:, 1] - d[:, 0] > 1e-9 * d[:, 1]), label
    if np.isfinite(d_max):
        assert np.all(np.abs(d[:, 0] - d_max) > 1e-9 * d_max), label


def check_sums(got, want, label):
    k = want["count"]
    assert got[0] == k, (label, got[0], k)
    err = np.abs(got - want["vec"])
    bound = C_ROUNDINGS * k * U * want["abs"]
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want["abs"] > 0, err / (k * U * want["abs"]), 0.0))) if k else 0.0
    print(f"{label}: k = {k}, worst |sum - fsum| = {worst:.3g} x k 2^-53 sum|term| (bound {C_ROUNDINGS})")
    assert np.all(err <= bound), (label, np.flatnonzero(err > bound), worst)
    assert np.all(got[want["abs"] == 0] == 0)  # [7], [37..39], and everything when no pair is kept


class _Resident:
    def __init__(self, eng, scan, na, ref, nref):
        from shot_fpfh_amd.icp import _Registration

        self.reg = _Registration(scan, ref, nref, engine=eng, scan_normals=na)

    def sums(self, R, t, d_max, rows=None, eps=1e-3):
        from shot_fpfh_amd.core import RigidTransform
        from shot_fpfh_amd.icp import _GICP

        by = None if R is None else RigidTransform(R, t)
        return self.reg.pairs(_GICP, d_max, moved_by=by, rows=rows, epsilon=eps).raw

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.reg.close()


# ---- one pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, M_MAX])
def test_one_pass_equals_fsum_within_the_rounding_bound(eng, m):
    """m = 1: a single pair; 63, 64, 65: below, at and above a wave; 257: one block plus one; 65 537: one past the grid's
    256 x 256 threads, the stride loop wraps."""
    s = one_pass_set()
    a, na = s["scan"][:m], s["na"][:m]
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            assert_unambiguous(s, a, R, t, D_MAX, (m, label))
            got = dev.sums(R, t, D_MAX)
            assert np.array_equal(got, dev.sums(R, t, D_MAX))  # two calls, bit for bit
            check_sums(got, G.sums(a, na, s["ref"], s["nref"], R, t, D_MAX, tree=s["tree"]), f"m={m} {label}")
    if m == 1:  # the single pair IS kept at the true motion (the bound above is not vacuous there)
        assert G.sums(a, na, s["ref"], s["nref"], s["states"][1][1], s["states"][1][2], D_MAX, tree=s["tree"])["count"] == 1


def test_one_pass_selection_limits_and_zero_normals(eng):
    s = one_pass_set()
    n = 5000
    a, na = s["scan"][:n], s["na"][:n].copy()
    na[::7] = 0.0  # some scan points without a normal: C = I
    nref = s["nref"].copy()
    nref[::11] = 0.0
    label, R, t = s["states"][1]
    with _Resident(eng, a, na, s["ref"], nref) as dev:
        assert_unambiguous(s, a, R, t, D_MAX, "zero normals")
        for eps in (1e-3, 1.0, 1e-6):
            got = dev.sums(R, t, D_MAX, eps=eps)
            check_sums(got, G.sums(a, na, s["ref"], nref, R, t, D_MAX, eps, tree=s["tree"]), f"zero normals, eps = {eps:g}")
        # a selection with repeated ids: points AND normals go through it
        ids = np.random.default_rng(5).integers(0, n, 777)
        assert np.unique(ids).size < 777
        for lab, R2, t2 in s["states"]:
            got = dev.sums(R2, t2, D_MAX, rows=ids)
            assert np.array_equal(got, dev.sums(R2, t2, D_MAX, rows=ids))
            check_sums(got, G.sums(a[ids], na[ids], s["ref"], nref, R2, t2, D_MAX, tree=s["tree"]), f"selection {lab}")
        # no pair at all: every one of the 40 sums is zero
        none = dev.sums(R, t, 1e-7)
        assert G.sums(a, na, s["ref"], nref, R, t, 1e-7, tree=s["tree"])["count"] == 0
        assert none.shape == (40,) and not none.any()
        # every pair
        assert_unambiguous(s, a, R, t, np.inf, "inf")
        got = dev.sums(R, t, np.inf)
        assert got[0] == n
        check_sums(got, G.sums(a, na, s["ref"], nref, R, t, np.inf, tree=s["tree"]), "d_max = inf")


def test_one_pass_argument_errors(eng):
    from shot_fpfh_amd import ShotFpfhError
    from shot_fpfh_amd.icp import _GICP, _Registration

    s = one_pass_set()
    with _Resident(eng, s["scan"][:100], s["na"][:100], s["ref"], s["nref"]) as dev:
        for eps in (0.0, 1.5, float("nan")):
            with pytest.raises(ShotFpfhError, match="epsilon"):
                dev.sums(None, None, D_MAX, eps=eps)
    reg = _Registration(s["scan"][:100], s["ref"], None, engine=eng, scan_normals=s["na"][:100])  # a reference without normals
    try:
        with pytest.raises(ShotFpfhError, match="normals"):
            reg.pairs(_GICP, D_MAX)
    finally:
        reg.close()
    with pytest.raises(ValueError):
        _Registration(s["scan"][:100], s["ref"], s["nref"], engine=eng, scan_normals=s["na"][:99])


# ---- the whole run ---------------------------------------------------------------------------------------------------------------------
STEP_TOLERANCE = 2e-9


def table_set(seed):
    if seed not in _cache:
        scan, ref, r0, t0 = G.corner_set(seed)
        _cache[seed] = (scan, G.knn_normals(scan), ref, G.knn_normals(ref), r0, t0)
    return _cache[seed]


def _diff(r1, t1, r2, t2):
    return max(float(np.abs(r1 - r2).max()), float(np.abs(t1 - t2).max()))


def test_whole_run_agrees_with_the_definition(eng):
    """Seed 0 of the parity table from the identity, 60 iterations allowed.  The statement's sensitivity to the order of its sums:
    the same run on row-permuted scans with NumPy's pairwise sums instead of math.fsum, the largest difference of four."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import _GICP, _refine

    scan, na, ref, nref, r0, t0 = table_set(0)
    exact = G.icp_generalized(scan, na, ref, nref, 0.15, max_iter=60, step_tolerance=STEP_TOLERANCE)
    steps = exact["steps"]
    # the stop is not a matter of rounding: the last step is 10 x below the tolerance, the one before 10 x above it
    assert exact["converged"] and exact["iterations"] < 60 and steps[-1] * 10 <= STEP_TOLERANCE <= steps[-2] / 10, steps
    own = 0.0
    for seed in range(4):
        order = np.random.default_rng(17 + seed).permutation(scan.shape[0])
        other = G.icp_generalized(scan[order], na[order], ref, nref, 0.15, max_iter=60, step_tolerance=STEP_TOLERANCE, how="np")
        assert other["iterations"] == exact["iterations"]
        own = max(own, _diff(exact["R"], exact["t"], other["R"], other["t"]))
    calls = []
    with _Resident(eng, scan, na, ref, nref) as dev:
        real = dev.reg.pairs
        dev.reg.pairs = lambda *a, **kw: calls.append(1) or real(*a, **kw)
        tf, rms, converged = _refine(dev.reg, RigidTransform(), _GICP, 0.15, 60, 0.0, 1e-3, STEP_TOLERANCE)
    d = _diff(tf.rotation, tf.translation, exact["R"], exact["t"])
    print(f"device vs fsum statement {d:.3e} after {len(calls)} iterations; the statement's own fsum vs permuted np.sum {own:.3e}; "
          f"bound 10 x that; |R - R0| = {G.rotation_error(tf.rotation, r0):.2e}; steps {['%.1e' % x for x in steps]}")
    assert (len(calls), bool(converged)) == (exact["iterations"], True)
    assert np.isclose(rms, exact["rms"], rtol=1e-9)
    assert d <= 10 * own, (d, own)


def test_iteration_cap_and_rms_stop(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_generalized

    scan, na, ref, nref, r0, t0 = table_set(0)
    kw = dict(scan_normals=na, ref_normals=nref, voxel_size=0.01)
    tf, rms, converged = icp_generalized(scan, ref, RigidTransform(), 0.15, max_iter=2, rms_threshold=0.0, **kw)
    assert not converged and rms > 0
    tf, rms2, converged = icp_generalized(scan, ref, RigidTransform(), 0.15, max_iter=60, rms_threshold=10.0, step_tolerance=0.0, **kw)
    assert converged and rms2 < 10.0 and rms2 > rms  # stopped by the rms after ONE step: the residual of the pairs of the start


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_device_beats_point_to_point_on_the_table_sets(eng, seed):
    """Normals from the device's own k-NN pass (k_normals = 20), both methods from the identity on the same subsampled scan."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_generalized, icp_point_to_point

    scan, na, ref, nref, r0, t0 = table_set(seed)
    tg, rms, converged = icp_generalized(scan, ref, RigidTransform(), 0.15, voxel_size=0.01, max_iter=60, rms_threshold=0.0)
    tp = icp_point_to_point(scan, ref, RigidTransform(), d_max=0.15, voxel_size=0.01, max_iter=60, rms_threshold=0.0)[0]
    eg, ep = G.rotation_error(tg.rotation, r0), G.rotation_error(tp.rotation, r0)
    print(f"seed {seed}: point-to-point {ep:.2e}, generalized {eg:.2e} (rms {rms:.2e}), ratio {ep / eg:.1f}")
    assert converged and eg <= 0.5 * ep


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_returns_what_the_function_returns(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_generalized
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    scan, na, ref, nref, r0, t0 = table_set(1)
    pipe = RegistrationPipeline(scan=scan, scan_normals=na, ref=ref, ref_normals=nref)
    got = pipe.run_icp("generalized", RigidTransform(), d_max=0.15, voxel_size=0.01, max_iter=40, rms_threshold=0.0, gicp_epsilon=1e-2)
    want = icp_generalized(scan, ref, RigidTransform(), 0.15, scan_normals=na, ref_normals=nref, epsilon=1e-2, voxel_size=0.01,
                           max_iter=40, rms_threshold=0.0)
    assert np.array_equal(got[0].rotation, want[0].rotation) and np.array_equal(got[0].translation, want[0].translation)
    assert got[1:] == want[1:] and got[2]
    # the pipeline computes the scan's normals itself when it has none
    bare = RegistrationPipeline(scan=scan, scan_normals=None, ref=ref, ref_normals=nref)
    tf = bare.run_icp("generalized", RigidTransform(), d_max=0.15, voxel_size=0.01, max_iter=40, rms_threshold=0.0, gicp_neighbors=15)[0]
    assert G.rotation_error(tf.rotation, r0) < 5e-3


def test_script_runs_generalized_icp_end_to_end(eng, tmp_path):
    """scripts/register_point_clouds.py --icp generalized on the pair of test_hip_parity's script test, in a process of its own:
    the refined alignment is written, lies within the RANSAC threshold of the generating motion and is no worse than the RANSAC
    start it was given."""
    from shot_fpfh_amd.helpers import read_ply, write_ply

    g = load_golden("icp_3500.npz")
    scan_file, ref_file = str(tmp_path / "scan.ply"), str(tmp_path / "ref.ply")
    write_ply(scan_file, [g["scan"]], ["x", "y", "z"])
    write_ply(ref_file, [g["ref"], g["ref_normals"]], ["x", "y", "z", "nx", "ny", "nz"])
    out = str(tmp_path / "aligned")
    r = run_program([sys.executable, os.path.join(ROOT, "scripts", "register_point_clouds.py"), scan_file, ref_file, "--radius", "0.2",
                     "--keypoints", "subsampling", "--keypoint-size", "0.05", "--min-neighborhood-size", "10", "--ransac-draws", "2000",
                     "--ransac-threshold", "0.02", "--icp", "generalized", "--icp-dmax", "0.05", "--icp-voxel", "0.04",
                     "--icp-rms", "1e-9", "--metric-threshold", "0.01", "--write", out], timeout=300)
    assert r["rc"] == 0, r["stderr"][-2000:]
    n_scan = g["scan"].shape[0]
    truth = g["scan"] @ g["true_rotation"].T + g["true_translation"]
    err = {}
    for stage in ("ransac", "icp"):
        merged = read_ply(f"{out}_{stage}.ply")
        assert merged.shape[0] == n_scan + g["ref"].shape[0]
        err[stage] = float(np.abs(np.vstack((merged["x"], merged["y"], merged["z"])).T[:n_scan] - truth).max())
    print(f"max |aligned - truth|: RANSAC {err['ransac']:.2e}, generalized ICP {err['icp']:.2e}")
    assert err["icp"] <= 0.02 and err["icp"] <= err["ransac"]
