"""Symmetric point-to-plane ICP on the MI355X (K19: k_icp_keys<3>, k_icp_sums<PASS, 3>, sf_icp_accumulate_symmetric, csrc/icp.hip;
shot_fpfh_amd.icp.icp_symmetric) against the NumPy statement of the definition (tests/icp_symmetric_numpy.py).

The check is split as its siblings' is (tests/test_hip_gicp.py, tests/test_hip_icp_trimmed.py).  ONE pass: the pair counts -- used,
n0, rank -- and the cut EQUAL the statement's, every sum lies within C k 2^-53 sum|term| of its math.fsum value, the slots of no
pass are exactly 0.0, and two calls agree bit for bit.  The whole run is held to its iteration count and flag, and to ten times the
statement's own sensitivity to the order of its sums."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gicp_numpy as G
import icp_robust_numpy as S
import icp_symmetric_numpy as Y
import icp_trimmed_numpy as TR
import test_hip_icp_robust as H
from conftest import ROOT, load_golden, run_program
from test_hip_gicp import M_MAX, assert_unambiguous, one_pass_set, table_set

pytestmark = pytest.mark.gpu

U = 2.0**-53
D_MAX = H.D_MAX
K_ONE = H.K_ONE[S.PLANE]  # h is a length, as in mode 1: the scale of that mode's one-pass tests
# Roundings that enter one term as k_icp_sums<PASS, 3> forms it, counted as the sibling files count them: every rounding of the
# expression's tree from the loaded coordinates.
#   a component of p = ((R0 x + R1 y) + R2 z) + t: 6;  of d = b - p: 7;  of c = p + b: 7
#   a component of m = (R0 x + R1 y) + R2 z: 5;  of n = 0.5 (nb + s m): 6 (s m and 0.5 (..) are exact)
#   h = (dx nx + dy ny) + dz nz: three products of 7 + 6 + 1 = 14 and two additions: 44
#   r2 = h h: 44 + 44 + 1 = 89;  w: r2's 89 and at most 5 of its own (Geman-McClure: k k, r2 / kk, 1 + s, 1 / ., c c): 94
#   a component of c x n: two products of 7 + 6 + 1 = 14 and a difference: 29
#   w (g_a g_b): 94 + (29 + 29 + 1) + 1 = 154;  w (g_a h): 94 + (29 + 44 + 1) + 1 = 169
#   the longest chain is [46], w r2, into which r2 enters twice: 94 + 89 + 1 = 184.
# The NumPy statement forms every term by the same operations in the same order, so what really differs is the order of the k
# additions (k - 1 roundings, each relative to a partial sum of magnitude <= sum|term|): C k 2^-53 sum|term| covers both with room
# to spare, the form of bound of the sibling files.
C_ROUNDINGS = 184
STEP_TOLERANCE = 1e-8  # corner seed 0 steps ... 5.6e-6, 2.9e-10: ten times clear of the tolerance on either side (asserted below)
# Two runs at the same fixed point still differ by the rounding of their last composition (dR, dt) o (R, t): per entry of R three
# products and two additions, then the round trip through a unit quaternion (about ten operations per entry), per entry of t the
# same product and one addition; entries at most 1 in magnitude, each rounding at most 2^-53 of that: 16 of them.
LAST_COMPOSITION = 16 * 2.0**-53
SAME_AS_PLANE = list(range(0, 8)) + list(range(23, 29)) + list(range(32, 36)) + list(range(40, 47))


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


class _Resident(H._Resident):
    """`sym` is one sf_icp_accumulate_symmetric call as `_Registration.pairs` makes it"""

    def sym(self, loss, k, trim, R, t, d_max, rows=None):
        from shot_fpfh_amd.icp import _SYMMETRIC

        got = self.reg.pairs(_SYMMETRIC, d_max, moved_by=self._by(R, t), rows=rows, loss=loss, scale=k, trim=trim).raw
        assert got.shape == (48,)
        return got


def raw_call(eng, reg, loss=0, k=1.0, trim=1.0, d_max=D_MAX, m=None, ctx=True, ref=True, pts=True, nrm=True, out=True):
    """the C call itself over all rows with no motion: (return code, 48 numbers)"""
    raw = np.full(48, -1.0)
    rc = eng.lib.sf_icp_accumulate_symmetric(eng.h if ctx else None, reg.ref.h if ref else None, reg.points.ptr if pts else None,
                                             reg.normals.ptr if nrm else None, None, reg.n if m is None else m, None, float(d_max), loss,
                                             float(k), float(trim), raw.ctypes.data_as(C.c_void_p) if out else None)
    return rc, raw


def check_sums(got, loss, k, trim, a, na, ref, nref, R, t, d_max, label, tree=None):
    """`got` (48 doubles of the device) against the statement: [0], [37], [38], [47] equal, the rest within the bound over the USED
    pairs, the slots of no pass exactly 0.0.  Returns the statement's numbers."""
    want = Y.sums(loss, k, trim, a, na, ref, nref, R, t, d_max, tree=tree)
    n = want["count"]
    print(f"{label}: n0 = {got[37]:.0f} (statement {want['n0']}), rank = {got[38]:.0f} ({want['rank']}), used = {got[0]:.0f} ({n}), "
          f"cut = {got[47]!r} ({want['cut']!r})")
    assert (got[0], got[37], got[38]) == (n, want["n0"], want["rank"]), label
    assert got[47] == want["cut"] and not np.signbit(got[47]), (label, got[47], want["cut"])
    err = np.abs(got - want["vec"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want["abs"] > 0, err / (n * U * want["abs"]), 0.0))) if n else 0.0
    print(f"{label}: sum w = {got[7]:.6g}, worst |sum - fsum| = {worst:.3g} x k 2^-53 sum|term| (bound {C_ROUNDINGS})")
    assert np.all(err <= C_ROUNDINGS * n * U * want["abs"]), (label, np.flatnonzero(err > C_ROUNDINGS * n * U * want["abs"]), worst)
    assert np.all(got[want["abs"] == 0] == want["vec"][want["abs"] == 0])
    assert not got[Y.UNUSED].any()
    return want


def assert_signs_unambiguous(s, a, na, nref, R, t, d_max, label):
    """no pair's normals are within 1e-12 of perpendicular: s is not a matter of rounding"""
    dot = Y.pairs(a, na, s["ref"], nref, R, t, d_max, tree=s["tree"])[5]
    assert np.all(np.abs(dot) > 1e-12), label


# ---- one pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [S.LOSSES["none"], S.LOSSES["cauchy"]])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, M_MAX])
def test_one_pass_equals_fsum_within_the_rounding_bound(eng, m, loss):
    """m = 1: a single pair; 63, 64, 65: below, at and above a wave; 257: one block plus one; 65 537: one past the grid's
    256 x 256 threads, the stride loop wraps.  Identity, true motion and 0.3 rad away."""
    s = one_pass_set()
    a, na = s["scan"][:m], s["na"][:m]
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            assert_unambiguous(s, a, R, t, D_MAX, (m, label))
            assert_signs_unambiguous(s, a, na, s["nref"], R, t, D_MAX, (m, label))
            got = dev.sym(loss, K_ONE, 1.0, R, t, D_MAX)
            assert np.array_equal(got, dev.sym(loss, K_ONE, 1.0, R, t, D_MAX))  # two calls, bit for bit
            want = check_sums(got, loss, K_ONE, 1.0, a, na, s["ref"], s["nref"], R, t, D_MAX, f"m={m} loss {loss} {label}", tree=s["tree"])
            if m == 1 and label == "true":  # the single pair IS kept at the true motion (the bound is not vacuous there)
                assert want["count"] == 1 and got[0] == 1


def test_relations_to_point_to_plane_are_exact(eng):
    """With every normal of both clouds (0, 0, 1) and no rotation, n is (0, 0, 1) and h is mode 1's: the pass A slots, the n n^T
    block of the matrix, the n h part of the right-hand side and sum |h| are sf_icp_accumulate_robust(mode 1)'s bit for bit.  With
    zero scan normals n is half the reference's normal, and sum |h| exactly half of mode 1's."""
    s = one_pass_set()
    a = s["scan"][:5000]
    up = np.tile([0.0, 0.0, 1.0], (5000, 1))
    up_ref = np.tile([0.0, 0.0, 1.0], (s["ref"].shape[0], 1))
    with _Resident(eng, a, up, s["ref"], up_ref) as dev:
        for R, t in ((None, None), (np.eye(3), np.array([0.01, -0.02, 0.015]))):
            for loss in (S.LOSSES["none"], S.LOSSES["cauchy"]):
                plane = dev.sums(S.PLANE, loss, K_ONE, R, t, D_MAX)
                got = dev.sym(loss, K_ONE, 1.0, R, t, D_MAX)
                assert plane[0] > 100 and plane[35] > 0
                assert np.array_equal(got[SAME_AS_PLANE], plane[SAME_AS_PLANE]), (loss, np.flatnonzero(got != plane))
    with _Resident(eng, a, np.zeros_like(a), s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            plane = dev.sums(S.PLANE, 0, 1.0, R, t, D_MAX)
            got = dev.sym(0, 1.0, 1.0, R, t, D_MAX)
            assert plane[35] > 0 and got[35] == 0.5 * plane[35] and got[0] == plane[0], label
            check_sums(got, 0, 1.0, 1.0, a, np.zeros_like(a), s["ref"], s["nref"], R, t, D_MAX, f"zero scan normals {label}", tree=s["tree"])


def test_flipping_normals_of_either_cloud_changes_no_bit(eng):
    s = one_pass_set()
    a, na = s["scan"][:5000], s["na"][:5000]
    rng = np.random.default_rng(19)
    fa, fb = na.copy(), s["nref"].copy()
    fa[rng.random(fa.shape[0]) < 0.5] *= -1.0
    fb[rng.random(fb.shape[0]) < 0.5] *= -1.0
    cases = ((0, 1.0, 1.0), (S.LOSSES["cauchy"], K_ONE, 0.8))
    want = {}
    for scan_n, ref_n in ((na, s["nref"]), (fa, s["nref"]), (na, fb), (fa, fb)):
        with _Resident(eng, a, scan_n, s["ref"], ref_n) as dev:
            for label, R, t in s["states"]:
                for loss, k, trim in cases:
                    got = dev.sym(loss, k, trim, R, t, D_MAX)
                    first = want.setdefault((label, loss), got)
                    assert got[0] > 100 and np.array_equal(got, first), (label, loss)


def test_selection_with_repeats_zero_rows_and_no_rows(eng):
    s = one_pass_set()
    n = 5000
    a, na = s["scan"][:n], s["na"][:n].copy()
    na[::7] = 0.0
    nref = s["nref"].copy()
    nref[::11] = 0.0  # some pairs have a zero row on one side, some on both
    ids = np.random.default_rng(5).integers(0, n, 777)
    assert np.unique(ids).size < 777
    with _Resident(eng, a, na, s["ref"], nref) as dev:
        for label, R, t in s["states"]:
            assert_unambiguous(s, a[ids], R, t, D_MAX, label)
            got = dev.sym(S.LOSSES["cauchy"], K_ONE, 1.0, R, t, D_MAX, rows=ids)
            assert np.array_equal(got, dev.sym(S.LOSSES["cauchy"], K_ONE, 1.0, R, t, D_MAX, rows=ids))
            check_sums(got, S.LOSSES["cauchy"], K_ONE, 1.0, a[ids], na[ids], s["ref"], nref, R, t, D_MAX, f"selection {label}", tree=s["tree"])
        label, R, t = s["states"][1]
        check_sums(dev.sym(0, 1.0, 0.5, R, t, D_MAX), 0, 1.0, 0.5, a, na, s["ref"], nref, R, t, D_MAX, "zero rows, all", tree=s["tree"])
        none = dev.sym(0, 1.0, 0.5, R, t, D_MAX, rows=np.zeros(0, dtype=np.int64))  # an empty selection
        assert none.shape == (48,) and not none.any()
        none = dev.sym(0, 1.0, 0.5, R, t, 1e-7)  # no pair inside d_max
        assert Y.sums(0, 1.0, 0.5, a, na, s["ref"], nref, R, t, 1e-7, tree=s["tree"])["n0"] == 0 and not none.any()
        rc, raw = raw_call(eng, dev.reg, m=0)
        assert rc == 0 and not raw.any()


@pytest.mark.parametrize("loss", [S.LOSSES["none"], S.LOSSES["tukey"]])
def test_trimmed_pass_equals_the_statement(eng, loss):
    """n0, rank, used count and the cut (`icp_trimmed_numpy.select_kth`'s) equal, the sums within the bound; a share of 1.0 launches
    no selection and equals, bit for bit, the pass whose rank is n0 with a selection."""
    s = one_pass_set()
    a, na = s["scan"][:5000], s["na"][:5000]
    same = list(range(37)) + list(range(40, 47))
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            assert_unambiguous(s, a, R, t, D_MAX, label)
            for trim in (0.5, 0.8):
                got = dev.sym(loss, K_ONE, trim, R, t, D_MAX)
                assert np.array_equal(got, dev.sym(loss, K_ONE, trim, R, t, D_MAX))
                want = check_sums(got, loss, K_ONE, trim, a, na, s["ref"], s["nref"], R, t, D_MAX, f"loss {loss} trim {trim} {label}", tree=s["tree"])
                assert want["rank"] == TR.trim_rank(trim, want["n0"]) and want["rank"] <= want["count"] < want["n0"]
            plain = dev.sym(loss, K_ONE, 1.0, R, t, D_MAX)
            check_sums(plain, loss, K_ONE, 1.0, a, na, s["ref"], s["nref"], R, t, D_MAX, f"loss {loss} trim 1.0 {label}", tree=s["tree"])
            assert plain[37] == plain[38] == plain[0] > 100 and plain[47] == 0.0
            every = dev.sym(loss, K_ONE, 1.0 - 2.0**-40, R, t, D_MAX)  # ceil((1 - 2^-40) n0) = n0: the selection runs and cuts nothing
            assert every[38] == every[37] == every[0] == plain[0] and every[47] > 0.0
            assert np.array_equal(every[same], plain[same]), (label, np.flatnonzero(every != plain))


def test_argument_errors_name_the_argument(eng):
    from shot_fpfh_amd import ShotFpfhError, _ffi
    from shot_fpfh_amd.icp import _SYMMETRIC, _Registration

    s = one_pass_set()
    nan, inf = float("nan"), float("inf")
    with _Resident(eng, s["scan"][:100], s["na"][:100], s["ref"], s["nref"]) as dev:
        for kw, word in ((dict(ctx=False), "ctx"), (dict(ref=False), "ref"), (dict(pts=False), "pts_dev"), (dict(nrm=False), "nrm_dev"),
                         (dict(out=False), "sums"), (dict(m=-1), "m (negative)"), (dict(loss=5), "loss"), (dict(loss=-1), "loss"),
                         (dict(k=0.0), "scale"), (dict(k=-1.0), "scale"), (dict(k=nan), "scale"), (dict(k=inf), "scale"),
                         (dict(trim=0.0), "trim"), (dict(trim=-0.5), "trim"), (dict(trim=1.5), "trim"), (dict(trim=nan), "trim")):
            rc, raw = raw_call(eng, dev.reg, **kw)
            assert rc != 0 and "sf_icp_accumulate_symmetric: bad argument " + word in _ffi.last_error(), (word, _ffi.last_error())
        rc, raw = raw_call(eng, dev.reg, loss=4, k=0.02, trim=0.5)
        assert rc == 0 and raw[0] > 0
        assert _SYMMETRIC != 3
        with pytest.raises(ShotFpfhError, match="mode"):  # the number 3 stays what it was: no mode of the shared calls
            dev.reg.pairs(3, D_MAX, loss=2, scale=0.02)
    with _Resident(eng, s["scan"][:100], s["na"][:100], s["ref"], None) as dev:  # a reference without normals
        with pytest.raises(ShotFpfhError, match="normals"):
            dev.sym(0, 1.0, 1.0, None, None, D_MAX)
    reg = _Registration(s["scan"][:100], s["ref"], s["nref"], engine=eng)  # a scan without normals: stopped on the host
    try:
        with pytest.raises(ValueError, match="normals"):
            reg.pairs(_SYMMETRIC, D_MAX)
    finally:
        reg.close()


# ---- the whole run ---------------------------------------------------------------------------------------------------------------------
def test_whole_run_agrees_with_the_definition(eng):
    """Corner seed 0 from the identity, 60 iterations allowed.  The statement's sensitivity to the order of its sums: the same run
    on row-permuted scans with NumPy's pairwise sums instead of math.fsum, the largest difference of four."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import _SYMMETRIC, _refine_robust

    scan, na, ref, nref, r0, t0 = table_set(0)
    args = dict(max_iter=60, rms_threshold=0.0, step_tolerance=STEP_TOLERANCE)
    exact = Y.refine(scan, na, ref, nref, 0.15, **args)
    steps = exact["steps"]
    # the stop is not a matter of rounding: the last step is 10 x below the tolerance, the one before 10 x above it
    assert exact["converged"] and exact["iterations"] < 60 and steps[-1] * 10 <= STEP_TOLERANCE <= steps[-2] / 10, steps
    own = 0.0
    for seed in range(4):
        order = np.random.default_rng(17 + seed).permutation(scan.shape[0])
        other = Y.refine(scan[order], na[order], ref, nref, 0.15, how="np", **args)
        assert other["iterations"] == exact["iterations"]
        own = max(own, H._diff(exact["R"], exact["t"], other["R"], other["t"]))
    calls = []
    with _Resident(eng, scan, na, ref, nref) as dev:
        real = dev.reg.pairs

        def pairs(*a, **kw):
            found = real(*a, **kw)
            calls.append(found.count)
            return found

        dev.reg.pairs = pairs
        tf, rms, converged = _refine_robust(dev.reg, RigidTransform(), _SYMMETRIC, 0.15, 0, 1.0, 1.0, 1.4, 60, 0.0, 1.0, STEP_TOLERANCE, 1.0, 0)
    d = H._diff(tf.rotation, tf.translation, exact["R"], exact["t"])
    print(f"device vs fsum statement {d:.3e} after {len(calls)} iterations; the statement's own fsum vs permuted np.sum {own:.3e}; "
          f"bound 10 x that; |R - R0| = {G.rotation_error(tf.rotation, r0):.4e} (statement {G.rotation_error(exact['R'], r0):.4e}); "
          f"steps {['%.1e' % x for x in steps]}")
    assert (len(calls), bool(converged)) == (exact["iterations"], True) and calls == exact["counts"]
    assert np.isclose(rms, exact["rms"], rtol=1e-9, atol=0.0)
    assert d <= 10 * own, (d, own)


def test_loss_and_overlap_run_agrees_with_the_definition(eng):
    """The clutter set through the loop of `icp_symmetric` with Cauchy and an overlap of 0.8 annealed, a fixed number of iterations:
    the used pair count of every iteration exact, R and t within ten times the statement's own sensitivity.  The run sits at its
    fixed point for its last ten iterations, where the statement's permuted runs can agree bit for bit; what then still differs is
    the rounding of the last composition, `LAST_COMPOSITION`."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import _SYMMETRIC, _refine_robust

    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    args = dict(loss=S.LOSSES["cauchy"], scale=S.SCALE, overlap=0.8, anneal_iterations=10, max_iter=20, rms_threshold=0.0, step_tolerance=0.0)
    exact = Y.refine(scan, na, ref, nref, S.D_MAX, **args)
    own = 0.0
    for seed in range(2):
        order = np.random.default_rng(17 + seed).permutation(scan.shape[0])
        other = Y.refine(scan[order], na[order], ref, nref, S.D_MAX, how="np", **args)
        own = max(own, H._diff(exact["R"], exact["t"], other["R"], other["t"]))
    calls = []
    with _Resident(eng, scan, na, ref, nref) as dev:
        real = dev.reg.pairs

        def pairs(*a, **kw):
            found = real(*a, **kw)
            calls.append(found.count)
            return found

        dev.reg.pairs = pairs
        tf, rms, converged = _refine_robust(dev.reg, RigidTransform(), _SYMMETRIC, S.D_MAX, S.LOSSES["cauchy"], S.SCALE, S.D_MAX, 1.4, 20, 0.0,
                                            1.0, 0.0, 0.8, 10)
    d = H._diff(tf.rotation, tf.translation, exact["R"], exact["t"])
    print(f"Cauchy, overlap 0.8: device vs fsum statement {d:.3e} after {len(calls)} iterations; the statement's own {own:.3e}; "
          f"|R - R0| = {G.rotation_error(tf.rotation, r0):.4e} (statement {G.rotation_error(exact['R'], r0):.4e})")
    assert calls == exact["counts"] and len(calls) == 20 and not converged
    assert np.isclose(rms, exact["rms"], rtol=1e-9, atol=0.0)
    assert d <= 10 * own + LAST_COMPOSITION, (d, own)


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_device_is_no_worse_than_the_statements_point_to_plane(eng, seed):
    """The corner sets from the identity, the statement's normals given, every scan point kept; against the point-to-plane run of the
    NumPy statement (tests/gicp_numpy.py) on the same clouds.  No margin."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_symmetric

    scan, na, ref, nref, r0, t0 = table_set(seed)
    tf, rms, converged = icp_symmetric(scan, ref, RigidTransform(), 0.15, scan_normals=na, ref_normals=nref, voxel_size=H.RUN_VOXEL,
                                       max_iter=60, rms_threshold=0.0)
    plane = G.icp_point_to_plane(scan, ref, nref, 0.15)
    es, ep = G.rotation_error(tf.rotation, r0), G.rotation_error(plane["R"], r0)
    print(f"seed {seed}: statement's point-to-plane {ep:.4e}, device symmetric {es:.4e} (rms {rms:.2e}), ratio {es / ep:.2f}")
    assert converged and es <= ep


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_returns_what_the_function_returns(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_symmetric
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    scan, na, ref, nref, r0, t0 = table_set(1)
    pipe = RegistrationPipeline(scan=scan, scan_normals=na, ref=ref, ref_normals=nref)

    def same(x, y):
        return np.array_equal(x[0].rotation, y[0].rotation) and np.array_equal(x[0].translation, y[0].translation) and x[1:] == y[1:]

    got = pipe.run_icp("symmetric", RigidTransform(), d_max=0.15, voxel_size=0.01, max_iter=40, rms_threshold=0.0)
    want = icp_symmetric(scan, ref, RigidTransform(), 0.15, scan_normals=na, ref_normals=nref, voxel_size=0.01, max_iter=40, rms_threshold=0.0)
    assert same(got, want) and got[2]
    got = pipe.run_icp("symmetric", RigidTransform(), d_max=0.15, voxel_size=0.01, max_iter=20, rms_threshold=0.0, robust_loss="cauchy",
                       robust_scale=0.006, trim_overlap=0.9, trim_anneal_iterations=5)
    want = icp_symmetric(scan, ref, RigidTransform(), 0.15, scan_normals=na, ref_normals=nref, loss="cauchy", scale=0.006, overlap=0.9,
                         anneal_iterations=5, voxel_size=0.01, max_iter=20, rms_threshold=0.0)
    assert same(got, want)
    # the pipeline computes the scan's normals itself when it has none
    bare = RegistrationPipeline(scan=scan, scan_normals=None, ref=ref, ref_normals=nref)
    tf = bare.run_icp("symmetric", RigidTransform(), d_max=0.15, voxel_size=0.01, max_iter=40, rms_threshold=0.0, gicp_neighbors=15)[0]
    assert G.rotation_error(tf.rotation, r0) < 5e-3


def test_script_runs_symmetric_icp_end_to_end(eng, tmp_path):
    """scripts/register_point_clouds.py --icp symmetric on the config-4-shaped pair (6 000 points and their rigidly moved, permuted
    copy), in a process of its own: the refined alignment is written, lies within the RANSAC threshold of the generating motion and
    is no worse than the RANSAC start it was given."""
    from shot_fpfh_amd.helpers import read_ply, write_ply

    g = load_golden("c4_pair_6k.npz")
    inverse = np.empty(6000, np.int64)
    inverse[g["perm"]] = np.arange(6000)
    truth = g["ref"][inverse]  # where every scan point belongs: its own copy in the reference
    scan_file, ref_file = str(tmp_path / "scan.ply"), str(tmp_path / "ref.ply")
    write_ply(scan_file, [g["scan"]], ["x", "y", "z"])
    write_ply(ref_file, [g["ref"], g["ref_normals"]], ["x", "y", "z", "nx", "ny", "nz"])
    out = str(tmp_path / "aligned")
    r = run_program([sys.executable, os.path.join(ROOT, "scripts", "register_point_clouds.py"), scan_file, ref_file, "--radius",
                     repr(float(g["radius"])), "--keypoints", "subsampling", "--keypoint-size", "0.1", "--min-neighborhood-size", "10",
                     "--ransac-draws", "2000", "--ransac-threshold", "0.02", "--icp", "symmetric", "--icp-dmax", "0.05", "--icp-voxel", "0.04",
                     "--icp-rms", "1e-9", "--metric-threshold", "0.01", "--write", out], timeout=300)
    assert r["rc"] == 0, r["stderr"][-2000:]
    err = {}
    for stage in ("ransac", "icp"):
        merged = read_ply(f"{out}_{stage}.ply")
        assert merged.shape[0] == 12000
        err[stage] = float(np.abs(np.vstack((merged["x"], merged["y"], merged["z"])).T[:6000] - truth).max())
    print(f"max |aligned - truth|: RANSAC {err['ransac']:.2e}, symmetric ICP {err['icp']:.2e}")
    assert err["icp"] <= 0.02 and err["icp"] <= err["ransac"]
