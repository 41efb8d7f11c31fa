"""Point-to-point and point-to-plane ICP on the MI355X (k_icp_sums<1, 0>, k_icp_sums<1, 1>, k_transform; sf_icp_accumulate,
sf_transform_points, csrc/icp.hip) against the NumPy statement of one pass (tests/icp_numpy.py).

As for K16 (tests/test_hip_gicp.py), the check is split where rounding is left to the implementation.  ONE pass is held to the
math.fsum value of each of its 40 numbers within C k 2^-53 sum|term| with an equal pair count, the slots of no pass to exactly 0.0
and the `d_max` decision to the bit; the whole run is held to ten times the statement's own sensitivity to the order of its sums,
measured on the NumPy statement alone, with an exact iteration count and convergence flag.

The input sets and the `measure_*` functions are plain functions: tests/test_icp_host.py asserts every condition the tests below
place on their inputs without a device, and tools/icp_sums_parity.py writes profiles/icp_sums_parity.md from the same calls."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import cKDTree

import gicp_numpy as G
import icp_numpy as I
from conftest import config1_cloud
from test_hip_gicp import assert_unambiguous, one_pass_set

pytestmark = pytest.mark.gpu

U = 2.0**-53
D_MAX = 0.05
M_SIZES = [1, 63, 64, 65, 257, 65537]
# Roundings that enter one term as k_icp_sums forms it from the loaded coordinates, for the longest chain of each mode.  A moved
# coordinate p = ((R0 x + R1 y) + R2 z) + t carries 6; a reference coordinate and a normal component are loaded, 0.
#   mode 0: d2 = (dx dx + dy dy) + dz dz with d = q - p: three differences of 6 + 1 (21), three products (3), two additions (2): 26.
#           (a_i b_j = (p_i - pm_i)(q_j - qm_j) is shorter: 6 + 1, 1, and the product: 9; pass A's p: 6.)
#   mode 1: g_a h with g_a a component of p x n and h = (dx nx + dy ny) + dz nz: g_a = py nz - pz ny, two moved coordinates (12),
#           two products (2), the difference (1): 15; h: three differences of 7 (21), three products (3), two additions (2): 26;
#           the product (1): 42.  (g_a g_b: 15 + 15 + 1 = 31; |h|: 26.)
# The NumPy statement forms every term by the same operations in the same order (and mode 0 with the centroids the device itself
# formed), so what really differs is the order of the k additions: k - 1 roundings, each relative to a partial sum of magnitude
# <= sum|term|.  C k 2^-53 sum|term| covers both with room to spare -- the same form of bound as K16's C_ROUNDINGS = 114.
C_ROUNDINGS = {I.POINT: 26, I.PLANE: 42}
WORST = {}  # label -> worst observed |sum - fsum| / (k 2^-53 sum|term|), for the printout and the parity table
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


# ---- the input sets (also asserted on the CPU: tests/test_icp_host.py) -------------------------------------------------------------
def selection_ids():
    """777 rows out of 5 000, some of them more than once"""
    return np.random.default_rng(5).integers(0, 5000, 777)


def far_set(offset=1000.0, n=5000):
    """The one-pass reference moved by `offset` on every axis, and a scan around it twice: `plain` lies on it as it is (no
    transform), `scan` is carried onto it by the true motion."""
    if ("far", offset) not in _cache:
        s = one_pass_set()
        rng = np.random.default_rng(1000)
        ref = s["ref"] + offset
        world = ref[rng.integers(0, 2000, n)] + 0.03 * rng.standard_normal((n, 3))
        r0, t0 = G.true_motion()
        _cache[("far", offset)] = dict(ref=ref, nref=s["nref"], plain=world, scan=(world - t0) @ r0, tree=cKDTree(ref),
                                       states=[("no transform", "plain", None, None), ("true", "scan", r0, t0)])
    return _cache[("far", offset)]


LATTICE_STEP, LATTICE_R = 2.0**-3, 5 * 2.0**-7


def lattice_set():
    """An 8 x 8 x 8 lattice of spacing 2^-3; `off` = every lattice point + (3, 4, 0) 2^-7, so d2 = 25 2^-14 and its square root
    5 2^-7 are exact; `mixed` = the same with every fifth row ON its lattice point (d2 = 0)."""
    g = np.arange(8) * LATTICE_STEP
    ref = np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    off = ref + np.array([3.0, 4.0, 0.0]) * 2.0**-7
    mixed = off.copy()
    mixed[::5] = ref[::5]
    nref = _unit(np.random.default_rng(8).standard_normal((512, 3)))
    return dict(ref=ref, nref=nref, off=off, mixed=mixed, on_lattice=len(range(0, 512, 5)), tree=cKDTree(ref))


def sqrt_cases(count=16, n=5000):
    """(scan rows, d_max values): the distances of 16 pairs of the random set at the true motion, spread over their range;
    d_max = np.sqrt(d2_i) keeps pair i, the next double below it does not."""
    s = one_pass_set()
    label, R, t = s["states"][1]
    a = s["scan"][:n]
    d2 = G.nearest(G.move(R, t, a), s["ref"], s["tree"])[1]
    order = np.argsort(d2)
    picks = order[np.linspace(10, n - 10, count).astype(int)]
    return a, R, t, np.sqrt(d2[picks])


def changed_normals():
    """Reference normals after the first call: new directions, every 9th row zero, every 7th row of length 0.25 .. 4."""
    s = one_pass_set()
    rng = np.random.default_rng(77)
    new = _unit(rng.standard_normal((2000, 3)))
    new[::7] *= rng.uniform(0.25, 4.0, (len(range(0, 2000, 7)), 1))
    new[::9] = 0.0
    return new


SURFACE_ROWS, SURFACE_FAR = 5000, 200  # >= 2 * SF_K2_SAMPLE = 4096 queries: sf_knn_search counts a sample and may shrink its radius


def surface_set():
    """A reference ON a surface (20 000 points of the noisy sphere of conftest.config1_cloud, stored normals) and a scan of
    5 000 rows: 4 800 near the surface, 200 at 3 to 5 bounding-box diagonals from its centre, in random rows.  The first grid's
    radius comes from the bounding box's mean density and shrinks on the sample count; the far rows then double it round by
    round, every round on a rebuilt, coarser grid."""
    if "surface" not in _cache:
        ref, nref = config1_cloud(20000, 31)
        rng = np.random.default_rng(32)
        near = ref[rng.integers(0, 20000, SURFACE_ROWS - SURFACE_FAR)] + 0.004 * rng.standard_normal((SURFACE_ROWS - SURFACE_FAR, 3))
        diag = float(np.linalg.norm(ref.max(axis=0) - ref.min(axis=0)))
        far = 0.5 + _unit(rng.standard_normal((SURFACE_FAR, 3))) * rng.uniform(3.0, 5.0, (SURFACE_FAR, 1)) * diag
        scan = np.vstack([near, far])[rng.permutation(SURFACE_ROWS)]
        _cache["surface"] = dict(ref=ref, nref=nref, scan=scan, diag=diag, tree=cKDTree(ref))
    return _cache["surface"]


def corner_run_set():
    if "corner" not in _cache:
        scan, ref, r0, t0 = G.corner_set(0)
        _cache["corner"] = (scan, ref, G.knn_normals(ref), r0, t0)
    return _cache["corner"]


# Seed 0 of the K16 corner set from the identity, d_max = 0.15.  Neither mode's residual ever falls a hundredfold from one
# iteration to the next (point-to-point: 2.8, 1.4, 1.07, 0.96, ... -> 0.806; point-to-plane: 5.4e-2, 5.6e-3, 2.8e-3, 2.7e-3 ...:
# the noise floor; test_icp_host.py asserts it), so no rms_threshold puts the last rms 10 x below and the one before 10 x above:
# the run held to the sensitivity bound has a FIXED iteration count and rms_threshold = 0.  The rms stop itself is run as well, at
# the geometric mean of two consecutive residuals that are at least 5 % apart, where rounding (1e-15) decides nothing.
RUN_D_MAX = 0.15
RUN_ITERATIONS = {I.POINT: 30, I.PLANE: 10}
STOP_AFTER = {I.POINT: 4, I.PLANE: 3}  # the rms threshold lies between the residuals of iterations STOP_AFTER - 1 and STOP_AFTER


def stop_threshold(trace, mode):
    k = STOP_AFTER[mode]
    return float(np.sqrt(trace[k - 2] * trace[k - 1]))


# ---- the device side -----------------------------------------------------------------------------------------------------------------
class _Resident:
    """Scan and reference resident on the device; `sums` is one sf_icp_accumulate call, as `_Registration.pairs` makes it."""

    def __init__(self, eng, scan, ref, nref=None):
        from shot_fpfh_amd.icp import _Registration

        self.reg = _Registration(scan, ref, nref, engine=eng)

    def sums(self, mode, R, t, d_max, rows=None):
        from shot_fpfh_amd.core import RigidTransform

        by = None if R is None else RigidTransform(R, t)
        return self.reg.pairs(mode, d_max, moved_by=by, rows=rows).raw

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.reg.close()


def check_sums(got, a, ref, nref, R, t, d_max, mode, label, tree=None):
    """`got` (40 doubles of the device) against the statement centred with the device's own centroids.  Returns the worst ratio."""
    assert got.shape == (40,)
    want = I.sums(a, ref, nref, R, t, d_max, mode, means=I.device_means(got), tree=tree)
    k, c = want["count"], C_ROUNDINGS[mode]
    assert got[0] == k, (label, got[0], k)
    err = np.abs(got - want["vec"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want["abs"] > 0, err / (k * U * want["abs"]), 0.0))) if k else 0.0
    WORST[label] = worst
    print(f"{label}: k = {k}, worst |sum - fsum| = {worst:.3g} x k 2^-53 sum|term| (bound {c})")
    assert np.all(err <= c * k * U * want["abs"]), (label, np.flatnonzero(err > c * k * U * want["abs"]), worst)
    assert np.all(got[want["abs"] == 0] == 0)
    assert not got[I.UNUSED[mode]].any(), (label, got[I.UNUSED[mode]])  # the slots of no pass: exactly 0.0
    return worst


def measure_one_pass(eng, mode, m):
    """worst ratio over the three states at m scan rows; two calls bit for bit"""
    s = one_pass_set()
    a = s["scan"][:m]
    worst = 0.0
    with _Resident(eng, a, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            assert_unambiguous(s, a, R, t, D_MAX, (m, label))
            got = dev.sums(mode, R, t, D_MAX)
            assert np.array_equal(got, dev.sums(mode, R, t, D_MAX))
            worst = max(worst, check_sums(got, a, s["ref"], s["nref"], R, t, D_MAX, mode, f"mode {mode} m={m} {label}", s["tree"]))
    return worst


def measure_far(eng):
    """mode 0 with both clouds 1000 from the origin on every axis; the magnitudes are those of the CENTRED factors"""
    f = far_set()
    worst = 0.0
    for label, which, R, t in f["states"]:
        a = f[which]
        assert_unambiguous(f, a, R, t, D_MAX, ("far", label))
        with _Resident(eng, a, f["ref"]) as dev:
            got = dev.sums(I.POINT, R, t, D_MAX)
        assert got[0] > 0.5 * a.shape[0]  # most pairs are kept: the bound is about something
        worst = max(worst, check_sums(got, a, f["ref"], None, R, t, D_MAX, I.POINT, f"mode 0, +1000, {label}", f["tree"]))
    return worst


def _diff(r1, t1, r2, t2):
    return max(float(np.abs(r1 - r2).max()), float(np.abs(t1 - t2).max()))


def measure_whole_run(eng, mode):
    """dict(device_vs_statement, own, iterations, rms_device, rms_statement): `_refine` from the identity for a fixed number of
    iterations against the fsum statement; `own` = the statement's fsum run against four runs on row-permuted scans with
    NumPy's pairwise sums, the largest difference of R and t."""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import _refine

    scan, ref, nref, r0, t0 = corner_run_set()
    n_it = RUN_ITERATIONS[mode]
    exact = I.refine(scan, ref, nref, mode, RUN_D_MAX, max_iter=n_it, rms_threshold=0.0)
    own = 0.0
    for seed in range(4):
        order = np.random.default_rng(17 + seed).permutation(scan.shape[0])
        other = I.refine(scan[order], ref, nref, mode, RUN_D_MAX, max_iter=n_it, rms_threshold=0.0, how="np")
        own = max(own, _diff(exact["R"], exact["t"], other["R"], other["t"]))
    calls = []
    with _Resident(eng, scan, ref, nref) as dev:
        real = dev.reg.pairs
        dev.reg.pairs = lambda *a, **kw: calls.append(1) or real(*a, **kw)
        tf, rms, converged = _refine(dev.reg, RigidTransform(), mode, RUN_D_MAX, n_it, 0.0)
        fixed = len(calls)
        # the rms stop, where two consecutive residuals of the statement are far apart
        thr = stop_threshold(exact["rms_trace"], mode)
        stopped = I.refine(scan, ref, nref, mode, RUN_D_MAX, max_iter=n_it, rms_threshold=thr)
        del calls[:]
        tf2, rms2, converged2 = _refine(dev.reg, RigidTransform(), mode, RUN_D_MAX, n_it, thr)
    return dict(device_vs_statement=_diff(tf.rotation, tf.translation, exact["R"], exact["t"]), own=own, iterations=fixed,
                want_iterations=exact["iterations"], converged=bool(converged), rms_device=rms, rms_statement=exact["rms"],
                rotation_error=G.rotation_error(tf.rotation, r0), stop_iterations=len(calls), stop_want=stopped["iterations"],
                stop_converged=bool(converged2), stop_want_converged=bool(stopped["converged"]), stop_rms_device=rms2,
                stop_rms_statement=stopped["rms"], stop_threshold=thr)


# ---- a. one pass equals fsum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", M_SIZES)
@pytest.mark.parametrize("mode", [I.POINT, I.PLANE])
def test_one_pass_equals_fsum_within_the_rounding_bound(eng, mode, m):
    """m = 1: a single pair; 63, 64, 65: below, at and above a wave; 257: one block plus one; 65 537: one past the grid's
    256 x 256 threads, the stride loop wraps.  Identity, true motion and 0.3 rad away; counts equal, every slot within the bound,
    two calls bit for bit, the slots of no pass exactly 0.0."""
    worst = measure_one_pass(eng, mode, m)
    print(f"mode {mode}, m = {m}: worst ratio {worst:.3g} of {C_ROUNDINGS[mode]}")


# ---- b. far from the origin ----------------------------------------------------------------------------------------------------------
def test_point_to_point_is_centred_far_from_the_origin(eng):
    """Both clouds + 1000 per axis.  The bound's magnitudes are |a_i b_j| of the centred factors (~0.1), a million times below the
    uncentred |p_i q_j|: a kernel that accumulated uncentred products and subtracted k pbar qbar^T would miss it by ~1e4 x."""
    worst = measure_far(eng)
    print(f"mode 0, +1000: worst ratio {worst:.3g} of {C_ROUNDINGS[I.POINT]}")


# ---- c. selection and transform ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [I.POINT, I.PLANE])
def test_selection_and_transform_combinations(eng, mode):
    s = one_pass_set()
    a, ids = s["scan"][:5000], selection_ids()
    assert np.unique(ids).size < 777
    label, R, t = s["states"][1]
    with _Resident(eng, a, s["ref"], s["nref"]) as dev:
        for rows, pts in ((ids, a[ids]), (None, a)):
            for R2, t2 in ((R, t), (None, None)):
                assert_unambiguous(s, pts, R2, t2, D_MAX, "selection")
                got = dev.sums(mode, R2, t2, D_MAX, rows=rows)
                assert np.array_equal(got, dev.sums(mode, R2, t2, D_MAX, rows=rows))
                check_sums(got, pts, s["ref"], s["nref"], R2, t2, D_MAX, mode,
                           f"mode {mode} {'selection' if rows is not None else 'all rows'} {'moved' if R2 is not None else 'as is'}", s["tree"])
        # an empty selection: zeros, and no device work
        assert not dev.sums(mode, R, t, D_MAX, rows=np.zeros(0, dtype=np.int64)).any()


@pytest.mark.parametrize("mode", [I.POINT, I.PLANE])
def test_moving_the_points_equals_passing_the_transform(eng, mode):
    """`move(T)` then `pairs(moved_by=None)` performs the operations of `pairs(moved_by=T)` on the unmoved points: the same numbers."""
    from shot_fpfh_amd.core import RigidTransform

    s = one_pass_set()
    a = s["scan"][:5000]
    label, R, t = s["states"][1]
    with _Resident(eng, a, s["ref"], s["nref"]) as dev:
        want = dev.sums(mode, R, t, D_MAX)
        dev.reg.move(RigidTransform(R, t))
        got = dev.sums(mode, None, None, D_MAX)
        assert np.array_equal(dev.reg.download(), G.move(R, t, a))
    assert want[0] > 2500 and np.array_equal(got, want)


# ---- d. the d_max decision -----------------------------------------------------------------------------------------------------------
def test_d_max_decision_on_the_exact_lattice(eng):
    """sqrt(d2) = 5 2^-7 exactly: kept at d_max = 5 2^-7 (`<=`), dropped at the next double below; d_max = 0 keeps exactly the
    coincident points.  Without a transform and with the identity as an explicit one (x 1 + y 0 + z 0 + 0 is exact)."""
    L = lattice_set()
    below = float(np.nextafter(LATTICE_R, 0.0))
    eye, zero = np.eye(3), np.zeros(3)
    for name, on in (("off", 0), ("mixed", L["on_lattice"])):
        with _Resident(eng, L[name], L["ref"], L["nref"]) as dev:
            for mode in (I.POINT, I.PLANE):
                for R, t in ((None, None), (eye, zero)):
                    for d_max, want in ((LATTICE_R, 512), (below, on), (0.0, on)):
                        got = dev.sums(mode, R, t, d_max)
                        assert got[0] == want, (name, mode, R is None, d_max, got[0], want)
                        check_sums(got, L[name], L["ref"], L["nref"], R, t, d_max, mode, f"lattice {name} mode {mode} d_max={d_max!r}", L["tree"])
                        if want == 0:
                            assert not got.any()


def test_d_max_decision_follows_the_correctly_rounded_square_root(eng):
    """d_max = np.sqrt(d2_i) of 16 pairs: the count equals the statement's there and at the next double below, where pair i (and
    whatever shares its distance) is gone.  d2 is the same number on both sides; this holds the device's sqrt to NumPy's."""
    s = one_pass_set()
    a, R, t, radii = sqrt_cases()
    assert_unambiguous(s, a, R, t, np.inf, "sqrt cases")
    with _Resident(eng, a, s["ref"]) as dev:
        for r in radii:
            want = [I.kept_pairs(a, s["ref"], R, t, d_max, s["tree"])[0].shape[0] for d_max in (float(r), float(np.nextafter(r, 0.0)))]
            got = [dev.sums(I.POINT, R, t, d_max)[0] for d_max in (float(r), float(np.nextafter(r, 0.0)))]
            assert got == want and want[0] - want[1] == 1, (r, got, want)


@pytest.mark.parametrize("mode", [I.POINT, I.PLANE])
def test_d_max_edge_values(eng, mode):
    s = one_pass_set()
    a = s["scan"][:5000]
    label, R, t = s["states"][1]
    with _Resident(eng, a, s["ref"], s["nref"]) as dev:
        assert_unambiguous(s, a, R, t, np.inf, "inf")
        got = dev.sums(mode, R, t, np.inf)
        assert got[0] == 5000
        check_sums(got, a, s["ref"], s["nref"], R, t, np.inf, mode, f"mode {mode} d_max = inf", s["tree"])
        for d_max in (float("nan"), -1.0):
            got = dev.sums(mode, R, t, d_max)
            assert got.shape == (40,) and not got.any() and not np.isnan(got).any(), d_max


# ---- e. no pair at all ---------------------------------------------------------------------------------------------------------------
NO_PAIR_RADIUS = 1e-7


def test_no_pair_at_all(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import (compute_point_to_point_error, icp_point_to_plane, icp_point_to_point, nearest_within)

    s = one_pass_set()
    a = s["scan"][:5000]
    label, R, t = s["states"][1]
    assert I.kept_pairs(a, s["ref"], R, t, NO_PAIR_RADIUS, s["tree"])[0].shape[0] == 0
    with _Resident(eng, a, s["ref"], s["nref"]) as dev:
        for mode in (I.POINT, I.PLANE):
            got = dev.sums(mode, R, t, NO_PAIR_RADIUS)
            assert got.shape == (40,) and not got.any()
    moved = G.move(R, t, a)
    assert nearest_within(moved, s["ref"], NO_PAIR_RADIUS) == 0
    assert nearest_within(moved, s["ref"], D_MAX) == I.kept_pairs(a, s["ref"], R, t, D_MAX, s["tree"])[0].shape[0] > 2500
    start = RigidTransform(R, t)
    with pytest.raises(np.linalg.LinAlgError):
        icp_point_to_point(a, s["ref"], start, d_max=NO_PAIR_RADIUS, voxel_size=0.05, max_iter=3)
    with pytest.raises(np.linalg.LinAlgError):
        icp_point_to_plane(a, s["ref"], s["nref"], start, d_max=NO_PAIR_RADIUS, voxel_size=0.05, max_iter=3)
    # no d_max there: every point counts, whatever its distance (at the identity most are beyond 0.05)
    for tf in (RigidTransform(), start):
        err, out = compute_point_to_point_error(a, s["ref"], tf)
        d = s["tree"].query(tf[a], k=1)[0]
        assert np.isclose(err, np.sqrt(np.sum(d * d) / 5000), rtol=1e-12, atol=0.0), (err, np.sqrt(np.sum(d * d) / 5000))
        assert np.array_equal(out, tf[a])


# ---- f. normals that change under the cloud ------------------------------------------------------------------------------------------
def test_normals_replaced_after_the_first_call(eng):
    """The cell-sorted copy of the normals must follow `set_normals`; zero rows and rows of length 0.25 .. 4 are used as they are."""
    s = one_pass_set()
    a, new = s["scan"][:5000], changed_normals()
    label, R, t = s["states"][1]
    with _Resident(eng, a, s["ref"], s["nref"]) as dev:
        first = dev.sums(I.PLANE, R, t, D_MAX)
        check_sums(first, a, s["ref"], s["nref"], R, t, D_MAX, I.PLANE, "mode 1, first normals", s["tree"])
        dev.reg.ref.set_normals(new)
        got = dev.sums(I.PLANE, R, t, D_MAX)
        check_sums(got, a, s["ref"], new, R, t, D_MAX, I.PLANE, "mode 1, replaced normals (zero and non-unit rows)", s["tree"])
        assert np.array_equal(got[:7], first[:7]) and not np.array_equal(got[8:36], first[8:36])
        # point-to-point does not read them
        check_sums(dev.sums(I.POINT, R, t, D_MAX), a, s["ref"], None, R, t, D_MAX, I.POINT, "mode 0 after set_normals", s["tree"])


# ---- g. a grid that is rebuilt inside the call ---------------------------------------------------------------------------------------
def test_reference_on_a_surface_with_scan_points_far_outside(eng):
    """Neighbour positions, the point records and the sorted normals must all belong to the FINAL grid of the search."""
    f = surface_set()
    assert f["scan"].shape[0] == SURFACE_ROWS >= 4096
    assert_unambiguous(f, f["scan"], None, None, np.inf, "surface")
    with _Resident(eng, f["scan"], f["ref"], f["nref"]) as dev:
        eng.sync(); eng.profile_reset(); eng.profile(True)
        got = dev.sums(I.PLANE, None, None, np.inf)
        eng.sync(); eng.profile(False)
        rounds = eng.profile_report().get("k2_knn", (0, 0.0))[0]
        print(f"surface: {rounds} search rounds")
        # the far rows are 3 to 5 diagonals out and the first radius holds ~7 points of 20 000: the radius doubles many times,
        # and every doubling is a round on a rebuilt grid
        assert rounds >= 5
        assert got[0] == SURFACE_ROWS
        check_sums(got, f["scan"], f["ref"], f["nref"], None, None, np.inf, I.PLANE, "mode 1, surface + 200 far rows", f["tree"])
        assert np.array_equal(got, dev.sums(I.PLANE, None, None, np.inf))
        check_sums(dev.sums(I.POINT, None, None, np.inf), f["scan"], f["ref"], None, None, None, np.inf, I.POINT,
                   "mode 0, surface + 200 far rows", f["tree"])


# ---- h. sf_transform_points alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70000])
def test_transform_points_in_place(eng, n):
    from shot_fpfh_amd import _ffi

    rng = np.random.default_rng(300 + n)
    pts = rng.standard_normal((max(n, 1), 3))
    R, t = G.true_motion()
    rt = np.ascontiguousarray(np.concatenate([R.reshape(9), t]))
    dev = eng.empty(pts.shape).from_host(pts)
    try:
        _ffi.check(eng.lib.sf_transform_points(eng.h, dev.ptr, n, rt.ctypes.data_as(C.c_void_p)), "sf_transform_points")
        got = dev.to_host()
    finally:
        dev.free()
    assert np.array_equal(got[:n], G.move(R, t, pts[:n]))
    assert np.array_equal(got[n:], pts[n:])  # n = 0: nothing is touched


# ---- i. whole runs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [I.POINT, I.PLANE])
def test_whole_run_agrees_with_the_statement(eng, mode):
    """Seed 0 of the K16 corner set from the identity (see RUN_ITERATIONS for why the count is fixed).  Iteration count and flag
    exact, rms to 1e-9 relative, max(|dR|, |dt|) within ten times the statement's own sensitivity to the order of its sums."""
    r = measure_whole_run(eng, mode)
    print(f"mode {mode}: device vs fsum statement {r['device_vs_statement']:.3e} after {r['iterations']} iterations; the statement's "
          f"own fsum vs permuted np.sum {r['own']:.3e}; bound 10 x that; |R - R0| = {r['rotation_error']:.2e}; rms "
          f"{r['rms_device']:.12e} vs {r['rms_statement']:.12e}; rms stop at {r['stop_threshold']:.3e}: {r['stop_iterations']} "
          f"iterations (statement {r['stop_want']})")
    assert (r["iterations"], r["converged"]) == (r["want_iterations"], False) and r["want_iterations"] == RUN_ITERATIONS[mode]
    assert np.isclose(r["rms_device"], r["rms_statement"], rtol=1e-9, atol=0.0)
    assert (r["stop_iterations"], r["stop_converged"]) == (r["stop_want"], True) and r["stop_want"] == STOP_AFTER[mode]
    assert r["stop_want_converged"] and np.isclose(r["stop_rms_device"], r["stop_rms_statement"], rtol=1e-9, atol=0.0)
    assert r["device_vs_statement"] <= 10 * r["own"], (r["device_vs_statement"], r["own"])
