"""ICP with a robust loss on the MI355X (K17: k_icp_sums, k_icp_means, sf_icp_accumulate_robust, csrc/icp.hip;
shot_fpfh_amd.icp.icp_robust) against the NumPy statement (tests/icp_robust_numpy.py).

The check is split as for its siblings (tests/test_hip_icp_sums.py, tests/test_hip_gicp.py).  ONE pass is held to the math.fsum value
of each of its 48 numbers within C k 2^-53 sum|term| with an equal pair count, the slots of no pass to exactly 0.0; with loss none
(and with Huber above every residual) the call is held to the plain entry points bit for bit, and those to the numbers recorded in
tests/golden/icp_plain_sums.npz; the whole run is held to ten times the statement's own sensitivity to the order of its sums, with
an exact iteration count and convergence flag.

The input sets and the `measure_*` functions are plain functions: tests/test_icp_robust_host.py asserts the conditions the tests
below place on their inputs without a device, and tools/icp_robust_parity.py writes profiles/icp_robust_parity.md from the same
calls."""
import ctypes as C
import math

import numpy as np
import pytest

import gicp_numpy as G
import icp_numpy as I
import icp_robust_numpy as S
import test_hip_icp_sums as T
from test_hip_gicp import assert_unambiguous, one_pass_set

pytestmark = pytest.mark.gpu

U = 2.0**-53
D_MAX = T.D_MAX
M_SIZES = T.M_SIZES
MODE_IDS = [S.POINT, S.PLANE, S.GICP]
LOSS_IDS = list(S.LOSSES.values())
EPS = 1e-3
# The scale of the one-pass tests.  At the true motion the distances of the random set spread up to d_max = 0.05 (0.03 of noise per
# axis): at k = 0.02 Huber takes both branches, Tukey cuts a part of the pairs off and the other two weights spread over (0.1, 1).
# Mode 2 measures the Mahalanobis distance; the set's normals are random directions, not those of a surface, so M's eigenvalues are
# of order one and sqrt(r2) spreads like the distance with a tail (median 0.03, one pair in ten beyond 0.065): k = 0.03 there.
# tests/test_icp_robust_host.py asserts that every loss really weights at these scales.
K_ONE = {S.POINT: 0.02, S.PLANE: 0.02, S.GICP: 0.03}
# Roundings that enter one term, for the longest chain of each mode, counted as the existing tests count them (every rounding of
# the expression's tree from the loaded coordinates), i.e. their count plus the weight's roundings.  The weight adds, from r2:
# Huber 2 (sqrt, k / a), Cauchy 4 (k k, r2 / kk, 1 + s, 1 / .), Tukey 4 (k k, r2 / kk, 1 - s, o o), Geman-McClure 5 (Cauchy's and
# c c): at most 5.  The longest chain is the new slot [46], w r2, into which r2 enters twice, through w and as the factor:
#   mode 0: r2 = d2, 26 (tests/test_hip_icp_sums.py): w 26 + 5 = 31, w r2 = 31 + 26 + 1 = 58.
#           (a weighted fit term w (a_i b_j): 31 + 9 + 1 = 41.)
#   mode 1: h carries 26, r2 = h h: 26 + 26 + 1 = 53, w 58, w r2 = 58 + 53 + 1 = 112.
#           (a weighted fit term w (g_a h): 58 + 42 + 1 = 101, with 42 the count of tests/test_hip_icp_sums.py.)
#   mode 2: r2 = the Mahalanobis term, 114 (tests/test_hip_gicp.py; the clamp is exact): w 119, w r2 = 119 + 114 + 1 = 234.
# The NumPy statement forms every term by the same operations in the same order (and mode 0 with the weighted centroids the device
# itself formed), so what really differs is the order of the k additions: k - 1 roundings, each relative to a partial sum of
# magnitude <= sum|term|.  C k 2^-53 sum|term| covers both with room to spare, the form of bound of the two sibling files.
C_ROUNDINGS = {S.POINT: 58, S.PLANE: 112, S.GICP: 234}
WORST = {}  # label -> worst observed |sum - fsum| / (k 2^-53 sum|term|)
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


# ---- the device side -----------------------------------------------------------------------------------------------------------------
class _Resident:
    """Scan (with normals) and reference resident on the device; `sums` is one sf_icp_accumulate_robust call as
    `_Registration.pairs` makes it, `plain` the plain call of the same mode (sf_icp_accumulate, sf_icp_accumulate_gicp)."""

    def __init__(self, eng, scan, na, ref, nref=None):
        from shot_fpfh_amd.icp import _Registration

        self.reg = _Registration(scan, ref, nref, engine=eng, scan_normals=na)

    @staticmethod
    def _by(R, t):
        from shot_fpfh_amd.core import RigidTransform

        return None if R is None else RigidTransform(R, t)

    def sums(self, mode, loss, k, R, t, d_max, rows=None, eps=EPS):
        return self.reg.pairs(mode, d_max, moved_by=self._by(R, t), rows=rows, epsilon=eps, loss=loss, scale=k).raw

    def plain(self, mode, R, t, d_max, rows=None, eps=EPS):
        return self.reg.pairs(mode, d_max, moved_by=self._by(R, t), rows=rows, epsilon=eps).raw

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.reg.close()


def check_sums(got, mode, loss, k, a, na, ref, nref, R, t, d_max, label, eps=EPS, tree=None):
    """`got` (48 doubles of the device, or of a transcription) against the statement, mode 0 centred with the weighted centroids
    `got` itself implies.  Returns the worst ratio."""
    assert got.shape == (48,)
    want = S.sums(mode, loss, k, a, na, ref, nref, R, t, d_max, eps, means=S.device_means(got) if mode == S.POINT else None, tree=tree)
    n, c = want["count"], C_ROUNDINGS[mode]
    assert got[0] == n, (label, got[0], n)
    err = np.abs(got - want["vec"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want["abs"] > 0, err / (n * U * want["abs"]), 0.0))) if n else 0.0
    WORST[label] = worst
    print(f"{label}: pairs = {n}, sum w = {got[7]:.6g}, worst |sum - fsum| = {worst:.3g} x k 2^-53 sum|term| (bound {c})")
    assert np.all(err <= c * n * U * want["abs"]), (label, np.flatnonzero(err > c * n * U * want["abs"]), worst)
    assert np.all(got[want["abs"] == 0] == 0)
    assert not got[S.UNUSED[mode]].any(), (label, got[S.UNUSED[mode]])  # the slots of no pass: exactly 0.0
    return worst


def measure_one_pass(eng, mode, loss, m):
    """worst ratio over the three states at m scan rows; two calls bit for bit"""
    s = one_pass_set()
    a, na = s["scan"][:m], s["na"][:m]
    worst = 0.0
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            assert_unambiguous(s, a, R, t, D_MAX, (m, label))
            got = dev.sums(mode, loss, K_ONE[mode], R, t, D_MAX)
            assert np.array_equal(got, dev.sums(mode, loss, K_ONE[mode], R, t, D_MAX))
            worst = max(worst, check_sums(got, mode, loss, K_ONE[mode], a, na, s["ref"], s["nref"], R, t, D_MAX,
                                          f"mode {mode} loss {loss} m={m} {label}", tree=s["tree"]))
    return worst


def measure_far(eng, loss=S.LOSSES["cauchy"]):
    """mode 0 with both clouds 1000 from the origin on every axis; the magnitudes are those of the weighted CENTRED factors"""
    f = T.far_set()
    worst = 0.0
    for label, which, R, t in f["states"]:
        a = f[which]
        assert_unambiguous(f, a, R, t, D_MAX, ("far", label))
        with _Resident(eng, a, None, f["ref"]) as dev:
            got = dev.sums(S.POINT, loss, K_ONE[S.POINT], R, t, D_MAX)
        assert got[0] > 0.5 * a.shape[0] and 0.1 * got[0] < got[7] < 0.9 * got[0]  # most pairs kept, and really weighted
        worst = max(worst, check_sums(got, S.POINT, loss, K_ONE[S.POINT], a, None, f["ref"], None, R, t, D_MAX,
                                      f"mode 0 loss {loss}, +1000, {label}", tree=f["tree"]))
    return worst


# ---- whole runs ------------------------------------------------------------------------------------------------------------------------
RUN_ITERATIONS = 25  # the scale comes down from d_max = 0.15 to 0.006 in ten iterations (1.4^10 = 28.9); fifteen more at the scale
RUN_LOSSES = ["cauchy", "tukey"]
RUN_VOXEL = 1e-4     # keeps every point of the set (tests/test_icp_robust_host.py asserts it): the statement sees the same scan


def clutter_run_set():
    if "clutter" not in _cache:
        scan, ref, r0, t0 = S.clutter_set(0)
        _cache["clutter"] = (scan, G.knn_normals(scan), ref, G.knn_normals(ref), r0, t0)
    return _cache["clutter"]


def _diff(r1, t1, r2, t2):
    return max(float(np.abs(r1 - r2).max()), float(np.abs(t1 - t2).max()))


def _count_calls(monkeypatch):
    from shot_fpfh_amd.icp import _Registration

    calls, real = [], _Registration.pairs
    monkeypatch.setattr(_Registration, "pairs", lambda self, *a, **kw: calls.append(kw.get("scale")) or real(self, *a, **kw))
    return calls


def run_device(mode_name, loss_name, **kw):
    """`icp_robust` on the clutter set from the identity with the table's scales"""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_robust

    scan, na, ref, nref, r0, t0 = clutter_run_set()
    k, k0 = S.table_scales(mode_name, loss_name)
    args = dict(mode=mode_name, loss=loss_name, scale=k, scale_start=k0, division_factor=S.FACTOR, ref_normals=nref, scan_normals=na,
                epsilon=EPS, voxel_size=RUN_VOXEL, max_iter=RUN_ITERATIONS, rms_threshold=0.0, step_tolerance=0.0)
    args.update(kw)
    return icp_robust(scan, ref, RigidTransform(), S.D_MAX, **args)


def run_statement(mode_name, loss_name, how="fsum", order=None, **kw):
    scan, na, ref, nref, r0, t0 = clutter_run_set()
    if order is not None:
        scan, na = scan[order], na[order]
    k, k0 = S.table_scales(mode_name, loss_name)
    args = dict(max_iter=RUN_ITERATIONS, rms_threshold=0.0, step_tolerance=0.0)
    args.update(kw)
    return S.refine(scan, na, ref, nref, S.MODES[mode_name], S.LOSSES[loss_name], S.D_MAX, k, k0, S.FACTOR, eps=EPS, how=how, **args)


def measure_whole_run(mode_name, loss_name, calls):
    """dict(device_vs_statement, own, ...): `icp_robust` for a fixed number of iterations against the fsum statement; `own` = the
    statement's fsum run against four runs on row-permuted scans with NumPy's pairwise sums, the largest difference of R and t."""
    scan, na, ref, nref, r0, t0 = clutter_run_set()
    exact = run_statement(mode_name, loss_name)
    own = 0.0
    for seed in range(4):
        order = np.random.default_rng(17 + seed).permutation(scan.shape[0])
        other = run_statement(mode_name, loss_name, how="np", order=order)
        own = max(own, _diff(exact["R"], exact["t"], other["R"], other["t"]))
    del calls[:]
    tf, rms, converged = run_device(mode_name, loss_name)
    return dict(device_vs_statement=_diff(tf.rotation, tf.translation, exact["R"], exact["t"]), own=own, iterations=len(calls),
                scales=list(calls), want_scales=exact["scales"], want_iterations=exact["iterations"], converged=bool(converged),
                rms_device=rms, rms_statement=exact["rms"], rotation_error=G.rotation_error(tf.rotation, r0),
                rotation_error_statement=G.rotation_error(exact["R"], r0))


# ---- 1. one pass equals fsum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", M_SIZES)
@pytest.mark.parametrize("loss", LOSS_IDS)
@pytest.mark.parametrize("mode", MODE_IDS)
def test_one_pass_equals_fsum_within_the_rounding_bound(eng, mode, loss, m):
    """m = 1: a single pair; 63, 64, 65: below, at and above a wave; 257: one block plus one; 65 537: one past the grid's 256 x 256
    threads, the stride loop wraps.  Identity, true motion and 0.3 rad away; counts equal, each of the 48 numbers within the bound,
    two calls bit for bit, the slots of no pass exactly 0.0."""
    worst = measure_one_pass(eng, mode, loss, m)
    print(f"mode {mode}, loss {loss}, m = {m}: worst ratio {worst:.3g} of {C_ROUNDINGS[mode]}")


# ---- 2. loss none is the plain call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_IDS)
def test_loss_none_and_huber_above_every_residual_return_todays_numbers_bit_for_bit(eng, mode):
    s = one_pass_set()
    a, na, ids = s["scan"][:5000], s["na"][:5000], T.selection_ids()
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            for rows in (None, ids):
                today = dev.plain(mode, R, t, D_MAX, rows=rows)
                assert today.shape == (40,) and today[0] > 0
                for loss, k in ((S.LOSSES["none"], 1.0), (S.LOSSES["none"], 1e-6), (S.LOSSES["huber"], 1e6)):
                    got = dev.sums(mode, loss, k, R, t, D_MAX, rows=rows)
                    same = got[:40].copy()
                    same[7] = 0.0  # today's [7] belongs to no pass; here it is sum w = the count
                    assert np.array_equal(same, today) and today[7] == 0.0, (label, loss, np.flatnonzero(same != today))
                    assert got[7] == got[0] and np.array_equal(got[40:46], got[1:7]) and got[47] == 0.0
                    if mode == S.POINT:
                        assert got[46] == got[17]  # sum 1 * d2


# ---- 2b. the plain calls return the numbers recorded before the unweighted sums kernels were deleted ----------------------------------
PLAIN_GOLDEN = "icp_plain_sums.npz"  # written by tools/gen_golden_icp_plain.py, inputs included
PLAIN_GOLDEN_KEPT = ((134, 37), (397, 106), (120, 34))  # kept pairs per (state, all rows / selection)


def plain_golden_cases(g):
    """(state, rows index, R, t, rows) of the fixture's six cases; state 0 is the call without a transform"""
    for si in range(3):
        R, t = (None, None) if si == 0 else (g["rotations"][si], g["translations"][si])
        for ri, rows in enumerate((None, g["selection"])):
            yield si, ri, R, t, rows


def plain_golden_input_conditions(g):
    """What the golden test asks of its inputs, without a device: unit normals, three blocks of scan rows, a selection with repeats
    that ends inside a wave, no case whose kept set is a matter of rounding, and the kept counts -- from under a wave to several,
    never under 30.  Returns the counts per (state, rows)."""
    from scipy.spatial import cKDTree

    ref, scan, ids, d_max = g["ref"], g["scan"], g["selection"], float(g["d_max"])
    assert ref.shape == g["ref_normals"].shape == (500, 3) and scan.shape == g["scan_normals"].shape == (600, 3)
    assert ids.shape == (150,) and ids.min() >= 0 and ids.max() < 600 and np.unique(ids).size < 150 and 150 % 64
    assert 2 * 256 < scan.shape[0] <= 3 * 256
    for nrm in (g["ref_normals"], g["scan_normals"]):
        assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1.0) <= 8 * U)  # a handful of roundings: the division, the squares, their sum, the root
    assert np.array_equal(g["rotations"][0], np.eye(3)) and not g["translations"][0].any()
    assert d_max == 0.05 and float(g["epsilon"]) == 1e-3
    s = dict(tree=cKDTree(ref))
    kept = [[0, 0] for _ in range(3)]
    for si, ri, R, t, rows in plain_golden_cases(g):
        a = scan if rows is None else scan[rows]
        assert_unambiguous(s, a, R, t, d_max, ("golden", si, ri))
        kept[si][ri] = I.kept_pairs(a, ref, R, t, d_max, s["tree"])[0].shape[0]
    assert kept == [list(x) for x in PLAIN_GOLDEN_KEPT] and min(min(x) for x in kept) >= 30
    assert min(min(x) for x in kept) < 64 < 4 * 64 < max(max(x) for x in kept)
    return kept


def plain_golden_sums(eng, g, modes=MODE_IDS):
    """sums[mode, state, rows] of the plain entry points (sf_icp_accumulate, sf_icp_accumulate_gicp) on the fixture's inputs, from
    a `_Registration` of its own"""
    out = np.zeros((len(modes), 3, 2, 40))
    with _Resident(eng, g["scan"], g["scan_normals"], g["ref"], g["ref_normals"]) as dev:
        for mi, mode in enumerate(modes):
            for si, ri, R, t, rows in plain_golden_cases(g):
                out[mi, si, ri] = dev.plain(mode, R, t, float(g["d_max"]), rows=rows, eps=float(g["epsilon"]))
    return out


@pytest.mark.parametrize("mode", MODE_IDS)
def test_plain_calls_return_the_recorded_numbers_bit_for_bit(eng, mode):
    """tests/golden/icp_plain_sums.npz holds the 40 numbers of the plain calls as the MI355X returned them from the unweighted sums
    kernels the library had before the weighted family became its only one: 600 scan rows (three blocks) and a selection of 150
    (partial waves) against 500 reference points, three states.  Any change of an operation, of its order or of the order of the
    additions moves a bit here."""
    from conftest import load_golden

    g = load_golden(PLAIN_GOLDEN)
    got = plain_golden_sums(eng, g, [mode])[0]
    want = g["sums"][mode]
    assert got[..., 0].tolist() == [list(x) for x in PLAIN_GOLDEN_KEPT]
    assert np.array_equal(got, want), np.argwhere(got != want)


# ---- 3. weight edge cases on the exact lattice ---------------------------------------------------------------------------------------
def lattice_scales():
    r = T.LATTICE_R
    return [("exactly k", r), ("just below k", float(np.nextafter(r, np.inf))), ("just above k", float(np.nextafter(r, 0.0)))]


@pytest.mark.parametrize("loss", [S.LOSSES["huber"], S.LOSSES["tukey"]])
def test_weight_edges_on_the_exact_lattice(eng, loss):
    """Every pair of `off` has d2 = 25 2^-14 and sqrt(d2) = 5 2^-7 =: r exactly.  With k = r the residual is exactly k (Huber 1, Tukey
    0); with k the next double above r it is just below k, with the next below r just above.  All 512 pairs (one per thread) have
    the same weight, so every partial sum is w times a power of two or a sum of such: sum w is exact on both sides and must be
    EQUAL.  `mixed` adds pairs of residual 0 (w = 1) and is held to the bound."""
    L = T.lattice_set()
    for name in ("off", "mixed"):
        with _Resident(eng, L[name], None, L["ref"], L["nref"]) as dev:
            for label, k in lattice_scales():
                for R, t in ((None, None), (np.eye(3), np.zeros(3))):
                    got = dev.sums(S.POINT, loss, k, R, t, T.LATTICE_R)
                    assert got[0] == 512
                    check_sums(got, S.POINT, loss, k, L[name], None, L["ref"], L["nref"], R, t, T.LATTICE_R,
                               f"lattice {name} loss {loss} {label}", tree=L["tree"])
                    if name == "off":
                        w = float(S.weight(loss, np.array([25 * 2.0**-14]), k)[0])
                        assert got[7] == 512 * w, (label, got[7], w)
                        if label == "exactly k":
                            assert w == (1.0 if loss == S.LOSSES["huber"] else 0.0)
                        elif label == "just above k":
                            assert (0.0 < 1.0 - w < 1e-15) if loss == S.LOSSES["huber"] else w == 0.0
                        else:
                            assert w == 1.0 if loss == S.LOSSES["huber"] else 0.0 < w < 1e-30
                    else:
                        assert got[7] >= L["on_lattice"]  # the coincident pairs weigh 1


# ---- 4. far from the origin ------------------------------------------------------------------------------------------------------------
def test_weighted_point_to_point_is_centred_far_from_the_origin(eng):
    """Both clouds + 1000 per axis, Cauchy.  The bound's magnitudes are w |a_i b_j| of the factors centred with the WEIGHTED
    centroids (~0.1): centring with the unweighted ones, or not at all, leaves k (pbar_w - pbar)(..)^T or products of 1e6."""
    worst = measure_far(eng)
    print(f"mode 0, Cauchy, +1000: worst ratio {worst:.3g} of {C_ROUNDINGS[S.POINT]}")


# ---- 5. call variants ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_IDS)
def test_selection_and_transform_combinations(eng, mode):
    s = one_pass_set()
    a, na, ids = s["scan"][:5000], s["na"][:5000], T.selection_ids()
    label, R, t = s["states"][1]
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for loss in (S.LOSSES["geman_mcclure"], S.LOSSES["huber"]):
            for rows, pts, nrm in ((ids, a[ids], na[ids]), (None, a, na)):
                for R2, t2 in ((R, t), (None, None)):
                    assert_unambiguous(s, pts, R2, t2, D_MAX, "selection")
                    got = dev.sums(mode, loss, K_ONE[mode], R2, t2, D_MAX, rows=rows)
                    assert np.array_equal(got, dev.sums(mode, loss, K_ONE[mode], R2, t2, D_MAX, rows=rows))
                    check_sums(got, mode, loss, K_ONE[mode], pts, nrm, s["ref"], s["nref"], R2, t2, D_MAX,
                               f"mode {mode} loss {loss} {'selection' if rows is not None else 'all rows'} "
                               f"{'moved' if R2 is not None else 'as is'}", tree=s["tree"])
        # an empty selection: zeros, and no device work
        got = dev.sums(mode, S.LOSSES["cauchy"], K_ONE[mode], R, t, D_MAX, rows=np.zeros(0, dtype=np.int64))
        assert got.shape == (48,) and not got.any()


@pytest.mark.parametrize("mode", MODE_IDS)
def test_moving_the_points_equals_passing_the_transform(eng, mode):
    """`move(T)` then a call without a transform performs the operations of the call with T on the unmoved points: the same
    numbers.  Mode 2 also turns the scan's normals by R: there the moved points come with normals turned on the host by the same
    operations."""
    from shot_fpfh_amd.core import RigidTransform

    s = one_pass_set()
    a, na = s["scan"][:5000], s["na"][:5000]
    label, R, t = s["states"][1]
    loss, k = S.LOSSES["cauchy"], K_ONE[mode]
    turned = G.rotate(R, na)
    with _Resident(eng, a, turned if mode == S.GICP else na, s["ref"], s["nref"]) as dev:
        dev.reg.move(RigidTransform(R, t))
        got = dev.sums(mode, loss, k, None, None, D_MAX)
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        want = dev.sums(mode, loss, k, R, t, D_MAX)
    assert want[0] > 2500 and np.array_equal(got, want)


def test_no_pair_at_all_and_no_weight_at_all(eng):
    s = one_pass_set()
    a, na = s["scan"][:5000], s["na"][:5000]
    label, R, t = s["states"][1]
    assert I.kept_pairs(a, s["ref"], R, t, T.NO_PAIR_RADIUS, s["tree"])[0].shape[0] == 0
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for mode in MODE_IDS:
            for loss in LOSS_IDS:
                got = dev.sums(mode, loss, K_ONE[mode], R, t, T.NO_PAIR_RADIUS)
                assert got.shape == (48,) and not got.any()
            # Tukey with every pair beyond k: sum w = 0 and every weighted slot is zero, the unweighted ones are the statement's
            tiny = 1e-9
            got = dev.sums(mode, S.LOSSES["tukey"], tiny, R, t, D_MAX)
            tm, _mg = S.terms(mode, S.LOSSES["tukey"], tiny, a, na, s["ref"], s["nref"], R, t, D_MAX, EPS, np.zeros(6), s["tree"])
            assert tm.shape[0] > 2500 and not tm[:, 7].any()
            check_sums(got, mode, S.LOSSES["tukey"], tiny, a, na, s["ref"], s["nref"], R, t, D_MAX, f"mode {mode}: no weight", tree=s["tree"])
            assert got[0] == tm.shape[0] and got[7] == 0.0 and not got[S.WEIGHTED[mode]].any() and not got[40:48].any()
            today = dev.plain(mode, R, t, D_MAX)
            unweighted = {S.POINT: [17], S.PLANE: [35], S.GICP: [35, 36]}[mode]
            assert np.array_equal(got[:7], today[:7]) and np.array_equal(got[unweighted], today[unweighted])


def test_argument_errors_name_the_argument(eng):
    from shot_fpfh_amd import ShotFpfhError, _ffi

    s = one_pass_set()
    with _Resident(eng, s["scan"][:100], s["na"][:100], s["ref"], s["nref"]) as dev:
        for kw, word in ((dict(loss=5), "loss"), (dict(loss=-1), "loss"), (dict(k=0.0), "scale"), (dict(k=-1.0), "scale"),
                         (dict(k=float("nan")), "scale"), (dict(k=float("inf")), "scale"), (dict(mode=3), "mode"),
                         (dict(mode=S.GICP, eps=0.0), "epsilon"), (dict(mode=S.GICP, eps=float("nan")), "epsilon")):
            args = dict(mode=S.PLANE, loss=2, k=0.02, eps=EPS)
            args.update(kw)
            with pytest.raises(ShotFpfhError, match=word):
                dev.sums(args["mode"], args["loss"], args["k"], None, None, D_MAX, eps=args["eps"])
        reg, raw = dev.reg, np.zeros(48)
        rc = eng.lib.sf_icp_accumulate_robust(eng.h, reg.ref.h, reg.points.ptr, None, None, 100, None, D_MAX, S.GICP, EPS, 2, 0.5,
                                              raw.ctypes.data_as(C.c_void_p))
        assert rc != 0 and "nrm_dev" in _ffi.last_error()
        # epsilon and the normals are not looked at in modes 0 and 1
        assert dev.sums(S.POINT, 2, 0.02, None, None, D_MAX, eps=float("nan"))[0] > 0
    with _Resident(eng, s["scan"][:100], None, s["ref"], None) as dev:  # a reference without normals
        with pytest.raises(ShotFpfhError, match="normals"):
            dev.sums(S.PLANE, 2, 0.02, None, None, D_MAX)
        assert dev.sums(S.POINT, 2, 0.02, None, None, D_MAX)[0] > 0


# ---- 6. whole runs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_name", RUN_LOSSES)
@pytest.mark.parametrize("mode_name", list(S.MODES))
def test_whole_run_agrees_with_the_statement(eng, monkeypatch, mode_name, loss_name):
    """`clutter_set(0)` through `icp_robust` from the identity, a FIXED number of iterations (rms_threshold = 0, step_tolerance = 0)
    with the table's annealing.  Iteration count, the scale of every iteration and the flag exact, rms to 1e-9 relative,
    max(|dR|, |dt|) within ten times the statement's own sensitivity to the order of its sums."""
    r = measure_whole_run(mode_name, loss_name, _count_calls(monkeypatch))
    print(f"{mode_name} {loss_name}: device vs fsum statement {r['device_vs_statement']:.3e} after {r['iterations']} iterations; the "
          f"statement's own fsum vs permuted np.sum {r['own']:.3e}; bound 10 x that; |R - R0| = {r['rotation_error']:.2e} (statement "
          f"{r['rotation_error_statement']:.2e}); rms {r['rms_device']:.12e} vs {r['rms_statement']:.12e}")
    assert (r["iterations"], r["converged"]) == (r["want_iterations"], False) and r["want_iterations"] == RUN_ITERATIONS
    assert r["scales"] == r["want_scales"]
    assert np.isclose(r["rms_device"], r["rms_statement"], rtol=1e-9, atol=0.0)
    assert r["device_vs_statement"] <= 10 * r["own"], (r["device_vs_statement"], r["own"])


STOP_MODE, STOP_LOSS = "point_to_plane", "cauchy"
STEP_STOP_ITERATIONS = 60


def step_stop_tolerance(steps):
    """a tolerance the statement's steps cross far from rounding: the geometric mean of the first step below 1e-8 and the one
    before it (the run contracts by a factor of about three per iteration there; rounding moves a step by ~1e-16), and the
    iteration the run then stops at"""
    i = next(i for i in range(12, len(steps)) if steps[i] < 1e-8)
    assert steps[i - 1] >= 2 * steps[i] and min(steps[:i]) == steps[i - 1], steps
    return math.sqrt(steps[i] * steps[i - 1]), i + 1


def test_step_tolerance_stop(eng, monkeypatch):
    """The step stop, once: not before the scale has reached `scale`, although the steps of the first iterations would allow a
    larger tolerance, and then at the iteration the statement stops at."""
    calls = _count_calls(monkeypatch)
    free = run_statement(STOP_MODE, STOP_LOSS, max_iter=STEP_STOP_ITERATIONS)
    tol, at = step_stop_tolerance(free["steps"])
    want = run_statement(STOP_MODE, STOP_LOSS, max_iter=STEP_STOP_ITERATIONS, step_tolerance=tol)
    assert want["converged"] and want["iterations"] == at and want["scales"][-1] == S.table_scales(STOP_MODE, STOP_LOSS)[0]
    tf, rms, converged = run_device(STOP_MODE, STOP_LOSS, max_iter=STEP_STOP_ITERATIONS, step_tolerance=tol)
    print(f"step tolerance {tol:.3e}: {len(calls)} iterations (statement {want['iterations']}), steps {['%.1e' % x for x in free['steps'][:at + 1]]}")
    assert (len(calls), bool(converged)) == (want["iterations"], True)
    assert np.isclose(rms, want["rms"], rtol=1e-9, atol=0.0)
    # a tolerance above every step stops at the first iteration whose scale is `scale`, not at the first iteration
    del calls[:]
    tf, rms, converged = run_device(STOP_MODE, STOP_LOSS, max_iter=STEP_STOP_ITERATIONS, step_tolerance=10.0)
    first = next(i for i, k in enumerate(want["scales"]) if k == want["scales"][-1]) + 1
    assert (len(calls), bool(converged)) == (first, True) and first > 5


def rms_stop_threshold(trace):
    """the geometric mean of the first two consecutive residuals that are at least 5 % apart, and the iteration it stops"""
    for i in range(1, len(trace)):
        if trace[i] * 1.05 <= trace[i - 1]:
            return math.sqrt(trace[i] * trace[i - 1]), i + 1
    raise AssertionError("no two consecutive residuals 5 % apart")


def test_rms_stop(eng, monkeypatch):
    calls = _count_calls(monkeypatch)
    free = run_statement(STOP_MODE, STOP_LOSS)
    thr, at = rms_stop_threshold(free["rms_trace"])
    want = run_statement(STOP_MODE, STOP_LOSS, rms_threshold=thr)
    assert want["converged"] and want["iterations"] == at
    tf, rms, converged = run_device(STOP_MODE, STOP_LOSS, rms_threshold=thr)
    print(f"rms threshold {thr:.3e}: {len(calls)} iterations (statement {want['iterations']})")
    assert (len(calls), bool(converged)) == (want["iterations"], True) and rms < thr
    assert np.isclose(rms, want["rms"], rtol=1e-9, atol=0.0)


def test_all_weights_zero_raises_and_names_the_scale(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_robust

    scan, na, ref, nref, r0, t0 = clutter_run_set()
    with pytest.raises(np.linalg.LinAlgError, match="scale 1e-09"):
        icp_robust(scan, ref, RigidTransform(), S.D_MAX, mode="point_to_plane", loss="tukey", scale=1e-9, scale_start=1e-9,
                   ref_normals=nref, voxel_size=RUN_VOXEL, max_iter=3)
    with pytest.raises(np.linalg.LinAlgError, match="d_max"):
        icp_robust(scan, ref, RigidTransform(), 1e-9, mode="point_to_point", loss="cauchy", scale=1e-3, voxel_size=RUN_VOXEL, max_iter=3)


# ---- 7. pipeline -----------------------------------------------------------------------------------------------------------------------
def test_pipeline_routes_a_loss_to_icp_robust_and_none_to_todays_function(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_generalized, icp_point_to_plane, icp_robust
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    scan, na, ref, nref, r0, t0 = clutter_run_set()
    pipe = RegistrationPipeline(scan=scan, scan_normals=na, ref=ref, ref_normals=nref)
    common = dict(d_max=S.D_MAX, voxel_size=0.01, max_iter=20, rms_threshold=0.0)

    def same(x, y):
        return np.array_equal(x[0].rotation, y[0].rotation) and np.array_equal(x[0].translation, y[0].translation) and x[1:] == y[1:]

    got = pipe.run_icp("point_to_plane", RigidTransform(), robust_loss="geman_mcclure", robust_scale=S.SCALE, **common)
    want = icp_robust(scan, ref, RigidTransform(), S.D_MAX, mode="point_to_plane", loss="geman_mcclure", scale=S.SCALE, ref_normals=nref,
                      voxel_size=0.01, max_iter=20, rms_threshold=0.0)
    assert same(got, want)
    none = pipe.run_icp("point_to_plane", RigidTransform(), **common)
    assert same(none, icp_point_to_plane(scan, ref, nref, RigidTransform(), **common))
    assert G.rotation_error(got[0].rotation, r0) < 0.5 * G.rotation_error(none[0].rotation, r0)  # and the loss is what it is for
    k, k0 = S.table_scales("generalized", "tukey")
    got = pipe.run_icp("generalized", RigidTransform(), robust_loss="tukey", robust_scale=k, robust_scale_start=k0, gicp_epsilon=EPS, **common)
    want = icp_robust(scan, ref, RigidTransform(), S.D_MAX, mode="generalized", loss="tukey", scale=k, scale_start=k0, ref_normals=nref,
                      scan_normals=na, epsilon=EPS, voxel_size=0.01, max_iter=20, rms_threshold=0.0)
    assert same(got, want)
    assert same(pipe.run_icp("generalized", RigidTransform(), **common),
                icp_generalized(scan, ref, RigidTransform(), S.D_MAX, scan_normals=na, ref_normals=nref, voxel_size=0.01, max_iter=20,
                                rms_threshold=0.0))
    with pytest.raises(ValueError, match="robust_scale"):
        pipe.run_icp("point_to_plane", RigidTransform(), robust_loss="cauchy", **common)
