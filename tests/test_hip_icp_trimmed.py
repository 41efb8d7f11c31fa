"""Trimmed ICP on the MI355X (K18: sf_select_kth, csrc/select.hip; k_icp_keys, k_icp_sums, sf_icp_accumulate_trimmed, csrc/icp.hip;
shot_fpfh_amd.icp.icp_trimmed) against the NumPy statement (tests/icp_trimmed_numpy.py).

The selection is held to np.partition by exact equality: value and both counts.  ONE pass of the chain is held as its siblings are
(tests/test_hip_icp_robust.py): n0, the rank, the cut and the used pair count EQUAL the statement's -- the `d_max` gate and the pair
count are already held exactly on the same operations, and the residual is formed by one function for the key pass and both sums
passes -- and each fit sum within C k 2^-53 sum|term| of its math.fsum value with K17's C_ROUNDINGS, since no new rounding enters a
term; the slots of no pass are exactly 0.0.  The whole run is held to ten times the statement's own sensitivity to the order of its
sums, with the iteration count, the flag and every iteration's (n0, rank, used) exact.

The input sets and the `measure_*` functions are plain functions: tests/test_icp_trimmed_host.py asserts the conditions the tests
below place on their inputs without a device, and tools/icp_trimmed_parity.py writes profiles/icp_trimmed_parity.md from them."""
import ctypes as C

import numpy as np
import pytest

import gicp_numpy as G
import icp_numpy as I
import icp_robust_numpy as S
import icp_trimmed_numpy as TR
import test_hip_icp_robust as H
import test_hip_icp_sums as T
from test_hip_gicp import assert_unambiguous, one_pass_set

pytestmark = pytest.mark.gpu

U = 2.0**-53
D_MAX = T.D_MAX
EPS = H.EPS
TRIMS = [1e-5, 0.3, 0.5, 0.8, 1.0]  # rank 1 at every size of the one-pass test; three shares; no selection
ONE_PASS_LOSSES = [S.LOSSES["none"], S.LOSSES["cauchy"], S.LOSSES["tukey"]]
RUN_ITERATIONS = 20  # the share comes down to 0.8 in ten iterations; ten more at it
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


# ---- the device side -----------------------------------------------------------------------------------------------------------------
def device_select(eng, dev, n, rank):
    out = np.full(4, -1.0)
    from shot_fpfh_amd import _ffi

    _ffi.check(eng.lib.sf_select_kth(eng.h, dev.ptr, n, rank, out.ctypes.data_as(C.c_void_p)), "sf_select_kth")
    return out


class _Resident(H._Resident):
    """`trimmed` is one sf_icp_accumulate_trimmed call as `_Registration.pairs` makes it"""

    def trimmed(self, mode, loss, k, trim, R, t, d_max, rows=None, eps=EPS):
        if trim == 1.0 and rows is None:  # `pairs` routes a trim of 1.0 to the call of today: the C call itself
            rc, raw = raw_trimmed(self.reg.engine, self.reg, mode, loss, k, trim, d_max, R, t, eps=eps)
            assert rc == 0
            return raw
        got = self.reg.pairs(mode, d_max, moved_by=self._by(R, t), rows=rows, epsilon=eps, loss=loss, scale=k, trim=trim)
        assert got.raw.shape == (48,)
        return got.raw


def raw_trimmed(eng, reg, mode, loss, k, trim, d_max, R=None, t=None, m=None, nrm=True, eps=EPS):
    """the C call itself over all rows: (return code, 48 numbers)"""
    from shot_fpfh_amd.core import RigidTransform

    raw = np.full(48, -1.0)
    rt = None if R is None else np.ascontiguousarray(RigidTransform(R, t).as_row12())
    rc = eng.lib.sf_icp_accumulate_trimmed(eng.h, reg.ref.h, reg.points.ptr, reg.normals.ptr if nrm and reg.normals is not None else None,
                                           None, reg.n if m is None else m, None if rt is None else rt.ctypes.data_as(C.c_void_p),
                                           float(d_max), mode, float(eps), loss, float(k), float(trim), raw.ctypes.data_as(C.c_void_p))
    return rc, raw


def check_sums(got, mode, loss, k, trim, a, na, ref, nref, R, t, d_max, label, eps=EPS, tree=None):
    """`got` (48 doubles of the device) against the statement, mode 0 centred with the weighted centroids `got` itself implies:
    [0], [37], [38], [47] equal, the rest within K17's bound over the USED pairs.  Returns the worst ratio."""
    assert got.shape == (48,)
    want = TR.sums(mode, loss, k, trim, a, na, ref, nref, R, t, d_max, eps, means=S.device_means(got) if mode == S.POINT else None, tree=tree)
    n, c = want["count"], H.C_ROUNDINGS[mode]
    print(f"{label}: n0 = {got[37]:.0f} (statement {want['n0']}), rank = {got[38]:.0f} ({want['rank']}), used = {got[0]:.0f} ({n}), "
          f"cut = {got[47]!r} ({want['cut']!r})")
    assert (got[0], got[37], got[38]) == (n, want["n0"], want["rank"]), label
    assert got[47] == want["cut"] and not np.signbit(got[47]), (label, got[47], want["cut"])
    err = np.abs(got - want["vec"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want["abs"] > 0, err / (n * U * want["abs"]), 0.0))) if n else 0.0
    print(f"{label}: sum w = {got[7]:.6g}, worst |sum - fsum| = {worst:.3g} x k 2^-53 sum|term| (bound {c})")
    assert np.all(err <= c * n * U * want["abs"]), (label, np.flatnonzero(err > c * n * U * want["abs"]), worst)
    assert np.all(got[want["abs"] == 0] == want["vec"][want["abs"] == 0])
    assert not got[TR.UNUSED[mode]].any(), (label, got[TR.UNUSED[mode]])  # the slots of no pass: exactly 0.0
    return worst


def one_pass_states(m):
    """identity, true motion and 0.3 rad away; at the largest size, where the statement's fsum takes a second per call, the true
    motion alone (it keeps the most pairs)"""
    states = one_pass_set()["states"]
    return states if m < T.M_SIZES[-1] else states[1:2]


def measure_one_pass(eng, mode, loss, m, trims=TRIMS):
    """worst ratio over the states and the trims at m scan rows; two calls bit for bit"""
    s = one_pass_set()
    a, na = s["scan"][:m], s["na"][:m]
    worst = 0.0
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in one_pass_states(m):
            assert_unambiguous(s, a, R, t, D_MAX, (m, label))
            for trim in trims:
                got = dev.trimmed(mode, loss, H.K_ONE[mode], trim, R, t, D_MAX)
                assert np.array_equal(got, dev.trimmed(mode, loss, H.K_ONE[mode], trim, R, t, D_MAX))
                worst = max(worst, check_sums(got, mode, loss, H.K_ONE[mode], trim, a, na, s["ref"], s["nref"], R, t, D_MAX,
                                              f"mode {mode} loss {loss} trim {trim} m={m} {label}", tree=s["tree"]))
    return worst


# ---- 1. the selection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TR.SELECT_SIZES)
@pytest.mark.parametrize("family", TR.SELECT_FAMILIES)
def test_select_kth_equals_np_partition(eng, family, n):
    """n = 1, 2: one lane; 63, 64, 65: a wave -+ 1; 257: a block + 1; 65 536, 65 537: one full stride of the 256 x 256 grid, + 1;
    200 001: several strides.  Ranks 1, 2, ceil(n / 2), n - 1, n and every tie boundary -+ 1.  The value (bit for bit, a zero as
    +0.0) and both counts EQUAL the statement's, and a second call returns the same bits."""
    x = TR.select_keys(family, n)
    dev = eng.empty((n,)).from_host(x)
    try:
        for rank in TR.select_ranks(x):
            v, below, at_or_below = TR.select_kth(x, rank)
            got = device_select(eng, dev, n, rank)
            assert got.view(np.uint64)[0] == np.float64(v).view(np.uint64), (family, n, rank, got[0], v)
            assert (got[1], got[2], got[3]) == (below, at_or_below, 0.0), (family, n, rank, got, below, at_or_below)
            again = device_select(eng, dev, n, rank)
            assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    finally:
        dev.free()


def test_select_kth_argument_errors_name_the_argument(eng):
    from shot_fpfh_amd import _ffi

    dev = eng.empty((8,)).from_host(np.arange(8.0))
    out = np.zeros(4)
    po = out.ctypes.data_as(C.c_void_p)
    try:
        for args, word in (((eng.h, dev.ptr, 0, 1, po), "n "), ((eng.h, dev.ptr, -3, 1, po), "n "), ((eng.h, dev.ptr, 8, 0, po), "rank"),
                           ((eng.h, dev.ptr, 8, 9, po), "rank"), ((eng.h, None, 8, 1, po), "keys_dev"), ((eng.h, dev.ptr, 8, 1, None), "out"),
                           ((None, dev.ptr, 8, 1, po), "ctx")):
            assert eng.lib.sf_select_kth(*args) != 0
            assert "sf_select_kth: bad argument " + word in _ffi.last_error(), (word, _ffi.last_error())
        assert eng.lib.sf_select_kth(eng.h, dev.ptr, 8, 8, po) == 0 and out.tolist() == [7.0, 7.0, 8.0, 0.0]
    finally:
        dev.free()


# ---- 2. one pass of the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", T.M_SIZES)
@pytest.mark.parametrize("loss", ONE_PASS_LOSSES)
@pytest.mark.parametrize("mode", H.MODE_IDS)
def test_one_pass_equals_the_statement(eng, mode, loss, m):
    """The sizes of tests/test_hip_icp_sums.py; identity, true motion and 0.3 rad away; trims for rank 1, 0.3, 0.5, 0.8 and none;
    no loss, Cauchy and Tukey.  n0, rank, cut and the used count equal, the sums within the sibling bound, two calls bit for bit."""
    worst = measure_one_pass(eng, mode, loss, m)
    print(f"mode {mode}, loss {loss}, m = {m}: worst ratio {worst:.3g} of {H.C_ROUNDINGS[mode]}")


# ---- 3. ties ------------------------------------------------------------------------------------------------------------------------------
def test_ties_at_the_cut_are_all_used(eng):
    """`mixed`: 103 pairs of d2 = 0 and 409 of d2 = 25 2^-14, all inside d_max = 5 2^-7.  The rank 103 cuts at 0.0 and uses the
    103; the rank 104 cuts at 25 2^-14 and uses all 512, whatever their order; with d_max just below 5 2^-7 only the 103 are
    inside it and every trim uses all of them."""
    L = T.lattice_set()
    d2 = 25 * 2.0**-14
    with _Resident(eng, L["mixed"], None, L["ref"], L["nref"]) as dev:
        for trim, used, cut in ((103 / 512, 103, 0.0), (104 / 512, 512, d2), (0.5, 512, d2), (1e-5, 103, 0.0)):
            for R, t in ((None, None), (np.eye(3), np.zeros(3))):
                got = dev.trimmed(S.POINT, 0, 1.0, trim, R, t, T.LATTICE_R)
                assert (got[37], got[38], got[0], got[47]) == (512, TR.trim_rank(trim, 512), used, cut), (trim, got[[37, 38, 0, 47]])
                assert got[17] == (used - 103) * d2 and got[7] == used  # sum d2 and sum w are exact here
                check_sums(got, S.POINT, 0, 1.0, trim, L["mixed"], None, L["ref"], L["nref"], R, t, T.LATTICE_R, f"lattice trim {trim}",
                           tree=L["tree"])
        below = float(np.nextafter(T.LATTICE_R, 0.0))
        for trim in TRIMS:
            got = dev.trimmed(S.POINT, 0, 1.0, trim, None, None, below)
            assert (got[0], got[37], got[38], got[47], got[17]) == (103, 103, TR.trim_rank(trim, 103), 0.0, 0.0), (trim, got[[0, 37, 38, 47]])


# ---- 4. boundaries of the chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", H.MODE_IDS)
def test_trim_one_is_the_robust_call_bit_for_bit(eng, mode):
    s = one_pass_set()
    a, na = s["scan"][:5000], s["na"][:5000]
    same = list(range(37)) + list(range(40, 47))
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for label, R, t in s["states"]:
            for loss in (S.LOSSES["none"], S.LOSSES["huber"], S.LOSSES["tukey"]):
                want = dev.sums(mode, loss, H.K_ONE[mode], R, t, D_MAX)
                rc, got = raw_trimmed(eng, dev.reg, mode, loss, H.K_ONE[mode], 1.0, D_MAX, R, t)
                assert rc == 0 and want[0] > 0
                assert np.array_equal(got[same], want[same]), (label, loss, np.flatnonzero(got != want))
                assert got[37] == got[38] == got[0] and got[47] == 0.0 and got[39] == 0.0
                # through `pairs` a trim of 1.0 IS the call of today
                assert np.array_equal(dev.reg.pairs(mode, D_MAX, moved_by=dev._by(R, t), epsilon=EPS, loss=loss, scale=H.K_ONE[mode], trim=1.0).raw, want)


@pytest.mark.parametrize("mode", H.MODE_IDS)
def test_selection_null_transform_and_zero_normals(eng, mode):
    s = one_pass_set()
    a, na, ids = s["scan"][:5000], s["na"][:5000].copy(), T.selection_ids()
    nref = s["nref"].copy()
    if mode == S.GICP:
        na[::7] = 0.0   # scan points without a normal: C = I
        nref[::11] = 0.0
    label, R, t = s["states"][1]
    loss, k = S.LOSSES["cauchy"], H.K_ONE[mode]
    with _Resident(eng, a, na, s["ref"], nref) as dev:
        for rows, pts, nrm in ((ids, a[ids], na[ids]), (None, a, na)):
            for R2, t2 in ((R, t), (None, None)):
                assert_unambiguous(s, pts, R2, t2, D_MAX, "selection")
                got = dev.trimmed(mode, loss, k, 0.5, R2, t2, D_MAX, rows=rows)
                assert np.array_equal(got, dev.trimmed(mode, loss, k, 0.5, R2, t2, D_MAX, rows=rows))
                check_sums(got, mode, loss, k, 0.5, pts, nrm, s["ref"], nref, R2, t2, D_MAX,
                           f"mode {mode} {'selection' if rows is not None else 'all rows'} {'moved' if R2 is not None else 'as is'}",
                           tree=s["tree"])
        got = dev.trimmed(mode, loss, k, 0.5, R, t, D_MAX, rows=np.zeros(0, dtype=np.int64))  # an empty selection: no device work
        assert got.shape == (48,) and not got.any()


def test_no_pair_inside_d_max_and_a_single_pair(eng):
    s = one_pass_set()
    a, na = s["scan"][:5000], s["na"][:5000]
    label, R, t = s["states"][1]
    assert I.kept_pairs(a, s["ref"], R, t, T.NO_PAIR_RADIUS, s["tree"])[0].shape[0] == 0
    d = s["tree"].query(G.move(R, t, a))[0]
    one = float(0.5 * (np.sort(d)[0] + np.sort(d)[1]))  # between the nearest pair and the second nearest: n0 = 1
    with _Resident(eng, a, na, s["ref"], s["nref"]) as dev:
        for mode in H.MODE_IDS:
            for trim in (1e-5, 0.5):
                got = dev.trimmed(mode, S.LOSSES["cauchy"], H.K_ONE[mode], trim, R, t, T.NO_PAIR_RADIUS)
                assert got.shape == (48,) and not got.any()
                got = dev.trimmed(mode, S.LOSSES["cauchy"], H.K_ONE[mode], trim, R, t, one)
                assert (got[0], got[37], got[38]) == (1, 1, 1)
                check_sums(got, mode, S.LOSSES["cauchy"], H.K_ONE[mode], trim, a, na, s["ref"], s["nref"], R, t, one, f"mode {mode}: one pair",
                           tree=s["tree"])


def test_argument_errors_name_the_argument(eng):
    from shot_fpfh_amd import ShotFpfhError, _ffi

    s = one_pass_set()
    with _Resident(eng, s["scan"][:100], s["na"][:100], s["ref"], s["nref"]) as dev:
        for kw, word in ((dict(trim=0.0), "trim"), (dict(trim=-0.5), "trim"), (dict(trim=1.5), "trim"), (dict(trim=float("nan")), "trim"),
                         (dict(loss=5), "loss"), (dict(k=0.0), "scale"), (dict(mode=3), "mode"), (dict(mode=S.GICP, eps=0.0), "epsilon")):
            args = dict(mode=S.PLANE, loss=2, k=0.02, eps=EPS, trim=0.5)
            args.update(kw)
            rc, raw = raw_trimmed(eng, dev.reg, args["mode"], args["loss"], args["k"], args["trim"], D_MAX, eps=args["eps"])
            assert rc != 0 and "sf_icp_accumulate_trimmed: bad argument " + word in _ffi.last_error(), (word, _ffi.last_error())
        rc, raw = raw_trimmed(eng, dev.reg, S.GICP, 2, 0.5, 0.5, D_MAX, nrm=False)
        assert rc != 0 and "nrm_dev" in _ffi.last_error()
        rc, raw = raw_trimmed(eng, dev.reg, S.PLANE, 2, 0.5, 0.5, D_MAX, m=-1)
        assert rc != 0 and "m (negative)" in _ffi.last_error()
        rc, raw = raw_trimmed(eng, dev.reg, S.PLANE, 2, 0.5, 0.5, D_MAX, m=0)
        assert rc == 0 and not raw.any()
    with _Resident(eng, s["scan"][:100], None, s["ref"], None) as dev:  # a reference without normals
        with pytest.raises(ShotFpfhError, match="normals"):
            dev.trimmed(S.PLANE, 2, 0.02, 0.5, None, None, D_MAX)
        assert dev.trimmed(S.POINT, 2, 0.02, 0.5, None, None, D_MAX)[0] > 0


# ---- 5. whole runs -----------------------------------------------------------------------------------------------------------------------
def _record_pairs(monkeypatch):
    from shot_fpfh_amd.icp import _Registration

    calls, real = [], _Registration.pairs

    def pairs(self, *a, **kw):
        found = real(self, *a, **kw)
        calls.append((kw.get("trim", 1.0), found))
        return found

    monkeypatch.setattr(_Registration, "pairs", pairs)
    return calls


def run_device(mode_name, overlap=TR.OVERLAP, anneal=TR.ANNEAL, **kw):
    """`icp_trimmed` on the clutter set from the identity"""
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_trimmed

    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    args = dict(overlap=overlap, anneal_iterations=anneal, mode=mode_name, ref_normals=nref, scan_normals=na, epsilon=EPS,
                voxel_size=H.RUN_VOXEL, max_iter=RUN_ITERATIONS, rms_threshold=0.0, step_tolerance=0.0)
    args.update(kw)
    return icp_trimmed(scan, ref, RigidTransform(), S.D_MAX, **args)


def run_statement(mode_name, how="fsum", order=None, overlap=TR.OVERLAP, anneal=TR.ANNEAL, **kw):
    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    if order is not None:
        scan, na = scan[order], na[order]
    args = dict(max_iter=RUN_ITERATIONS, rms_threshold=0.0, step_tolerance=0.0)
    args.update(kw)
    return TR.refine(scan, na, ref, nref, S.MODES[mode_name], S.D_MAX, overlap, anneal, eps=EPS, how=how, **args)


def measure_whole_run(mode_name, calls):
    """`icp_trimmed` for a fixed number of iterations against the fsum statement; `own` = the statement's fsum run against four runs
    on row-permuted scans with NumPy's pairwise sums, the largest difference of R and t"""
    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    exact = run_statement(mode_name)
    own = 0.0
    for seed in range(4):
        order = np.random.default_rng(17 + seed).permutation(scan.shape[0])
        other = run_statement(mode_name, how="np", order=order)
        own = max(own, H._diff(exact["R"], exact["t"], other["R"], other["t"]))
    del calls[:]
    tf, rms, converged = run_device(mode_name)
    # a share of 1.0 goes through the call of today, which reports no selection: all its pairs are used
    selections = [(f.count, f.count, f.count) if trim == 1.0 else (f.inside, f.rank, f.count) for trim, f in calls]
    return dict(device_vs_statement=H._diff(tf.rotation, tf.translation, exact["R"], exact["t"]), own=own, iterations=len(calls),
                shares=[trim for trim, f in calls], want_shares=exact["shares"], selections=selections, want_selections=exact["selections"],
                want_iterations=exact["iterations"], converged=bool(converged), rms_device=rms, rms_statement=exact["rms"],
                rotation_error=G.rotation_error(tf.rotation, r0), rotation_error_statement=G.rotation_error(exact["R"], r0))


@pytest.mark.parametrize("mode_name", list(S.MODES))
def test_whole_run_agrees_with_the_statement(eng, monkeypatch, mode_name):
    """`clutter_set(0)` through `icp_trimmed` from the identity, overlap 0.8 annealed over 10 iterations, a FIXED number of
    iterations (rms_threshold = 0, step_tolerance = 0).  Iteration count, flag, the share and (n0, rank, used) of every iteration
    exact, rms to 1e-9 relative, max(|dR|, |dt|) within ten times the statement's own sensitivity to the order of its sums."""
    r = measure_whole_run(mode_name, _record_pairs(monkeypatch))
    print(f"{mode_name}: device vs fsum statement {r['device_vs_statement']:.3e} after {r['iterations']} iterations; the statement's own "
          f"fsum vs permuted np.sum {r['own']:.3e}; bound 10 x that; |R - R0| = {r['rotation_error']:.2e} (statement "
          f"{r['rotation_error_statement']:.2e}); rms {r['rms_device']:.12e} vs {r['rms_statement']:.12e}; last (n0, rank, used) "
          f"{r['selections'][-1]}")
    assert (r["iterations"], r["converged"]) == (r["want_iterations"], False) and r["want_iterations"] == RUN_ITERATIONS
    assert r["shares"] == r["want_shares"] and r["selections"] == r["want_selections"]
    assert np.isclose(r["rms_device"], r["rms_statement"], rtol=1e-9, atol=0.0)
    assert r["device_vs_statement"] <= 10 * r["own"], (r["device_vs_statement"], r["own"])


def test_step_stop_waits_for_the_share(eng, monkeypatch):
    """a tolerance above every step stops at the first iteration whose share is `overlap`, not before"""
    calls = _record_pairs(monkeypatch)
    tf, rms, converged = run_device("point_to_plane", step_tolerance=10.0)
    assert (len(calls), bool(converged)) == (TR.ANNEAL + 1, True) and calls[-1][0] == TR.OVERLAP
    want = run_statement("point_to_plane", step_tolerance=10.0)
    assert want["iterations"] == TR.ANNEAL + 1 and want["converged"] and np.isclose(rms, want["rms"], rtol=1e-9, atol=0.0)


def test_overlap_one_without_a_loss_is_the_plain_function_bit_for_bit(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_generalized, icp_point_to_plane, icp_point_to_point

    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    common = dict(voxel_size=H.RUN_VOXEL, max_iter=8, rms_threshold=0.0)
    want = {"point_to_point": icp_point_to_point(scan, ref, RigidTransform(), S.D_MAX, **common),
            "point_to_plane": icp_point_to_plane(scan, ref, nref, RigidTransform(), S.D_MAX, **common),
            "generalized": icp_generalized(scan, ref, RigidTransform(), S.D_MAX, scan_normals=na, ref_normals=nref, epsilon=EPS,
                                           step_tolerance=0.0, **common)}
    for mode_name, (tf, rms, converged) in want.items():
        got = run_device(mode_name, overlap=1.0, max_iter=8)
        assert np.array_equal(got[0].rotation, tf.rotation) and np.array_equal(got[0].translation, tf.translation), mode_name
        assert (got[1], bool(got[2])) == (rms, bool(converged)), mode_name


# ---- 6. pipeline ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_routes_an_overlap_to_icp_trimmed(eng):
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.icp import icp_trimmed
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    pipe = RegistrationPipeline(scan=scan, scan_normals=na, ref=ref, ref_normals=nref)
    common = dict(d_max=S.D_MAX, voxel_size=0.01, max_iter=20, rms_threshold=0.0)

    def same(x, y):
        return np.array_equal(x[0].rotation, y[0].rotation) and np.array_equal(x[0].translation, y[0].translation) and x[1:] == y[1:]

    got = pipe.run_icp("point_to_plane", RigidTransform(), trim_overlap=0.8, **common)
    want = icp_trimmed(scan, ref, RigidTransform(), S.D_MAX, overlap=0.8, mode="point_to_plane", ref_normals=nref, voxel_size=0.01,
                       max_iter=20, rms_threshold=0.0)
    assert same(got, want)
    none = pipe.run_icp("point_to_plane", RigidTransform(), **common)
    assert G.rotation_error(got[0].rotation, r0) < 0.5 * G.rotation_error(none[0].rotation, r0)  # and the trimming is what it is for
    got = pipe.run_icp("generalized", RigidTransform(), trim_overlap=0.8, trim_anneal_iterations=5, robust_loss="cauchy",
                       robust_scale=S.table_scales("generalized", "cauchy")[0], gicp_epsilon=EPS, **common)
    want = icp_trimmed(scan, ref, RigidTransform(), S.D_MAX, overlap=0.8, anneal_iterations=5, mode="generalized", loss="cauchy",
                       scale=S.table_scales("generalized", "cauchy")[0], ref_normals=nref, scan_normals=na, epsilon=EPS, voxel_size=0.01,
                       max_iter=20, rms_threshold=0.0)
    assert same(got, want)
