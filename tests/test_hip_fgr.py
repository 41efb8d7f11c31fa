"""Fast global registration on the MI355X (K12, csrc/fgr.hip) against the NumPy statement of the definition (tests/fgr_numpy.py).

The check is split where the definition leaves rounding to the implementation.  ONE pass (sf_fgr_sums) is held to the math.fsum
value of each of its 29 sums within c k 2^-53 sum|term|; the whole optimisation (sf_fgr) amplifies rounding through 64 dependent
steps, so its bound is ten times the definition's own sensitivity to the order of its sums, measured on the NumPy statement
alone; the schedule (mu), status, iteration and inlier counts are exact."""
import numpy as np
import pytest

import fgr_numpy as F
import ransac_numpy as N
from shot_fpfh_amd.matching import fast_global_registration

pytestmark = pytest.mark.gpu

U = 2.0**-53
THR = 0.01
# Roundings that enter one term as k12_fgr_sums forms it from the loaded coordinates (the longest chain, the cross-product and
# E columns): x and y, a subtraction and a division per component (12); p = ((r0 x0 + r1 x1) + r2 x2) + t, 6 per component (18);
# r = p - y (3); r.r (5); l = mu / (mu + r.r) (2); w = l l (1); w r for two components (2); p1 wr2 - p2 wr1 (3): 46.  The NumPy
# statement forms every term by the same operations in the same order, so what really differs is the order of the k additions
# (k - 1 roundings, each relative to a partial sum of magnitude <= sum|term|): c k 2^-53 sum|term| covers both with room to spare.
C_ROUNDINGS = 46
SYNTH = [(5000, 0.5), (5000, 0.2), (5000, 0.1), (20000, 0.5), (20000, 0.2), (20000, 0.1)]  # test_hip_ransac_prerejective.SYNTH
ACCURACY_SETS = [(20000, 0.30, 0), (20000, 0.10, 1), (20000, 0.05, 2), (2000, 0.30, 3), (200000, 0.30, 4), (20000, 0.50, 5)]
CAP = 2e-3
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _matches(name):
    if name not in _cache:
        if name == "duplicates":  # 40 distinct reference keypoints for 4000 matches
            sk, rk, si, ri, r0, t0 = N.synthetic_matches(4000, 0.5, seed=11)
            _cache[name] = (sk, rk, si, ri[np.random.default_rng(3).integers(0, 40, 4000)], r0, t0)
        elif len(name) == 3:
            _cache[name] = N.synthetic_matches(name[0], name[1], seed=name[2])
        else:
            m, share = name
            _cache[name] = N.synthetic_matches(m, share, seed=m + int(100 * share))
    return _cache[name]


class _Resident:
    """The matched points of a set on the device."""

    def __init__(self, eng, name):
        sk, rk, si, ri, self.r0, self.t0 = _matches(name)
        self.a, self.b = N.matched_points(si, ri, sk, rk)
        self.m = self.a.shape[0]
        self.eng, self.held = eng, [eng.empty((self.m, 3)), eng.empty((self.m, 3))]
        self.da, self.db = self.held
        self.da.from_host(self.a), self.db.from_host(self.b)

    def sel(self, ids):
        d = self.eng.empty((len(ids),), np.int64)
        self.held.append(d)
        return d.from_host(np.asarray(ids, dtype=np.int64))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in self.held:
            h.free()


def _states(dev, a, b):
    """(label, 20 state doubles, R, t, mu) at identity, the true motion and 0.3 rad from it, mu in {1, 1e-2, mu_floor}; x, y."""
    ca, cb, s, x, y = F.normalise(a, b)
    t_true = (dev.r0 @ ca + dev.t0 - cb) / s
    away = F.rodrigues(0.3 * np.array([2.0, -1.0, 2.0]) / 3.0) @ dev.r0
    out = []
    for label, rot, t in (("identity", np.eye(3), np.zeros(3)), ("true", dev.r0, t_true), ("0.3 rad", away, t_true)):
        for mu in (1.0, 1e-2, (THR / s) ** 2):
            out.append((f"{label} mu={mu:.3g}", np.concatenate([ca, cb, [s], rot.reshape(9), t, [mu]]), rot, t, mu))
    return out, x, y


def _check_sums(got, want, k, label):
    assert got[29] == k and got[30] == 0 and got[31] == 0, (label, got[29:])
    err = np.abs(got[:29] - want["vec"])
    bound = C_ROUNDINGS * k * U * want["abs"]
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(want["abs"] > 0, err / (k * U * want["abs"]), 0.0)))
    print(f"{label}: k = {k}, worst |sum - fsum| = {worst:.3g} x k 2^-53 sum|term| (bound {C_ROUNDINGS})")
    assert np.all(err <= bound), (label, np.flatnonzero(err > bound), worst)
    assert np.all(got[:29][want["abs"] == 0] == 0)  # A's structural zeros


# ---- 6. one pass --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYNTH + ["duplicates"], ids=str)
def test_one_pass_equals_fsum_within_the_rounding_bound(eng, name):
    with _Resident(eng, name) as dev:
        states, x, y = _states(dev, dev.a, dev.b)
        for label, st, rot, t, mu in states:
            got = eng.fgr_sums(dev.da, dev.db, dev.m, st)
            assert np.array_equal(got, eng.fgr_sums(dev.da, dev.db, dev.m, st))  # two calls, bit for bit
            _check_sums(got, F.sums(x, y, rot, t, mu), dev.m, f"{name} {label}")
        # a selection with repeated ids
        ids = np.random.default_rng(5).integers(0, dev.m, 777)
        ca, cb, s, xs, ys = F.normalise(dev.a[ids], dev.b[ids])
        st = np.concatenate([ca, cb, [s], dev.r0.reshape(9), np.zeros(3), [0.05]])
        got = eng.fgr_sums(dev.da, dev.db, dev.m, st, sel=dev.sel(ids))
        _check_sums(got, F.sums(xs, ys, dev.r0, np.zeros(3), 0.05), 777, f"{name} selection")


@pytest.mark.parametrize("k", [3, 64, 65, 1000003])
def test_one_pass_row_counts(eng, k):
    """k below, at and just over a wave, and past the grid's 1024 x 256 rows (the grid-stride loop wraps, the last block is ragged)."""
    with _Resident(eng, (max(k, 1000), 0.3, 7)) as dev:
        a, b = dev.a[:k], dev.b[:k]
        states, x, y = _states(dev, a, b)
        for label, st, rot, t, mu in states:
            got = eng.fgr_sums(dev.da, dev.db, dev.m, st, k=k)
            assert np.array_equal(got, eng.fgr_sums(dev.da, dev.db, dev.m, st, k=k))
            _check_sums(got, F.sums(x, y, rot, t, mu), k, f"k={k} {label}")


def test_one_pass_argument_errors(eng):
    from shot_fpfh_amd import ShotFpfhError

    with _Resident(eng, (5000, 0.5)) as dev:
        st = np.concatenate([np.zeros(6), [1.0], np.eye(3).reshape(9), np.zeros(3), [1.0]])
        with pytest.raises(ShotFpfhError, match="at least 3"):
            eng.fgr_sums(dev.da, dev.db, dev.m, st, k=2)
        with pytest.raises(ShotFpfhError, match="outside"):
            eng.fgr_sums(dev.da, dev.db, dev.m, st, sel=dev.sel([0, 1, dev.m, 2]))  # never dereferenced, reported
        for kw in (dict(iterations=0), dict(decrease_every=0), dict(division_factor=1.0)):
            with pytest.raises(ShotFpfhError, match="sf_fgr"):
                eng.fgr_device(dev.da, dev.db, dev.m, THR, **kw)
        with pytest.raises(ShotFpfhError):
            eng.fgr_device(dev.da, dev.db, dev.m, float("nan"))
        with pytest.raises(ShotFpfhError, match="outside"):
            eng.fgr_device(dev.da, dev.db, dev.m, THR, sel=dev.sel([0, 1, -1, 2]))


# ---- 7. the whole optimisation -------------------------------------------------------------------------------------------------------
def _diff(r1, t1, r2, t2):
    return max(float(np.abs(r1 - r2).max()), float(np.abs(t1 - t2).max()))


@pytest.fixture(scope="module")
def sensitivity():
    """The definition run twice per set -- sums by math.fsum, and by np.sum over a permuted row order: the largest difference of
    the two transforms over the sets is its own sensitivity to the order of summation."""
    runs, worst = {}, 0.0
    for name in SYNTH + ["duplicates"]:
        sk, rk, si, ri = _matches(name)[:4]
        a, b = N.matched_points(si, ri, sk, rk)
        exact = F.fgr_rows(a, b, THR)
        other = F.fgr_rows(a, b, THR, how="np", order=np.random.default_rng(17).permutation(a.shape[0]))
        d = _diff(exact["R"], exact["t"], other["R"], other["t"])
        runs[str(name)] = (exact, d)
        worst = max(worst, d)
    return runs, worst


@pytest.mark.parametrize("name", SYNTH + ["duplicates"], ids=str)
def test_optimisation_agrees_with_the_definition(eng, sensitivity, name):
    runs, worst = sensitivity
    exact, own = runs[str(name)]
    with _Resident(eng, name) as dev:
        rt, info, trace = eng.fgr_device(dev.da, dev.db, dev.m, THR)
    d = _diff(rt[:9].reshape(3, 3), rt[9:], exact["R"], exact["t"])
    print(f"{name}: device vs fsum statement {d:.3e}; the statement's own fsum vs permuted np.sum {own:.3e}; bound 10 x {worst:.3e}")
    assert (int(info[0]), int(info[1])) == (exact["status"], exact["iterations"]) == (0, 64)
    assert np.array_equal(trace[:, 0], exact["trace"][:, 0])  # the schedule, exactly
    assert info[2] == exact["mu"] and np.isclose(info[3], exact["s"], rtol=1e-14)
    assert np.allclose(trace[:, 1:3], exact["trace"][:, 1:3], rtol=1e-9) and np.isclose(info[4], exact["E"], rtol=1e-9)
    assert d <= 10 * worst, (d, worst)


# ---- 8. degenerate input ---------------------------------------------------------------------------------------------------------------
def test_points_on_one_line_are_degenerate(eng):
    line = np.outer(np.linspace(-1, 1, 300), [1.0, 2.0, -0.5])
    idx = np.arange(300)
    da, db = eng.empty((300, 3)), eng.empty((300, 3))
    try:
        da.from_host(line + 0.3), db.from_host(line - 0.1)
        rt, info, trace = eng.fgr_device(da, db, 300, THR)
    finally:
        da.free(), db.free()
    assert int(info[0]) == 1 and int(info[1]) == 0
    assert np.isfinite(rt).all() and np.isfinite(info).all() and np.isfinite(trace).all() and not trace.any()
    assert np.array_equal(rt[:9], np.eye(3).reshape(9))  # the transform before the failed step
    with pytest.raises(ValueError, match="degenerate"):
        fast_global_registration(idx, idx, line + 0.3, line - 0.1, distance_threshold=THR, engine=eng)
    one = np.full((50, 3), 0.25)
    with pytest.raises(ValueError, match="extent"):
        fast_global_registration(idx[:50], idx[:50], one, one, distance_threshold=THR, engine=eng)


def test_three_generic_points_are_fitted_exactly(eng):
    a = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.7]])
    b = a @ F.rodrigues(np.array([0.3, -0.2, 0.4])).T + [0.2, -0.1, 0.05]
    idx = np.arange(3)
    ratio, tf, rec = fast_global_registration(idx, idx, a, b, distance_threshold=THR, engine=eng)
    res = float(np.abs(a @ tf.rotation.T + tf.translation - b).max())
    print(f"three points: residual {res:.3e}, s = {rec.scale:.3f}")
    assert rec.status == "done" and rec.rows == 3 and ratio == 1.0 and res <= 1e-12 * rec.scale


# ---- 9, 11, 13. determinism, the inlier ratio, no wait inside -------------------------------------------------------------------------
def test_repeats_bit_for_bit_counts_like_k11_and_waits_once(eng):
    name = (20000, 0.2)
    sk, rk, si, ri = _matches(name)[:4]
    with _Resident(eng, name) as dev:
        before = eng.lib.sf_sync_count()
        first = eng.fgr_device(dev.da, dev.db, dev.m, THR)
        assert eng.lib.sf_sync_count() - before == 1  # 4 + 2 x 64 launches, ONE host wait: no read-back between the iterations
        second = eng.fgr_device(dev.da, dev.db, dev.m, THR)
        for x, y in zip(first, second):
            assert np.array_equal(x, y)
        count = int(eng.ransac_refit_sums(dev.da, dev.db, dev.m, first[0], THR)[0])
    ratio, tf, rec = fast_global_registration(si, ri, sk, rk, distance_threshold=THR, seed=72, engine=eng)
    other = fast_global_registration(si, ri, sk, rk, distance_threshold=THR, seed=1, engine=eng)
    assert rec.inliers == count and ratio == count / dev.m
    assert count == F.inlier_count(dev.a, dev.b, first[0][:9].reshape(3, 3), first[0][9:], THR)
    assert other[0] == ratio and np.array_equal(other[1].rotation, tf.rotation) and np.array_equal(other[1].translation, tf.translation)
    assert np.array_equal(rec.trace, first[2]) and np.array_equal(other[2].trace, rec.trace)
    # (64 products of rotations leave R^T R - I at some tens of 2^-52: what normalize_rotation takes out)
    assert np.abs(tf.rotation - first[0][:9].reshape(3, 3)).max() <= 1e-13 and np.array_equal(tf.translation, first[0][9:])


# ---- 10. the tuple test ----------------------------------------------------------------------------------------------------------------
def test_tuple_selection_path(eng, sensitivity, monkeypatch):
    name = (20000, 0.5)
    sk, rk, si, ri, r0, t0 = _matches(name)
    a, b = N.matched_points(si, ri, sk, rk)
    seen = []
    real = eng.fgr_device

    def spy(da, db, m, thr, *args, sel=None, k=None, **kw):
        seen.append(sel.to_host()[:k])
        seen.append(real(da, db, m, thr, *args, sel=sel, k=k, **kw))
        return seen[-1]

    monkeypatch.setattr(eng, "fgr_device", spy, raising=False)
    ratio, tf, rec = fast_global_registration(si, ri, sk, rk, distance_threshold=THR, tuple_count=1000, engine=eng)
    want_sel = F.tuple_selection(a, b, 1000)
    assert rec.rows == 3000 and np.array_equal(seen[0], want_sel)
    want = F.fgr_rows(a[want_sel], b[want_sel], THR)
    rt = seen[1][0]  # (the device's transform before the returned rotation is re-normalised)
    d = _diff(rt[:9].reshape(3, 3), rt[9:], want["R"], want["t"])
    print(f"tuples: 3000 rows, device vs statement {d:.3e} (bound 10 x {sensitivity[1]:.3e}); |R - R0| = {np.linalg.norm(tf.rotation - r0):.2e}")
    assert d <= 10 * sensitivity[1]
    assert np.abs(tf.rotation - rt[:9].reshape(3, 3)).max() <= 1e-13 and np.array_equal(tf.translation, rt[9:])
    assert ratio == rec.inliers / a.shape[0] and abs(rec.inliers - F.inlier_count(a, b, want["R"], want["t"], THR)) <= 2


# ---- 12. it does what it is for ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACCURACY_SETS, ids=str)
def test_device_recovers_the_motion(eng, case):
    sk, rk, si, ri, r0, t0 = _matches(case)
    ratio, tf, rec = fast_global_registration(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    er, et = float(np.linalg.norm(tf.rotation - r0)), float(np.linalg.norm(tf.translation - t0))
    print(f"{case}: |R - R0| = {er:.2e}, |t - t0| = {et:.2e}, inlier ratio {ratio:.4f}")
    assert rec.status == "done" and rec.iterations == 64 and er <= CAP and et <= CAP
