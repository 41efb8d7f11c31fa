"""RANSAC with pre-rejection on the MI355X (K11, csrc/ransac.hip) against the NumPy statement of the definition
(tests/ransac_numpy.py: np.linalg.svd Kabsch, edge test, first maximum, refit loop).

The check is split where the definition leaves rounding to the implementation.  Status bytes are compared exactly outside a
1 +- 1e-9 band around the two thresholds; rotations under the perturbation bound of the polar factor, 64 x 2^-52 x s1 / gap;
everything after the hypotheses -- K9's counts, the compaction, the first maximum, the inlier masks of the refit -- exactly, on
the device's own transforms, where it is nothing but the bit-exact residual expression and integer bookkeeping."""
import os

import numpy as np
import pytest

import ransac_numpy as N
from conftest import load_golden
from shot_fpfh_amd.matching import ransac_on_matches, ransac_prerejective
from shot_fpfh_amd.matching.ransac import draw_stream

pytestmark = pytest.mark.gpu

EPS = 2.0**-52
THR = 0.01
SYNTH = [(5000, 0.5), (5000, 0.2), (5000, 0.1), (20000, 0.5), (20000, 0.2), (20000, 0.1)]
_cache = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _matches(name):
    """name -> (scan_kp, ref_kp, scan_idx, ref_idx, R0 or None, t0 or None)"""
    if name not in _cache:
        if name == "golden":
            g = load_golden("ransac_500.npz")
            _cache[name] = (g["scan_kp"], g["ref_kp"], g["scan_idx"], g["ref_idx"], None, None)
        elif name == "duplicates":  # reference rows heavily duplicated: 40 distinct reference keypoints for 4000 matches
            sk, rk, si, ri, r0, t0 = N.synthetic_matches(4000, 0.5, seed=11)
            _cache[name] = (sk, rk, si, ri[np.random.default_rng(3).integers(0, 40, 4000)], r0, t0)
        else:
            m, share = name
            _cache[name] = N.synthetic_matches(m, share, seed=m + int(100 * share))
    return _cache[name]


class _Device:
    """The matched points and one set of draws resident on the device, every output of sf_ransac_prerejective exported."""

    def __init__(self, eng, name, draw_size, sim, n_draws=10000, thr=THR, seed=72):
        sk, rk, si, ri = _matches(name)[:4]
        self.a, self.b = N.matched_points(si, ri, sk, rk)
        self.m = self.a.shape[0]
        self.draws = draw_stream(np.random.default_rng(seed), self.m, draw_size, n_draws)
        held = [eng.empty((self.m, 3)), eng.empty((self.m, 3)), eng.empty((n_draws, draw_size), np.int64),
                eng.empty((n_draws,), np.uint8), eng.empty((n_draws, 12)), eng.empty((n_draws,), np.int64),
                eng.empty((n_draws,), np.int64)]
        try:
            da, db, dd, dst, drt, dmap, dcnt = held
            da.from_host(self.a), db.from_host(self.b), dd.from_host(self.draws)
            self.result, self.best = eng.ransac_prerejective_device(da, db, self.m, dd, n_draws, draw_size, sim, thr, status=dst,
                                                                    rt=drt, slot_draw=dmap, counts=dcnt)
            ns = int(self.result[2])
            self.status = dst.to_host()
            self.rt, self.slot_draw, self.counts = drt.to_host()[:ns], dmap.to_host()[:ns], dcnt.to_host()[:ns]
        finally:
            for h in held:
                h.free()


def _need_survivors(dev):
    assert int(dev.result[2]) >= 20, f"only {int(dev.result[2])} status-0 draws: the comparison would be empty"


# ---- 1. edge test and status ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYNTH + ["golden", "duplicates"], ids=str)
def test_status_bytes_equal_numpy_outside_the_band(eng, name):
    for draw_size in (3, 4, 8):
        for sim in (0.0, 0.5, 0.9):
            dev = _Device(eng, name, draw_size, sim)
            status, _, near, _, _ = N.hypotheses(dev.a, dev.b, dev.draws, sim)
            differ = dev.status != status
            print(f"{name} k={draw_size} sim={sim}: scored {int((status == 0).sum())}, rejected {int((status == 1).sum())}, "
                  f"degenerate {int((status == 2).sum())}; in the band {int(near.sum())}, differing {int(differ.sum())}")
            assert near.sum() <= 1e-3 * status.size
            assert not (differ & ~near).any(), np.flatnonzero(differ & ~near)[:10]
            assert not (dev.status == 3).any()
            assert (int(dev.result[0]), int(dev.result[1]), int(dev.result[2])) == tuple(int((dev.status == v).sum()) for v in (1, 2, 0))


# ---- 2. hypotheses ------------------------------------------------------------------------------------------------------------------
HYP_CASES = [((5000, 0.5), 3, 0.9), ((20000, 0.2), 3, 0.9), ((20000, 0.1), 3, 0.9), ((5000, 0.5), 3, 0.0), ((5000, 0.2), 4, 0.0),
             ((20000, 0.5), 8, 0.0), ((5000, 0.5), 4, 0.5), ((20000, 0.5), 8, 0.5), ("golden", 4, 0.0), ("golden", 3, 0.5),
             ("duplicates", 3, 0.5), ("duplicates", 4, 0.0)]
_worst = {}


@pytest.mark.parametrize("name,draw_size,sim", HYP_CASES, ids=str)
def test_rotations_orthonormal_and_within_the_polar_factor_bound(eng, name, draw_size, sim):
    dev = _Device(eng, name, draw_size, sim)
    _need_survivors(dev)
    status, rt, near, cond, anorm = N.hypotheses(dev.a, dev.b, dev.draws, sim)
    both = np.flatnonzero((dev.status == 0) & (status == 0))
    assert both.size >= 20
    slot = np.searchsorted(dev.slot_draw, both)
    assert np.array_equal(dev.slot_draw[slot], both)
    r = dev.rt[slot, :9].reshape(-1, 3, 3)
    assert np.isfinite(dev.rt).all()
    orth = np.abs(np.matmul(r.transpose(0, 2, 1), r) - np.eye(3)).max(axis=(1, 2))
    assert orth.max() <= 8 * EPS, orth.max() / EPS
    assert np.all(np.linalg.det(r) > 0.5)
    unit = EPS * cond[both]
    mult_r = np.abs(r - rt[both, :9].reshape(-1, 3, 3)).max(axis=(1, 2)) / unit
    mult_t = np.abs(dev.rt[slot, 9:] - rt[both, 9:]).max(axis=1) / (unit * (1 + anorm[both]))
    _worst[(str(name), draw_size, sim)] = (both.size, float(mult_r.max()), float(mult_t.max()), float(orth.max() / EPS))
    print(f"{name} k={draw_size} sim={sim}: {both.size} draws, worst |R - R_numpy| = {mult_r.max():.2f}, worst |t - t_numpy| = "
          f"{mult_t.max():.2f} x 2^-52 s1/gap (x (1 + |abar|) for t); R^T R - I <= {orth.max() / EPS:.1f} x 2^-52")
    assert mult_r.max() <= 64, (mult_r.max(), cond[both][np.argmax(mult_r)])
    assert mult_t.max() <= 64, (mult_t.max(), cond[both][np.argmax(mult_t)])


# ---- 3. everything after the hypotheses is exact on the device's own Rt ---------------------------------------------------------------
@pytest.mark.parametrize("name,draw_size,sim,n_draws", [((5000, 0.5), 3, 0.9, 10000), ((20000, 0.2), 3, 0.9, 10000),
                                                        ((5000, 0.2), 4, 0.0, 3000), ("golden", 4, 0.0, 9000),
                                                        ("duplicates", 3, 0.5, 10000), ((5000, 0.5), 3, 0.0, 20000)], ids=str)
def test_counts_winner_and_compaction_are_exact(eng, name, draw_size, sim, n_draws):
    dev = _Device(eng, name, draw_size, sim, n_draws=n_draws)
    _need_survivors(dev)
    rej, deg, ns = (int(dev.result[i]) for i in range(3))
    assert ns + rej + deg == n_draws
    assert np.array_equal(dev.slot_draw, np.flatnonzero(dev.status == 0))  # nothing lost, nothing reordered
    assert np.all(np.diff(dev.slot_draw) > 0)
    check = np.unique(np.concatenate([np.arange(min(ns, 60)), np.linspace(0, ns - 1, 120).astype(int), [int(dev.result[5])]]))
    assert np.array_equal(dev.counts[check], N.score(dev.a, dev.b, dev.rt[check], THR))
    w = N.first_max(dev.counts)
    assert (int(dev.result[5]), int(dev.result[3]), int(dev.result[4])) == (w, int(dev.slot_draw[w]), int(dev.counts[w]))
    assert np.array_equal(dev.best, dev.rt[w])


# ---- 4. refit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [(5000, 0.5), (20000, 0.1), "duplicates"], ids=str)
def test_refit_sums_masks_and_decisions(eng, name):
    sk, rk, si, ri = _matches(name)[:4]
    a, b = N.matched_points(si, ri, sk, rk)
    m = a.shape[0]
    dev = _Device(eng, name, 3, 0.9 if name != "duplicates" else 0.5)
    _need_survivors(dev)
    da, db = eng.empty((m, 3)), eng.empty((m, 3))
    try:
        da.from_host(a), db.from_host(b)
        rt, count, kept = dev.best.copy(), int(dev.result[4]), []
        for it in range(3):
            sums = eng.ransac_refit_sums(da, db, m, rt, THR)
            assert np.array_equal(sums, eng.ransac_refit_sums(da, db, m, rt, THR))  # two runs, bit for bit
            mask = N.inlier_mask(a, b, rt, THR)
            want = N.refit_sums(a, b, mask)
            assert int(sums[0]) == want["count"] == count
            tol = m * EPS
            assert np.all(np.abs(sums[17:20] - want["sum_a"]) <= tol * want["sum_a_abs"])
            assert np.all(np.abs(sums[20:23] - want["sum_b"]) <= tol * want["sum_b_abs"])
            assert np.all(np.abs(sums[1:4] - want["abar"]) <= tol * want["sum_a_abs"] / max(count, 1))
            assert np.all(np.abs(sums[4:7] - want["bbar"]) <= tol * want["sum_b_abs"] / max(count, 1))
            assert np.all(np.abs(sums[7:16].reshape(3, 3) - want["h"]) <= tol * want["h_abs"])
            res2 = N.residual_norms(a, b, rt)[mask] ** 2
            assert abs(sums[16] - float(np.sum(res2))) <= tol * float(np.sum(res2))
            if count < 3:  # (non-congruent triangles fit nobody: the duplicated set's winner may have fewer inliers than points)
                break
            new = N.fit_from_sums(sums[7:16].reshape(3, 3), sums[1:4], sums[4:7])
            new_count = int(np.count_nonzero(N.inlier_mask(a, b, new, THR)))
            if new_count < count:
                break
            rt, unchanged, count = new, new_count == count, new_count
            kept.append(new_count)
            if unchanged:
                break
        # the public call takes the same decisions: kept while the count does not drop, stopped when it stops changing
        ratio, tf, rec = ransac_prerejective(si, ri, sk, rk, n_draws=10000, draw_size=3, distance_threshold=THR,
                                             edge_similarity=0.9 if name != "duplicates" else 0.5, refit_iterations=3, engine=eng)
        assert rec.winner_draw == int(dev.result[3]) and rec.winner_inliers == int(dev.result[4])
        assert rec.refit_inliers == kept, (rec.refit_inliers, kept)
        assert all(x >= y for x, y in zip(rec.refit_inliers, [rec.winner_inliers] + rec.refit_inliers))
        assert ratio == (kept[-1] if kept else rec.winner_inliers) / m
        again = ransac_prerejective(si, ri, sk, rk, n_draws=10000, draw_size=3, distance_threshold=THR,
                                    edge_similarity=0.9 if name != "duplicates" else 0.5, refit_iterations=3, engine=eng)
        assert again[0] == ratio and np.array_equal(again[1].rotation, tf.rotation) and np.array_equal(again[1].translation, tf.translation)
        assert again[2] == rec
    finally:
        da.free(), db.free()


# ---- 5. it does what it is for -------------------------------------------------------------------------------------------------------
_ratios = {}


@pytest.mark.parametrize("name", SYNTH, ids=str)
def test_refit_brings_the_transform_closer_to_the_truth(eng, name):
    import shot_fpfh_amd.matching.ransac as R

    sk, rk, si, ri, r0, t0 = _matches(name)

    def err(rot, tr):
        return float(np.linalg.norm(rot - r0)), float(np.linalg.norm(tr - t0))

    kw = dict(n_draws=10000, draw_size=3, distance_threshold=THR, edge_similarity=0.9, seed=72)
    _, tf2, rec2 = ransac_prerejective(si, ri, sk, rk, refit_iterations=2, engine=eng, **kw)
    _, tf0, rec0 = ransac_prerejective(si, ri, sk, rk, refit_iterations=0, engine=eng, **kw)
    assert rec2.n_scored >= 20
    R.rng = np.random.default_rng(seed=72)
    _, tfr = ransac_on_matches(si, ri, sk, rk, n_draws=10000, draw_size=4, distance_threshold=THR, disable_progress_bar=True, engine=eng)
    _, rn, tn, recn = N.ransac_prerejective(si, ri, sk, rk, refit_iterations=2, **kw)
    e2, e0, er, en = err(tf2.rotation, tf2.translation), err(tf0.rotation, tf0.translation), err(tfr.rotation, tfr.translation), err(rn, tn)
    _ratios[str(name)] = (rec2.n_scored, rec2.winner_draw, recn["winner_draw"], e0, e2, er, en)
    print(f"{name}: scored {rec2.n_scored}, winner {rec2.winner_draw} (NumPy {recn['winner_draw']}); |R - R0|, |t - t0|: no refit "
          f"{e0[0]:.2e} {e0[1]:.2e}, refit {e2[0]:.2e} {e2[1]:.2e} ({e0[0] / e2[0]:.1f}x, {e0[1] / e2[1]:.1f}x), "
          f"ransac_on_matches {er[0]:.2e} {er[1]:.2e}, NumPy {en[0]:.2e} {en[1]:.2e}")
    for k in (0, 1):
        assert e2[k] < e0[k]
        assert e2[k] < er[k]
        assert e2[k] <= 1.5 * en[k]


def test_write_parity_record():
    """Writes what the tests above measured to SF_RANSAC_PARITY_OUT (a markdown file) when that is set; asserts nothing new."""
    out = os.environ.get("SF_RANSAC_PARITY_OUT")
    if not out or not (_worst or _ratios):
        return
    with open(out, "w") as f:
        f.write("| case | draw size | similarity | draws compared | worst R multiple | worst t multiple | R^T R - I (x 2^-52) |\n|---|---|---|---|---|---|---|\n")
        for (name, k, sim), (n, mr, mt, orth) in _worst.items():
            f.write(f"| {name} | {k} | {sim} | {n} | {mr:.2f} | {mt:.2f} | {orth:.1f} |\n")
        f.write("\n| case | scored | winner (NumPy) | no refit dR, dt | refit dR, dt | ratio dR, dt | ransac_on_matches dR, dt | NumPy dR, dt |\n|---|---|---|---|---|---|---|---|\n")
        for name, (ns, w, wn, e0, e2, er, en) in _ratios.items():
            f.write(f"| {name} | {ns} | {w} ({wn}) | {e0[0]:.2e}, {e0[1]:.2e} | {e2[0]:.2e}, {e2[1]:.2e} | {e0[0] / e2[0]:.1f}x, {e0[1] / e2[1]:.1f}x | "
                    f"{er[0]:.2e}, {er[1]:.2e} | {en[0]:.2e}, {en[1]:.2e} |\n")


# ---- 6. corners ----------------------------------------------------------------------------------------------------------------------
def test_corners(eng):
    sk, rk, si, ri = _matches((5000, 0.5))[:4]
    kw = dict(distance_threshold=THR, engine=eng)
    with pytest.raises(ValueError):
        ransac_prerejective(si[:0], ri[:0], sk, rk, **kw)  # m = 0
    with pytest.raises(ValueError):
        ransac_prerejective(si[:3], ri[:3], sk, rk, draw_size=4, **kw)  # m < draw_size
    with pytest.raises(ValueError):
        ransac_prerejective(si, ri, sk, rk, n_draws=0, **kw)
    # all draws rejected: an 8-point draw at similarity 0.9 among 10 % true matches practically never survives
    sk1, rk1, si1, ri1 = _matches((20000, 0.1))[:4]
    with pytest.raises(ValueError, match="rejected"):
        ransac_prerejective(si1, ri1, sk1, rk1, n_draws=2000, draw_size=8, **kw)
    # all-identical points at similarity 0: every draw passes the edge test, every H is 0 -> all degenerate, no NaN anywhere
    one = np.full((50, 3), 0.25)
    idx = np.arange(50)
    dev_kw = dict(n_draws=500, draw_size=3, edge_similarity=0.0)
    with pytest.raises(ValueError, match="500 degenerate"):
        ransac_prerejective(idx, idx, one, one, **dev_kw, **kw)
    da, db, dd, dst, drt = eng.empty((50, 3)), eng.empty((50, 3)), eng.empty((500, 3), np.int64), eng.empty((500,), np.uint8), eng.empty((500, 12))
    try:
        da.from_host(one), db.from_host(one)
        dd.from_host(draw_stream(np.random.default_rng(72), 50, 3, 500))
        eng.ransac_hypotheses_device(da, db, 50, dd, 500, 3, 0.0, dst, drt)
        assert (dst.to_host() == 2).all() and not drt.to_host().any()
    finally:
        for h in (da, db, dd, dst, drt):
            h.free()
    # thresholds 0, inf, NaN behave as K9's do: 0 admits exact fits only, inf everything, NaN nothing
    a, b = N.matched_points(si, ri, sk, rk)
    for thr, want in ((np.inf, 5000), (np.nan, 0)):
        dev = _Device(eng, (5000, 0.5), 3, 0.9, n_draws=2000, thr=thr)
        assert np.all(dev.counts == want) and int(dev.result[5]) == 0 and int(dev.result[3]) == int(dev.slot_draw[0])
    dev = _Device(eng, (5000, 0.5), 3, 0.9, n_draws=2000, thr=0.0)
    assert np.array_equal(dev.counts, N.score(a, b, dev.rt, 0.0))
    ratio, tf, rec = ransac_prerejective(si, ri, sk, rk, n_draws=2000, distance_threshold=np.nan, engine=eng)
    assert ratio == 0.0 and rec.refit_inliers == [] and np.isfinite(tf.rotation).all()


def test_more_draws_than_one_workgroup_scores(eng):
    """n_draws above 8 192: K9 splits the survivors over workgroups and the compaction crosses its blocks."""
    name = (5000, 0.5)
    dev = _Device(eng, name, 3, 0.0, n_draws=20000)  # similarity 0: nearly all 20 000 survive
    assert int(dev.result[2]) > 8192
    assert np.array_equal(dev.slot_draw, np.flatnonzero(dev.status == 0))
    check = np.r_[0:40, 8150:8230, int(dev.result[2]) - 40:int(dev.result[2])]
    assert np.array_equal(dev.counts[check], N.score(dev.a, dev.b, dev.rt[check], THR))
    w = N.first_max(dev.counts)
    assert (int(dev.result[5]), int(dev.result[3])) == (w, int(dev.slot_draw[w]))
