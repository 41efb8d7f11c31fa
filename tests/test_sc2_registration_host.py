"""Host side of sc2_registration: the NumPy statement of the definition (tests/sc2_registration_numpy.py) on small hand-made
sets and on the set the estimator exists for, and the public call's results, arguments, caps, exports, pipeline method and
command-line flags -- on a stand-in engine that answers the K15 call from the statement."""
import importlib
import inspect
import os
import sys

import numpy as np
import pytest

import consistency_numpy as C
import ransac_numpy as N
import sc2_numpy as S
import sc2_registration_numpy as R
from fake_engine import FakeArray, FakeEngine

import shot_fpfh_amd
import shot_fpfh_amd.matching as matching
from shot_fpfh_amd import _ffi

G = importlib.import_module("shot_fpfh_amd.matching.sc2_registration")  # (the package attribute of that name is the function)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.01


# ---- 1. the statement on small hand-made sets ---------------------------------------------------------------------------------------
def _two_cliques():
    """Nine matches that keep every length but are a MIRROR image (no rotation fits them), then six under one translation, on the
    2^-3 lattice so that every length is exact.  The mirrored ones are the larger clique and have the larger s2."""
    rng = np.random.default_rng(5)
    cells = rng.permutation(8 ** 3)[:15]
    a = np.stack([cells % 8, (cells // 8) % 8, cells // 64], axis=1) / 8.0
    a[9:] += [40.0, 0.0, 0.0]
    b = a.copy()
    b[:9, 2] *= -1.0
    b[:9] += [0.0, 7.0, 0.0]
    b[9:] += [0.25, -0.5, 3.0]
    return a, b


def test_a_seed_that_is_not_the_first_maximum_of_s2_wins():
    a, b = _two_cliques()
    idx = np.arange(15)
    cmat = S.compat_matrix(a, b, THR)
    assert cmat[:9, :9].sum() == 72 and cmat[9:, 9:].sum() == 30 and not cmat[:9, 9:].any()  # two cliques, nothing across
    group = S.group(a, b, THR)
    assert group["seed"] == 0 and list(group["keep"]) == list(range(9))  # the filter keeps the mirrored ones
    ratio, rot, t, rec = R.sc2_registration(idx, idx, a, b, THR, n_seeds=15)
    assert list(rec["second_degree"]) == [56] * 9 + [20] * 6 and list(rec["seeds"]) == list(range(15))
    assert list(rec["size"]) == [9] * 9 + [6] * 6 and not rec["seed_status"].any()
    assert list(rec["counts"][9:]) == [6] * 6 and rec["counts"][:9].max() < 6  # a rotation fits few of a mirror image
    assert (rec["winner_rank"], rec["winner_seed"], rec["winner_size"], rec["winner_inliers"]) == (9, 9, 6, 6)
    assert ratio == 6 / 15 and np.abs(rot - np.eye(3)).max() < 1e-12 and np.abs(t - [0.25, -0.5, 3.0]).max() < 1e-12
    # with the seeds cut off in front of the second clique the first one is all there is
    assert R.sc2_registration(idx, idx, a, b, THR, n_seeds=9)[3]["winner_rank"] < 9


def test_ties_pick_the_lower_position():
    a, b, thr, edge = C.tie_set(40, seed=2)  # rows 5 .. 39: one clique, all scores equal
    idx = np.arange(40)
    ratio, rot, t, rec = R.sc2_registration(idx, idx, a, b, thr, edge, n_seeds=8)
    assert list(rec["seeds"]) == list(range(5, 13)) and (rec["size"] == 35).all() and (rec["counts"] == 35).all()
    assert (rec["winner_rank"], rec["winner_seed"]) == (0, 5) and ratio == 35 / 40
    for s in range(8):
        assert int(rec["rows"][s].sum()) == int(rec["second_degree"][rec["seeds"][s]]) == 34 * 33


def test_a_nan_row_is_never_a_seed_or_a_member():
    sk, rk, si, ri, _, _ = N.synthetic_matches(40, 0.5, sigma=0.002, seed=9)
    a, b = N.matched_points(si, ri, sk, rk)
    a = a.copy()
    a[5, 1] = np.nan
    hyp = R.hypotheses(a, b, THR, n_seeds=40)
    assert hyp["second_degree"][5] == 0 and 5 not in hyp["seeds"] and not hyp["member"][:, 5].any()
    assert hyp["n_found"] >= 10 and (hyp["seeds"][hyp["n_found"]:] == -1).all() and (hyp["status"][hyp["n_found"]:] == 3).all()
    assert np.isfinite(hyp["rt"]).all()


def test_a_collinear_consensus_set_is_degenerate_and_nothing_is_scored():
    a, b, thr, edge = C.lattice_set(40, seed=1)  # every point on one axis
    idx = np.arange(40)
    ratio, rot, t, rec = R.sc2_registration(idx, idx, a, b, thr, edge, n_seeds=16)
    assert rec["n_found"] == 16 and (rec["seed_status"] == 2).all() and (rec["size"] >= 3).all() and not rec["rt"].any()
    assert (ratio, rot, t, rec["status"], rec["winner_seed"]) == (0.0, None, None, R.STATUS_NO_FIT, -1)


def test_fewer_than_three_members_and_the_other_corners():
    # 0 - 1 share four neighbours (2 .. 5) that share nothing else: row_0 = [0, 4, 1, 1, 1, 1], at share 0.5 only match 1 stays
    cmat = np.zeros((6, 6), dtype=np.uint8)
    cmat[0, 1:] = cmat[1, 2:] = 1
    cmat = cmat + cmat.T
    rows = R.seed_rows(cmat, [0, 2, -1])
    assert rows.tolist() == [[0, 4, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0], [0] * 6]
    s2 = S.second_order(cmat)[0]
    assert list(s2) == [8, 8, 2, 2, 2, 2] and list(R.seeds_of(s2, 8)) == [0, 1, 2, 3, 4, 5, -1, -1]
    mask = R.members_of(rows[0], 0, 0.5)
    assert list(np.flatnonzero(mask)) == [0, 1]
    pts = np.random.default_rng(1).random((6, 3))
    assert R.fit_members(pts, pts + 1.0, mask)[0] == 1                                  # two members: status 1
    assert list(np.flatnonzero(R.members_of(rows[0], 0, 0.25))) == [0, 1, 2, 3, 4, 5]   # a looser share takes them all
    status, rt, _, cond = R.fit_members(pts, pts + 1.0, R.members_of(rows[0], 0, 0.25))
    assert status == 0 and np.abs(rt - np.concatenate([np.eye(3).reshape(9), np.ones(3)])).max() < 1e-12 and cond < 100
    # not symmetric: rows of C against rows of C, weighted by the seed's own row
    c = (np.random.default_rng(3).random((23, 23)) < 0.5).astype(np.uint8)
    want = [[int(c[s, j]) * sum(int(c[s, k]) * int(c[j, k]) for k in range(23)) for j in range(23)] for s in (4, 22, 4)]
    assert R.seed_rows(c, [4, 22, 4]).tolist() == want
    idx = np.arange(2)
    assert R.sc2_registration(idx, idx, pts, pts, THR)[3]["status"] == R.STATUS_TOO_FEW
    far = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    moved = far.copy()
    moved[2:] += [0.0, 5.0, 0.0]
    assert R.sc2_registration(np.arange(4), np.arange(4), far, moved, THR)[3]["status"] == R.STATUS_NO_TRIPLE


# ---- 2. the statement on the set the estimator exists for -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def thin():
    """(5000, 0.004, 1): 15 true matches in 5000."""
    m, share, seed = 5000, 0.004, 1
    sk, rk, si, ri, r0, t0 = N.synthetic_matches(m, share, seed=seed)
    true, replayed = C.synthetic_truth(m, share, seed)
    assert np.array_equal(replayed, sk)
    return sk, rk, si, ri, r0, t0, true


def test_statement_recovers_the_true_matches_where_the_single_seed_is_false(thin):
    sk, rk, si, ri, r0, t0, true = thin
    a, b = N.matched_points(si, ri, sk, rk)
    ratio, rot, t, rec = R.sc2_registration(si, ri, sk, rk, THR, n_seeds=64)
    group = S.group(a, b, THR)
    assert np.array_equal(group["second_degree"], rec["second_degree"]) and group["seed"] == rec["seeds"][0]
    assert group["seed"] not in true and np.intersect1d(group["keep"], true).size == 0 and group["keep"].size == 53
    near_truth = np.flatnonzero(N.inlier_mask(a, b, np.concatenate([r0.reshape(9), t0]), THR))
    inliers = np.flatnonzero(N.inlier_mask(a, b, np.concatenate([rot.reshape(9), t]), THR))
    print(f"{true.size} true, {near_truth.size} within the threshold of (R0, t0); winner: rank {rec['winner_rank']}, seed "
          f"{rec['winner_seed']}, consensus {rec['winner_size']}, inliers {rec['winner_inliers']} -> {rec['refit_inliers']}, "
          f"|R - R0| = {np.linalg.norm(rot - r0):.2e}")
    assert np.array_equal(inliers, near_truth) and np.array_equal(inliers, true) and true.size == 15
    assert ratio == 15 / 5000 and rec["winner_rank"] > 0 and rec["winner_seed"] in true
    assert np.linalg.norm(rot - r0) <= 2e-3
    # one seed is the filter's seed: nothing true
    one = R.sc2_registration(si, ri, sk, rk, THR, n_seeds=1)
    assert one[3]["winner_seed"] == group["seed"] and one[0] * 5000 < 3


# ---- 3. the public call on a stand-in engine ------------------------------------------------------------------------------------------
class _Tracked(FakeArray):
    live = 0

    def __init__(self, shape, dtype=np.float64):
        super().__init__(shape, dtype)
        _Tracked.live += 1
        self.freed = False

    def free(self):
        if not self.freed:
            self.freed = True
            _Tracked.live -= 1


class _Engine(FakeEngine):
    """FakeEngine + the two calls sc2_registration makes, answered by the NumPy statements."""

    SC2_MAX_SEEDS = R.MAX_SEEDS

    def __init__(self, fail=None):
        self.fail, self.calls, self.refits = fail, [], 0

    def empty(self, shape, dtype=np.float64):
        if self.fail == "empty" and np.dtype(dtype) == np.uint8:
            raise MemoryError("no room for the status bytes")
        return _Tracked(shape, dtype)

    def sc2_registration_device(self, a, b, m, thr, edge, n_seeds, share, *, s2, seeds, status, size, slot_seed, counts, rt=None):
        if self.fail == "chain":
            raise RuntimeError("device call failed")
        self.calls.append((m, thr, edge, n_seeds, share))
        hyp = R.hypotheses(a.a[:m], b.a[:m], thr, edge, n_seeds, share)
        s2.a[:m], seeds.a[:], status.a[:], size.a[:] = hyp["second_degree"], hyp["seeds"], hyp["status"], hyp["size"]
        slots = np.flatnonzero(hyp["status"] == 0)
        slot_seed.a[:], counts.a[:] = -1, -1
        slot_seed.a[:slots.size] = slots
        counts.a[:slots.size] = N.score(a.a[:m], b.a[:m], hyp["rt"][slots], thr)
        result, best = np.array([hyp["n_found"], (hyp["status"] == 1).sum(), (hyp["status"] == 2).sum(), slots.size, -1, 0, -1, 0],
                                dtype=np.int64), np.zeros(12)
        if slots.size:
            w = N.first_max(counts.a[:slots.size])
            rank = int(slots[w])
            result[4:], best = [hyp["seeds"][rank], counts.a[w], rank, hyp["size"][rank]], hyp["rt"][rank].copy()
        return result, best

    def ransac_refit_sums(self, a, b, m, rt, thr):
        self.refits += 1
        s = N.refit_sums(a.a[:m], b.a[:m], N.inlier_mask(a.a[:m], b.a[:m], np.asarray(rt), thr))
        out = np.zeros(24)
        out[0], out[1:4], out[4:7], out[7:16], out[17:20], out[20:23] = s["count"], s["abar"], s["bbar"], s["h"].reshape(9), s["sum_a"], s["sum_b"]
        return out


@pytest.fixture(scope="module")
def matches():
    return N.synthetic_matches(600, 0.1, seed=5)


def test_exports_signature_and_abi_table():
    assert shot_fpfh_amd.sc2_registration is G.sc2_registration is matching.sc2_registration
    assert shot_fpfh_amd.Sc2RegistrationRecord is matching.Sc2RegistrationRecord is G.Sc2RegistrationRecord
    for name in ("sc2_registration", "Sc2RegistrationRecord"):
        assert name in shot_fpfh_amd.__all__ and name in matching.__all__ and name in G.__all__
    assert G.SC2_MAX_SEEDS == shot_fpfh_amd.Engine.SC2_MAX_SEEDS == R.MAX_SEEDS == 1024
    assert shot_fpfh_amd.Engine.SC2_SEED_TILE == R.SEED_TILE == 64 and G.SC2_MAX_MATCHES == S.MAX_MATCHES
    p = inspect.signature(G.sc2_registration).parameters
    names = list(p)
    assert names == ["scan_descriptors_indices", "ref_descriptors_indices", "scan_keypoints", "ref_keypoints", "distance_threshold",
                     "min_edge", "n_seeds", "group_share", "refit_iterations", "verbose", "engine"]
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:4])
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[4:])
    assert p["distance_threshold"].default is inspect.Parameter.empty
    assert tuple(p[n].default for n in names[5:]) == (None, 256, 0.5, 2, False, None)
    assert {"status", "seeds", "seed_status", "seed_size", "seed_inliers", "winner_seed", "winner_size", "winner_inliers",
            "refit_inliers", "second_degree"} <= set(G.Sc2RegistrationRecord.__dataclass_fields__)
    header = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name, n_args in (("sf_sc2_seeds", 5), ("sf_sc2_seed_rows", 6), ("sf_sc2_seed_fits", 13), ("sf_sc2_registration", 17)):
        assert name in _ffi.SIGNATURES and f"int {name}(" in header and len(_ffi.SIGNATURES[name][1]) == n_args
    assert "#define SF_SC2_MAX_SEEDS 1024" in header and f"#define SF_SC2_SEED_TILE {R.SEED_TILE}" in header
    for method in ("sc2_seeds_device", "sc2_seed_rows_device", "sc2_seed_fits_device", "sc2_registration_device"):
        assert callable(getattr(shot_fpfh_amd.Engine, method))
    source = open(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "consistency.hip")).read()
    assert "k15_seed_rows" in source and "k15_seeds" in source and "k15_fit" in source
    assert source.count("__builtin_amdgcn_mfma_i32_32x32x32_i8") >= 2 and "sf_horn::kabsch_rotation" in source
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "sf_sc2_registration" in text and "K15" in text, doc
    # the estimators that were there keep their shape
    assert inspect.signature(matching.ransac_prerejective).parameters["refit_iterations"].default == 2
    assert inspect.signature(matching.second_order_consistency_filter).parameters["group_share"].default == 0.5


@pytest.mark.parametrize("kw", [dict(distance_threshold=-1e-3), dict(distance_threshold=float("nan")), dict(distance_threshold=float("inf")),
                                dict(min_edge=-1.0), dict(min_edge=float("nan")), dict(min_edge=float("inf")), dict(group_share=0.0),
                                dict(group_share=1.5), dict(group_share=float("nan")), dict(n_seeds=0), dict(n_seeds=-4),
                                dict(n_seeds=R.MAX_SEEDS + 1), dict(refit_iterations=-1)])
def test_bad_arguments_raise_before_any_device_work(matches, kw):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    eng = _Engine()
    with pytest.raises(ValueError):
        G.sc2_registration(si, ri, sk, rk, **{"distance_threshold": THR, "engine": eng, **kw})
    assert _Tracked.live == before and not eng.calls
    with pytest.raises(TypeError):
        G.sc2_registration(si, ri, sk, rk, THR, engine=eng)  # the threshold is keyword-only
    with pytest.raises(ValueError):
        G.sc2_registration(si, ri[:-1], sk, rk, distance_threshold=THR, engine=eng)


def test_caps_and_too_few_matches_are_refused_before_any_device_work(matches):
    sk, rk, si, ri = matches[:4]
    eng = _Engine()
    before = _Tracked.live
    idx = np.zeros(G.SC2_MAX_MATCHES + 1, dtype=np.int64)
    with pytest.raises(ValueError, match="ratio_test_matching|geometric_consistency_filter") as err:
        G.sc2_registration(idx, idx, sk, rk, distance_threshold=THR, engine=eng)
    assert "32768" in str(err.value)
    for n in (0, 1, 2):
        with pytest.raises(ValueError, match="fewer than three matches"):
            G.sc2_registration(si[:n], ri[:n], sk, rk, distance_threshold=THR, engine=eng)
    assert _Tracked.live == before and not eng.calls


def test_result_follows_the_numpy_statement(matches):
    sk, rk, si, ri, r0, t0 = matches
    eng = _Engine()
    ratio, tf, rec = G.sc2_registration(si, ri, sk, rk, distance_threshold=THR, n_seeds=32, engine=eng)
    want_ratio, want_r, want_t, want = R.sc2_registration(si, ri, sk, rk, THR, n_seeds=32)
    assert eng.calls == [(600, THR, THR, 32, 0.5)]  # min_edge defaults to the threshold
    assert ratio == want_ratio and isinstance(tf, shot_fpfh_amd.core.RigidTransform)
    assert np.abs(tf.rotation - want_r).max() < 1e-12 and np.abs(tf.translation - want_t).max() < 1e-12
    assert np.abs(tf.rotation.T @ tf.rotation - np.eye(3)).max() < 1e-14 and np.linalg.norm(tf.rotation - r0) < 2e-3
    assert (rec.status, rec.winner_seed, rec.winner_rank, rec.winner_size, rec.winner_inliers, rec.refit_inliers) == (
        "done", want["winner_seed"], want["winner_rank"], want["winner_size"], want["winner_inliers"], want["refit_inliers"])
    assert np.array_equal(rec.seeds, want["seeds"]) and rec.seeds.dtype == np.int64
    assert np.array_equal(rec.seed_status, want["seed_status"]) and np.array_equal(rec.seed_size, want["size"])
    assert np.array_equal(rec.second_degree, want["second_degree"]) and rec.second_degree.dtype == np.uint32
    assert np.array_equal(rec.seed_inliers[want["slot_seed"]], want["counts"])
    assert (rec.n_scored, rec.n_too_small, rec.n_degenerate) == (want["slot_seed"].size, 0, 0)
    assert set(np.flatnonzero(N.inlier_mask(*N.matched_points(si, ri, sk, rk), np.concatenate([want_r.reshape(9), want_t]), THR))) >= set(
        C.synthetic_truth(600, 0.1, 5)[0][:5])
    # the arguments reach the engine; no refit: the winner as it was fitted
    G.sc2_registration(si, ri, sk, rk, distance_threshold=THR, min_edge=0.05, n_seeds=7, group_share=0.9, engine=eng)
    assert eng.calls[-1] == (600, THR, 0.05, 7, 0.9)
    refits = eng.refits
    plain = G.sc2_registration(si, ri, sk, rk, distance_threshold=THR, n_seeds=32, refit_iterations=0, engine=eng)
    assert eng.refits == refits and plain[2].refit_inliers == [] and plain[0] == want["winner_inliers"] / 600


def test_nothing_scored_raises_as_ransac_prerejective_does(matches):
    a, b, thr, edge = C.lattice_set(40, seed=1)
    idx = np.arange(40)
    before = _Tracked.live
    with pytest.raises(ValueError, match="no seed gave a fit"):
        G.sc2_registration(idx, idx, a, b, distance_threshold=thr, min_edge=edge, n_seeds=16, engine=_Engine())
    far = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    moved = far.copy()
    moved[2:] += [0.0, 5.0, 0.0]
    with pytest.raises(ValueError, match="no consistent triple"):
        G.sc2_registration(np.arange(4), np.arange(4), far, moved, distance_threshold=THR, engine=_Engine())
    assert _Tracked.live == before


@pytest.mark.parametrize("fail", ["empty", "chain", "index"])
def test_device_buffers_are_freed_on_every_error_path(matches, fail):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    if fail == "index":
        with pytest.raises(IndexError):
            G.sc2_registration(si + 600, ri, sk, rk, distance_threshold=THR, engine=_Engine())
    else:
        with pytest.raises((MemoryError, RuntimeError)):
            G.sc2_registration(si, ri, sk, rk, distance_threshold=THR, engine=_Engine(fail))
    assert _Tracked.live == before
    G.sc2_registration(si, ri, sk, rk, distance_threshold=THR, n_seeds=4, engine=_Engine())
    assert _Tracked.live == before


def test_the_refit_helper_is_the_one_ransac_prerejective_uses():
    import shot_fpfh_amd.matching.ransac as ransac

    assert G._refit_over_inliers is ransac._refit_over_inliers
    assert "_refit_over_inliers(" in inspect.getsource(ransac.ransac_prerejective)


# ---- 4. pipeline and command line ---------------------------------------------------------------------------------------------------
def test_run_ransac_reaches_the_call(monkeypatch):
    import shot_fpfh_amd.pipeline as P

    calls = []

    def fake(*args, **kw):
        calls.append((args, kw))
        return 0.25, shot_fpfh_amd.core.RigidTransform(), G.Sc2RegistrationRecord(n_scored=3)

    monkeypatch.setattr(P, "sc2_registration", fake)
    pipe = P.RegistrationPipeline.__new__(P.RegistrationPipeline)
    pipe.scan, pipe.ref = np.zeros((4, 3)), np.ones((4, 3))
    pipe.scan_keypoints = pipe.ref_keypoints = np.arange(4)
    pipe.matches = (np.arange(4), np.arange(4)[::-1])
    tf, ratio = pipe.run_ransac(n_draws=10, draw_size=5, max_inliers_distance=0.1, method="sc2")
    args, kw = calls[-1]
    assert ratio == 0.25 and len(args) == 4 and np.array_equal(args[1], np.arange(4)[::-1]) and np.array_equal(args[3], np.ones((4, 3)))
    assert kw == dict(distance_threshold=0.1, n_seeds=256, refit_iterations=2)  # n_draws and draw_size do not reach it
    pipe.run_ransac(max_inliers_distance=0.2, method="sc2", sc2_seeds=64, refit_iterations=0)
    assert calls[-1][1] == dict(distance_threshold=0.2, n_seeds=64, refit_iterations=0)
    p = inspect.signature(P.RegistrationPipeline.run_ransac).parameters
    assert p["method"].default == "reference" and p["sc2_seeds"].default == 256
    with pytest.raises(ValueError):
        pipe.run_ransac(method="sc3")
    assert len(calls) == 2


def test_command_line_reaches_the_call(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import register_point_clouds as cli
    finally:
        sys.path.pop(0)
    base = ["scan.ply", "ref.ply", "--radius", "0.1", "--icp", "none"]
    a = cli.parse_args(base)
    assert (a.ransac, a.sc2_seeds) == ("reference", 256)
    a = cli.parse_args(base + ["--ransac", "sc2", "--sc2-seeds", "64", "--ransac-threshold", "0.02", "--consistency-sc2", "0.02"])
    assert (a.ransac, a.sc2_seeds, a.ransac_threshold, a.consistency_sc2) == ("sc2", 64, 0.02, 0.02)
    assert cli.parse_args(base + ["--ransac", "sc2", "--consistency", "0.03"]).consistency == 0.03
    order = []

    class Pipe:
        def __init__(self, **kw):
            self.matches = (np.arange(3), np.arange(3))

        def select_keypoints(self, *a, **kw):
            pass

        compute_descriptors = find_descriptors_matches = select_keypoints

        def filter_matches_by_consistency(self, *a, **kw):
            order.append("consistency")

        def run_ransac(self, **kw):
            order.append(kw)
            return shot_fpfh_amd.core.RigidTransform(), 0.5

        def compute_metrics_post_icp(self, *a):
            return 1.0, 1.0

    monkeypatch.setattr(cli, "RegistrationPipeline", Pipe)
    monkeypatch.setattr(cli, "get_data", lambda *a, **kw: (np.zeros((3, 3)), np.zeros((3, 3))))
    assert cli.main(base + ["--ransac", "sc2", "--sc2-seeds", "64", "--ransac-threshold", "0.02", "--consistency", "0.03"]) == 0
    assert order[0] == "consistency"  # the filter thins the matches first
    seen = order[1]
    assert (seen["method"], seen["sc2_seeds"], seen["max_inliers_distance"], seen["refit_iterations"]) == ("sc2", 64, 0.02, 2)
    assert cli.main(base) == 0 and order[-1]["method"] == "reference" and order[-1]["sc2_seeds"] == 256
