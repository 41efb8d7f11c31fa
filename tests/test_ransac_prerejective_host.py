"""Host side of ransac_prerejective: arguments, exports, the draw stream of a call, buffers on the error paths, the pipeline keyword
and the command line -- on tests/fake_engine.py with the K11 calls answered by the NumPy statement (tests/ransac_numpy.py)."""
import inspect
import os
import sys

import numpy as np
import pytest

import ransac_numpy as N
from fake_engine import FakeArray, FakeEngine

import shot_fpfh_amd
import shot_fpfh_amd.matching as matching
import shot_fpfh_amd.matching.ransac as R
from shot_fpfh_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """FakeEngine + the three K11 calls, from the NumPy statement.  `fail` names a call that raises."""

    def __init__(self, fail=None):
        self.fail, self.draw_tables = fail, []

    def empty(self, shape, dtype=np.float64):
        if self.fail == "empty_draws" and np.dtype(dtype) == np.int64 and len(shape) == 2:
            raise MemoryError("no room for the draws")
        return _Tracked(shape, dtype)

    def ransac_prerejective_device(self, a, b, m, draws, n_draws, draw_size, sim, thr, **_):
        if self.fail == "prerejective":
            raise RuntimeError("device call failed")
        self.draw_tables.append(draws.a.copy())
        status, rt, _, _, _ = N.hypotheses(a.a[:m], b.a[:m], draws.a, sim)
        slot_draw = np.flatnonzero(status == 0)
        res = np.array([(status == 1).sum(), (status == 2).sum(), slot_draw.size, -1, 0, -1, 0, 0], dtype=np.int64)
        best = np.zeros(12)
        if slot_draw.size:
            counts = N.score(a.a[:m], b.a[:m], rt[slot_draw], thr)
            w = N.first_max(counts)
            res[3:6] = slot_draw[w], counts[w], w
            best = rt[slot_draw[w]]
        return res, best

    def ransac_refit_sums(self, a, b, m, rt, thr):
        if self.fail == "refit":
            raise RuntimeError("refit failed")
        s = N.refit_sums(a.a[:m], b.a[:m], N.inlier_mask(a.a[:m], b.a[:m], rt, thr))
        out = np.zeros(24)
        out[0], out[1:4], out[4:7], out[7:16], out[17:20], out[20:23] = s["count"], s["abar"], s["bbar"], s["h"].reshape(9), s["sum_a"], s["sum_b"]
        return out


@pytest.fixture()
def matches():
    return N.synthetic_matches(600, 0.5, seed=5)


def test_exports_and_signatures():
    assert shot_fpfh_amd.ransac_prerejective is R.ransac_prerejective is matching.ransac_prerejective
    assert "ransac_prerejective" in shot_fpfh_amd.__all__ and "ransac_prerejective" in matching.__all__ and "ransac_prerejective" in R.__all__
    p = inspect.signature(R.ransac_prerejective).parameters
    assert (p["n_draws"].default, p["draw_size"].default, p["edge_similarity"].default, p["refit_iterations"].default, p["seed"].default) == (10000, 3, 0.9, 2, 72)
    header = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name in ("sf_ransac_hypotheses", "sf_ransac_refit_sums", "sf_ransac_prerejective"):
        assert name in _ffi.SIGNATURES and f"int {name}(" in header
    for method in ("ransac_hypotheses_device", "ransac_refit_sums", "ransac_prerejective_device"):
        assert callable(getattr(shot_fpfh_amd.Engine, method))
    # the old call is what it was
    q = inspect.signature(R.ransac_on_matches).parameters
    assert (q["n_draws"].default, q["draw_size"].default, q["distance_threshold"].default) == (10000, 4, 1)


@pytest.mark.parametrize("kw", [dict(draw_size=2), dict(draw_size=9), dict(edge_similarity=1.0), dict(edge_similarity=-0.1),
                                dict(edge_similarity=float("nan")), dict(refit_iterations=-1), dict(n_draws=0), dict(n_draws=-5)])
def test_bad_arguments_raise_before_any_device_work(matches, kw):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    with pytest.raises(ValueError):
        R.ransac_prerejective(si, ri, sk, rk, engine=_Engine(), **kw)
    assert _Tracked.live == before


def test_too_few_matches_and_mismatched_indices(matches):
    sk, rk, si, ri = matches[:4]
    for a, b, kw in ((si[:0], ri[:0], {}), (si[:3], ri[:3], dict(draw_size=4)), (si, ri[:-1], {})):
        with pytest.raises(ValueError):
            R.ransac_prerejective(a, b, sk, rk, engine=_Engine(), **kw)


def test_result_follows_the_numpy_statement(matches):
    sk, rk, si, ri, r0, t0 = matches
    ratio, tf, rec = R.ransac_prerejective(si, ri, sk, rk, n_draws=800, distance_threshold=0.01, engine=_Engine())
    want = N.ransac_prerejective(si, ri, sk, rk, n_draws=800, distance_threshold=0.01)
    assert ratio == want[0] and rec.winner_draw == want[3]["winner_draw"] and rec.refit_inliers == want[3]["refit_inliers"]
    assert (rec.n_rejected, rec.n_degenerate, rec.n_scored) == (want[3]["n_rejected"], want[3]["n_degenerate"], want[3]["n_scored"])
    assert rec.n_rejected + rec.n_degenerate + rec.n_scored == rec.n_draws == 800
    assert np.allclose(tf.rotation, want[1], atol=1e-12) and np.allclose(tf.translation, want[2], atol=1e-12)
    assert np.allclose(tf.rotation.T @ tf.rotation, np.eye(3), atol=1e-14)  # normalize_rotation applied
    assert np.linalg.norm(tf.rotation - r0) < 5e-3


def test_seed_makes_a_call_reproducible_and_leaves_the_module_generator_alone(matches):
    sk, rk, si, ri = matches[:4]
    state = R.rng.bit_generator.state
    eng = _Engine()
    for seed in (72, 72, 73):
        R.ransac_prerejective(si, ri, sk, rk, n_draws=300, distance_threshold=0.01, seed=seed, engine=eng)
    assert np.array_equal(eng.draw_tables[0], eng.draw_tables[1]) and not np.array_equal(eng.draw_tables[0], eng.draw_tables[2])
    assert eng.draw_tables[0].shape == (300, 3) and eng.draw_tables[0].dtype == np.int64
    assert np.array_equal(eng.draw_tables[0], R.draw_stream(np.random.default_rng(72), 600, 3, 300))
    assert R.rng.bit_generator.state == state


@pytest.mark.parametrize("fail", ["empty_draws", "prerejective", "refit", "no_survivor"])
def test_device_buffers_are_freed_on_every_error_path(matches, fail):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    if fail == "no_survivor":
        with pytest.raises(ValueError, match="rejected"):
            R.ransac_prerejective(si, ri, sk, rk, n_draws=200, draw_size=8, distance_threshold=0.01, edge_similarity=0.99, engine=_Engine())
    else:
        with pytest.raises((MemoryError, RuntimeError)):
            R.ransac_prerejective(si, ri, sk, rk, n_draws=200, distance_threshold=0.01, engine=_Engine(fail))
    assert _Tracked.live == before
    R.ransac_prerejective(si, ri, sk, rk, n_draws=200, distance_threshold=0.01, engine=_Engine())
    assert _Tracked.live == before


def test_old_path_frees_the_chunks_nobody_collected(matches, monkeypatch):
    """ransac_on_matches queues one scoring job per chunk; an error while a later chunk is being queued used to leave the buffers
    of the earlier ones to the garbage collector."""
    sk, rk, si, ri = matches[:4]

    class Eng(_Engine):
        calls = 0

        def ransac_score_device(self, a, b, m, rt, n, thr, out):
            Eng.calls += 1
            if Eng.calls == 2:
                raise RuntimeError("second chunk failed")

    before = _Tracked.live
    with pytest.raises(RuntimeError, match="second chunk"):
        R.ransac_on_matches(si, ri, sk, rk, n_draws=3000, distance_threshold=0.01, engine=Eng())
    assert Eng.calls == 2 and _Tracked.live == before


def test_run_ransac_method_keyword(monkeypatch):
    import shot_fpfh_amd.pipeline as P

    calls = []

    def old(*args, **kw):
        calls.append(("reference", kw))
        return 0.5, shot_fpfh_amd.core.RigidTransform()

    def new(*args, **kw):
        calls.append(("prerejective", kw))
        return 0.25, shot_fpfh_amd.core.RigidTransform(), R.RansacRecord()

    monkeypatch.setattr(P, "ransac_on_matches", old)
    monkeypatch.setattr(P, "ransac_prerejective", new)
    pipe = P.RegistrationPipeline.__new__(P.RegistrationPipeline)
    pipe.scan, pipe.ref = np.zeros((4, 3)), np.zeros((4, 3))
    pipe.scan_keypoints = pipe.ref_keypoints = np.arange(4)
    pipe.matches = (np.arange(4), np.arange(4))
    assert inspect.signature(P.RegistrationPipeline.run_ransac).parameters["method"].default == "reference"
    tf, ratio = pipe.run_ransac(n_draws=10, max_inliers_distance=0.1)
    assert ratio == 0.5 and calls[-1][0] == "reference" and calls[-1][1]["draw_size"] == 4 and calls[-1][1]["distance_threshold"] == 0.1
    tf, ratio = pipe.run_ransac(n_draws=10, method="reference", draw_size=5)
    assert calls[-1][0] == "reference" and calls[-1][1]["draw_size"] == 5
    tf, ratio = pipe.run_ransac(n_draws=10, method="prerejective", edge_similarity=0.8, refit_iterations=1)
    assert ratio == 0.25 and calls[-1][0] == "prerejective"
    assert (calls[-1][1]["draw_size"], calls[-1][1]["edge_similarity"], calls[-1][1]["refit_iterations"]) == (4, 0.8, 1)
    pipe.run_ransac(n_draws=10, method="prerejective", draw_size=3)
    assert (calls[-1][1]["draw_size"], calls[-1][1]["edge_similarity"], calls[-1][1]["refit_iterations"]) == (3, 0.9, 2)
    with pytest.raises(ValueError):
        pipe.run_ransac(method="other")


def test_command_line_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import register_point_clouds as cli
    finally:
        sys.path.pop(0)
    base = ["scan.ply", "ref.ply", "--radius", "0.1"]
    a = cli.parse_args(base)
    assert (a.ransac, a.ransac_edge_similarity, a.ransac_refit, a.ransac_draw_size) == ("reference", 0.9, 2, None)
    a = cli.parse_args(base + ["--ransac", "prerejective", "--ransac-edge-similarity", "0.8", "--ransac-refit", "0", "--ransac-draw-size", "4"])
    assert (a.ransac, a.ransac_edge_similarity, a.ransac_refit, a.ransac_draw_size) == ("prerejective", 0.8, 0, 4)
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--ransac", "open3d"])
