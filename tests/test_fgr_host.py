"""Host side of fast_global_registration: the NumPy statement of the definition itself (tests/fgr_numpy.py) converges, and the
public call's arguments, exports, tuple selection, buffers on the error paths, the pipeline keyword and the command line -- on
tests/fake_engine.py with the K12 calls answered by the NumPy statement."""
import inspect
import os
import sys

import numpy as np
import pytest

import fgr_numpy as F
import ransac_numpy as N
from fake_engine import FakeArray, FakeEngine

import shot_fpfh_amd
import shot_fpfh_amd.matching as matching
import shot_fpfh_amd.matching.fgr as G
from shot_fpfh_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.01
# (m, share of true matches, seed) and the values a sketch of the definition gave: |R - R0|_F, |t - t0|
SETS = [(20000, 0.30, 0), (20000, 0.10, 1), (20000, 0.05, 2), (2000, 0.30, 3), (200000, 0.30, 4), (20000, 0.50, 5)]
CAP = 2e-3  # three times the sketch's worst value, one order under what outliers do to an unweighted fit
_runs = {}


def _run(case):
    if case not in _runs:
        m, share, seed = case
        sk, rk, si, ri, r0, t0 = F.synthetic_matches(m, share, seed=seed)
        ratio, rot, tr, rec = F.fast_global_registration(si, ri, sk, rk, THR)
        _runs[case] = (ratio, rot, tr, rec, r0, t0)
    return _runs[case]


# ---- 1, 2: the definition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SETS, ids=str)
def test_definition_recovers_the_motion(case):
    ratio, rot, tr, rec, r0, t0 = _run(case)
    er, et = float(np.linalg.norm(rot - r0)), float(np.linalg.norm(tr - t0))
    print(f"{case}: |R - R0| = {er:.2e}, |t - t0| = {et:.2e}, inlier ratio {ratio:.4f}, final mu {rec['mu']:.4g}")
    assert rec["status"] == F.STATUS_OK and rec["iterations"] == 64
    assert er <= CAP and et <= CAP
    assert abs(ratio - case[1]) <= 0.02  # (the true matches, and a few random ones, are its inliers)


@pytest.mark.parametrize("case", SETS, ids=str)
def test_cost_does_not_rise_while_mu_stays(case):
    trace = _run(case)[3]["trace"]
    same_mu = trace[1:, 0] == trace[:-1, 0]
    rise = trace[1:, 1] - trace[:-1, 1]
    print(f"{case}: largest change of E between two iterations of one mu: {rise[same_mu].max():.3e}")
    assert same_mu.sum() == 48 and np.all(rise[same_mu] <= 0.0)
    # the schedule: mu divided after every fourth iteration, never under its floor
    assert np.array_equal(trace[::4, 0], trace[3::4, 0]) and np.all(trace[4::4, 0] == np.maximum(trace[:-4:4, 0] / 1.4, (THR / _run(case)[3]["s"]) ** 2))


def test_sums_are_the_gauss_newton_system_of_the_cost():
    """A and g against the Jacobian formed explicitly, E against the cost; the gradient of E is 2 g."""
    rng = np.random.default_rng(1)
    x, y = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    rot, t, mu = F.rodrigues(np.array([0.2, -0.1, 0.3])), np.array([0.1, 0.2, -0.3]), 0.37
    s = F.sums(x, y, rot, t, mu)
    p = x @ rot.T + t
    r = p - y
    w = (mu / (mu + (r * r).sum(axis=1))) ** 2
    J = np.zeros((50, 3, 6))
    J[:, :, 3:] = np.eye(3)
    J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = p[:, 2], -p[:, 1], -p[:, 2], p[:, 0], p[:, 1], -p[:, 0]
    assert np.allclose(s["A"], np.einsum("k,kij,kil->jl", w, J, J), atol=1e-12)
    assert np.allclose(s["g"], np.einsum("k,kij,ki->j", w, J, r), atol=1e-12)
    rr = (r * r).sum(axis=1)
    assert np.isclose(s["E"], (mu * rr / (mu + rr)).sum(), rtol=1e-12) and np.isclose(s["W"], w.sum(), rtol=1e-12)
    assert np.all(s["abs"] >= np.abs(s["vec"]) * (1 - 1e-12))

    def cost(xi):
        q = x @ (F.rodrigues(xi[:3]) @ rot).T + F.rodrigues(xi[:3]) @ t + xi[3:] - y
        qq = (q * q).sum(axis=1)
        return (mu * qq / (mu + qq)).sum()

    h = 1e-6
    grad = np.array([(cost(h * e) - cost(-h * e)) / (2 * h) for e in np.eye(6)])
    assert np.allclose(grad, 2 * s["g"], rtol=1e-6, atol=1e-8)


def test_definition_corners():
    line = np.outer(np.linspace(-1, 1, 30), [1.0, 2.0, -0.5])
    out = F.fgr_rows(line + 0.3, line * 1.0 - 0.1, THR)
    assert out["status"] == F.STATUS_DEGENERATE and out["iterations"] == 0 and np.array_equal(out["R"], np.eye(3))
    assert np.isfinite(out["t"]).all() and not out["trace"].any()
    one = np.full((10, 3), 0.5)
    for a, b in ((one, one), (one[:2], one[:2])):
        with pytest.raises(ValueError):
            F.fgr_rows(a, b, THR)
    for kw in (dict(iterations=0), dict(decrease_every=0), dict(division_factor=1.0)):
        with pytest.raises(ValueError):
            F.fgr_rows(line, line, THR, **kw)
    # three generic points: an exact fit
    a = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.4], [0.3, 0.8, 0.7]])
    rot = F.rodrigues(np.array([0.3, -0.2, 0.4]))
    b = a @ rot.T + [0.2, -0.1, 0.05]
    out = F.fgr_rows(a, b, THR)
    assert out["status"] == F.STATUS_OK and np.abs(a @ out["R"].T + out["t"] - b).max() <= 1e-12 * out["s"]


@pytest.mark.parametrize("scale", [(1.0, 1.0, 1e-3), (1.0, 1e-3, 1e-3)], ids=["slab", "needle"])
def test_thin_but_valid_sets_are_still_fitted(scale):
    """The pivot rule d_j <= 1e-12 A_jj must not take a thin slab or a needle of keypoints for points on one line: their
    smallest pivot is about (thickness / extent)^2 = 1e-6 of its diagonal entry."""
    rng = np.random.default_rng(8)
    a = (rng.random((400, 3)) - 0.5) * np.array(scale)
    rot = F.rodrigues(np.array([0.2, 0.5, -0.3]))
    b = a @ rot.T + [0.3, -0.2, 0.1]
    out = F.fgr_rows(a, b, 1e-5)
    assert out["status"] == F.STATUS_OK and out["iterations"] == 64
    assert np.abs(a @ out["R"].T + out["t"] - b).max() <= 1e-9


# ---- 3: the public call on a stand-in engine ----------------------------------------------------------------------------------------
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
    """FakeEngine + the calls fast_global_registration makes, from the NumPy statements.  `fail` names a call that raises."""

    def __init__(self, fail=None):
        self.fail, self.selections, self.draw_tables = fail, [], []

    def empty(self, shape, dtype=np.float64):
        if self.fail == "empty_sel" and np.dtype(dtype) == np.int64 and len(shape) == 1 and self.draw_tables:
            raise MemoryError("no room for the selection")
        return _Tracked(shape, dtype)

    def ransac_hypotheses_device(self, a, b, m, draws, n_draws, draw_size, sim, status, rt):
        if self.fail == "hypotheses":
            raise RuntimeError("hypotheses failed")
        self.draw_tables.append(draws.a.copy())
        status.a[:n_draws] = N.hypotheses(a.a[:m], b.a[:m], draws.a[:n_draws], sim)[0]

    def fgr_device(self, a, b, m, thr, iterations=64, decrease_every=4, division_factor=1.4, sel=None, k=None):
        if self.fail == "fgr":
            raise RuntimeError("device call failed")
        rows = slice(0, m) if sel is None else sel.a[:k]
        self.selections.append(None if sel is None else sel.a[:k].copy())
        try:
            out = F.fgr_rows(a.a[:m][rows], b.a[:m][rows], thr, iterations, division_factor, decrease_every)
        except ValueError:  # no extent: what the device reports as status 2
            return np.zeros(12), np.array([2.0, 0, 1, 0, 0, 0, 0, 0]), np.zeros((iterations, 4))
        info = np.array([out["status"], out["iterations"], out["mu"], out["s"], out["E"], out["W"], 0, 0], dtype=np.float64)
        return np.concatenate([out["R"].reshape(9), out["t"]]), info, out["trace"]

    def ransac_refit_sums(self, a, b, m, rt, thr):
        if self.fail == "count":
            raise RuntimeError("count failed")
        out = np.zeros(24)
        out[0] = np.count_nonzero(N.inlier_mask(a.a[:m], b.a[:m], np.asarray(rt), thr))
        return out


@pytest.fixture()
def matches():
    return N.synthetic_matches(600, 0.5, seed=5)


def test_exports_signature_and_abi_table():
    assert shot_fpfh_amd.fast_global_registration is G.fast_global_registration is matching.fast_global_registration
    assert matching.FgrRecord is G.FgrRecord
    assert "fast_global_registration" in shot_fpfh_amd.__all__ and "fast_global_registration" in matching.__all__
    assert "FgrRecord" in matching.__all__ and set(G.__all__) == {"fast_global_registration", "FgrRecord"}
    p = inspect.signature(G.fast_global_registration).parameters
    names = list(p)
    assert names[:4] == ["scan_descriptors_indices", "ref_descriptors_indices", "scan_keypoints", "ref_keypoints"]
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:4])
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[4:])
    assert p["distance_threshold"].default is inspect.Parameter.empty
    got = tuple(p[n].default for n in ("iterations", "division_factor", "decrease_every", "tuple_count", "tuple_scale", "seed"))
    assert got == (64, 1.4, 4, 0, 0.95, 72)
    header = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name in ("sf_fgr_sums", "sf_fgr"):
        assert name in _ffi.SIGNATURES and f"int {name}(" in header
    assert len(_ffi.SIGNATURES["sf_fgr"][1]) == 13 and len(_ffi.SIGNATURES["sf_fgr_sums"][1]) == 8
    for method in ("fgr_sums", "fgr_device"):
        assert callable(getattr(shot_fpfh_amd.Engine, method))
    assert "fgr.hip" in open(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(decrease_every=0), dict(division_factor=1.0), dict(division_factor=float("nan")),
                                dict(distance_threshold=float("inf")), dict(distance_threshold=float("nan")), dict(tuple_count=-1), dict(iterations=2.9),
                                dict(tuple_scale=1.0)])
def test_bad_arguments_raise_before_any_device_work(matches, kw):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    eng = _Engine()
    with pytest.raises(ValueError):
        G.fast_global_registration(si, ri, sk, rk, **{"distance_threshold": THR, "engine": eng, **kw})
    assert _Tracked.live == before and not eng.selections
    with pytest.raises(TypeError):
        G.fast_global_registration(si, ri, sk, rk, THR, engine=eng)  # the threshold is keyword-only


def test_too_few_matches_and_mismatched_indices(matches):
    sk, rk, si, ri = matches[:4]
    for a, b in ((si[:0], ri[:0]), (si[:2], ri[:2]), (si, ri[:-1])):
        with pytest.raises(ValueError):
            G.fast_global_registration(a, b, sk, rk, distance_threshold=THR, engine=_Engine())


def test_result_follows_the_numpy_statement(matches):
    sk, rk, si, ri, r0, t0 = matches
    state = np.random.get_state()[1].copy()
    ratio, tf, rec = G.fast_global_registration(si, ri, sk, rk, distance_threshold=THR, engine=_Engine())
    want = F.fast_global_registration(si, ri, sk, rk, THR)
    assert ratio == want[0] and rec.inliers == want[3]["inliers"] and rec.rows == 600 and rec.status == "done"
    assert (rec.iterations, rec.mu, rec.scale) == (64, want[3]["mu"], want[3]["s"]) and np.array_equal(rec.trace, want[3]["trace"])
    assert np.allclose(tf.rotation, want[1], atol=1e-12) and np.allclose(tf.translation, want[2], atol=1e-12)
    assert np.allclose(tf.rotation.T @ tf.rotation, np.eye(3), atol=1e-14)  # normalize_rotation applied
    assert np.linalg.norm(tf.rotation - r0) < 5e-3
    assert np.array_equal(np.random.get_state()[1], state)
    # no draws: the seed changes nothing
    again = G.fast_global_registration(si, ri, sk, rk, distance_threshold=THR, seed=5, engine=_Engine())
    assert again[0] == ratio and np.array_equal(again[1].rotation, tf.rotation) and np.array_equal(again[1].translation, tf.translation)


def test_tuple_selection_equals_the_numpy_statement(matches):
    import shot_fpfh_amd.matching.ransac as R

    sk, rk, si, ri = matches[:4]
    a, b = N.matched_points(si, ri, sk, rk)
    state = R.rng.bit_generator.state
    eng = _Engine()
    ratio, tf, rec = G.fast_global_registration(si, ri, sk, rk, distance_threshold=THR, tuple_count=40, seed=9, engine=eng)
    want = F.tuple_selection(a, b, 40, 0.95, 9)
    assert want.shape == (120,) and want.dtype == np.int64 and rec.rows == 120
    assert np.array_equal(eng.selections[0], want)
    assert eng.draw_tables[0].shape == (4000, 3) and np.array_equal(eng.draw_tables[0], R.draw_stream(np.random.default_rng(9), 600, 3, 4000))
    ref = F.fast_global_registration(si, ri, sk, rk, THR, tuple_count=40, seed=9)
    assert ratio == ref[0] and np.allclose(tf.rotation, ref[1], atol=1e-12)
    assert R.rng.bit_generator.state == state  # the module generator of ransac_on_matches is left alone
    other = _Engine()
    G.fast_global_registration(si, ri, sk, rk, distance_threshold=THR, tuple_count=40, seed=10, engine=other)
    assert not np.array_equal(other.selections[0], want)


@pytest.mark.parametrize("fail", ["hypotheses", "empty_sel", "fgr", "count", "no_tuple", "degenerate", "no_extent"])
def test_device_buffers_are_freed_on_every_error_path(matches, fail):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    kw = dict(distance_threshold=THR)
    if fail == "no_tuple":  # random pairings only: no triple keeps its edge lengths within 0.1 %
        with pytest.raises(ValueError, match="tuple test"):
            G.fast_global_registration(si, np.roll(ri, 7), sk, rk, tuple_count=2, tuple_scale=0.999, engine=_Engine(), **kw)
    elif fail == "degenerate":
        line = np.outer(np.linspace(-1, 1, 30), [1.0, 2.0, -0.5])
        with pytest.raises(ValueError, match="degenerate"):
            G.fast_global_registration(np.arange(30), np.arange(30), line, line + 0.25, engine=_Engine(), **kw)
    elif fail == "no_extent":
        one = np.full((30, 3), 0.5)
        with pytest.raises(ValueError, match="extent"):
            G.fast_global_registration(np.arange(30), np.arange(30), one, one, engine=_Engine(), **kw)
    else:
        with pytest.raises((MemoryError, RuntimeError)):
            G.fast_global_registration(si, ri, sk, rk, tuple_count=20, engine=_Engine(fail), **kw)
    assert _Tracked.live == before
    G.fast_global_registration(si, ri, sk, rk, tuple_count=20, engine=_Engine(), **kw)
    assert _Tracked.live == before


# ---- 4: pipeline and command line ---------------------------------------------------------------------------------------------------
def test_run_ransac_reaches_the_call(monkeypatch):
    import shot_fpfh_amd.pipeline as P

    calls = []

    def fgr(*args, **kw):
        calls.append((args, kw))
        return 0.75, shot_fpfh_amd.core.RigidTransform(), G.FgrRecord(iterations=7)

    monkeypatch.setattr(P, "fast_global_registration", fgr)
    pipe = P.RegistrationPipeline.__new__(P.RegistrationPipeline)
    pipe.scan, pipe.ref = np.zeros((4, 3)), np.ones((4, 3))
    pipe.scan_keypoints = pipe.ref_keypoints = np.arange(4)
    pipe.matches = (np.arange(4), np.arange(4)[::-1])
    tf, ratio = pipe.run_ransac(n_draws=10, draw_size=5, max_inliers_distance=0.1, method="fgr")
    args, kw = calls[-1]
    assert ratio == 0.75 and len(args) == 4 and np.array_equal(args[1], np.arange(4)[::-1]) and np.array_equal(args[3], np.ones((4, 3)))
    assert kw == dict(distance_threshold=0.1, iterations=64, tuple_count=0)  # n_draws and draw_size do not reach it
    pipe.run_ransac(max_inliers_distance=0.2, method="fgr", fgr_iterations=32, fgr_tuple_count=500)
    assert calls[-1][1] == dict(distance_threshold=0.2, iterations=32, tuple_count=500)
    assert inspect.signature(P.RegistrationPipeline.run_ransac).parameters["method"].default == "reference"
    with pytest.raises(ValueError):
        pipe.run_ransac(method="open3d")
    assert len(calls) == 2


def test_command_line_reaches_the_call(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import register_point_clouds as cli
    finally:
        sys.path.pop(0)
    base = ["scan.ply", "ref.ply", "--radius", "0.1"]
    a = cli.parse_args(base)
    assert (a.ransac, a.fgr_iterations, a.fgr_tuples) == ("reference", 64, 0)
    a = cli.parse_args(base + ["--ransac", "fgr", "--fgr-iterations", "48", "--fgr-tuples", "1000", "--ransac-threshold", "0.02"])
    assert (a.ransac, a.fgr_iterations, a.fgr_tuples, a.ransac_threshold) == ("fgr", 48, 1000, 0.02)
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--ransac", "open3d"])
    # main() hands them to run_ransac
    seen = {}

    class Pipe:
        def __init__(self, **kw):
            self.matches = (np.arange(3), np.arange(3))

        def select_keypoints(self, *a, **kw):
            pass

        compute_descriptors = find_descriptors_matches = select_keypoints

        def run_ransac(self, **kw):
            seen.update(kw)
            return shot_fpfh_amd.core.RigidTransform(), 0.5

        def compute_metrics_post_icp(self, *a):
            return 1.0, 1.0

    monkeypatch.setattr(cli, "RegistrationPipeline", Pipe)
    monkeypatch.setattr(cli, "get_data", lambda *a, **kw: (np.zeros((3, 3)), np.zeros((3, 3))))
    cli.main(base + ["--ransac", "fgr", "--fgr-iterations", "48", "--ransac-threshold", "0.02", "--icp", "none"])
    assert (seen["method"], seen["fgr_iterations"], seen["fgr_tuple_count"], seen["max_inliers_distance"]) == ("fgr", 48, 0, 0.02)
