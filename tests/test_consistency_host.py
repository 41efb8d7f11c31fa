"""Host side of geometric_consistency_filter: the NumPy statement of the definition (tests/consistency_numpy.py) against loops
over the pairs, what it does on the project's synthetic matches, and the public call's arguments, exports, pipeline stage and
command-line flag -- on a stand-in engine that answers the K13 calls from the statement."""
import inspect
import math
import os
import sys

import numpy as np
import pytest

import consistency_numpy as C
import ransac_numpy as N
from fake_engine import FakeArray, FakeEngine

import shot_fpfh_amd
import shot_fpfh_amd.matching as matching
import shot_fpfh_amd.matching.consistency as G
from shot_fpfh_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.01
# (m, share of true matches, seed): the sets of the issue's table that a CPU can afford
PURPOSE_SETS = [(5000, 0.10, 5010), (5000, 0.05, 1), (2000, 0.05, 2), (2000, 0.30, 3)]


# ---- 1. the statement against loops -------------------------------------------------------------------------------------------------
def _length(p, i, j):
    s = None
    for c in range(3):
        d = float(p[i, c]) - float(p[j, c])
        s = d * d if s is None else s + d * d
    return math.sqrt(s) if s == s and s >= 0 else float("nan")


def _brute_compat(a, b, i, j, thr, edge):
    if i == j:
        return False
    dp, dq = _length(a, i, j), _length(b, i, j)
    return abs(dp - dq) <= thr and min(dp, dq) >= edge and dp == dp and dq == dq


def _brute_degree(a, b, thr, edge, member=None):
    m = a.shape[0]
    return np.array([sum(1 for j in range(m) if (member is None or member[j]) and _brute_compat(a, b, i, j, thr, edge))
                     for i in range(m)], dtype=np.uint32)


def _brute_group(a, b, thr, edge, share):
    m = a.shape[0]
    deg = _brute_degree(a, b, thr, edge)
    seed = min(i for i in range(m) if deg[i] == deg.max())
    if deg[seed] == 0:
        return dict(status=C.STATUS_NO_PAIR, seed=-1, degree=deg, keep=[])
    member = [1 if j == seed or _brute_compat(a, b, seed, j, thr, edge) else 0 for j in range(m)]
    g = sum(member)
    gdeg = _brute_degree(a, b, thr, edge, member)
    keep = [i for i in range(m) if member[i] and float(gdeg[i]) >= share * float(g - 1)]
    return dict(status=C.STATUS_OK, seed=seed, degree=deg, member=np.array(member, dtype=np.uint8), g=g, group_degree=gdeg, keep=keep)


def _small_sets():
    rng = np.random.default_rng(4)
    sk, rk, si, ri, _, _ = N.synthetic_matches(40, 0.5, sigma=0.002, seed=9)
    a, b = N.matched_points(si, ri, sk, rk)
    out = {"synthetic": (a, b, THR, THR), "lattice": C.lattice_set(40, seed=1), "tie": C.tie_set(40, seed=2)}
    shared = b.copy()
    shared[rng.integers(0, 40, 12)] = b[7]  # many-to-one: twelve matches end on reference keypoint 7
    out["shared keypoint"] = (a, shared, THR, THR)
    out["shared keypoint, min_edge 0"] = (a, shared, THR, 0.0)
    bad = a.copy()
    bad[5, 1] = np.nan
    out["nan row"] = (bad, b, THR, THR)
    worse = b.copy()
    worse[3] = np.inf
    out["inf row"] = (a, worse, THR, THR)
    return out


SMALL = _small_sets()


@pytest.mark.parametrize("name", list(SMALL), ids=str)
def test_statement_equals_loops_over_the_pairs(name):
    a, b, thr, edge = SMALL[name]
    want = _brute_group(a, b, thr, edge, 0.4)
    got = C.group(a, b, thr, edge, 0.4)
    assert got["status"] == want["status"] and got["seed"] == want["seed"]
    assert np.array_equal(C.degree(a, b, thr, edge), want["degree"])
    assert list(got["keep"]) == want["keep"]
    if want["status"] == C.STATUS_OK:
        for key in ("degree", "member", "group_degree"):
            assert np.array_equal(got[key], want[key]), key
        assert got["g"] == want["g"]
    mask = np.random.default_rng(6).random(a.shape[0]) < 0.4
    assert np.array_equal(C.degree(a, b, thr, edge, member=mask), _brute_degree(a, b, thr, edge, mask))
    assert not C.degree(a, b, thr, edge, member=np.zeros(a.shape[0], dtype=np.uint8)).any()  # an all-zero mask
    assert np.array_equal(C.degree(a, b, thr, edge, chunk=7), want["degree"])  # the chunking changes nothing


def test_the_constructed_sets_hit_their_edges():
    a, b, thr, edge = SMALL["lattice"]
    rows = np.arange(40)
    dp, dq = C.lengths(a, rows), C.lengths(b, rows)
    off = ~np.eye(40, dtype=bool)
    on_thr = off & (np.abs(dp - dq) == thr) & (np.minimum(dp, dq) >= edge)
    on_edge = off & (np.minimum(dp, dq) == edge) & (np.abs(dp - dq) <= thr)
    assert on_thr.sum() >= 20 and on_edge.sum() >= 20 and (off & (dp == 0)).sum() >= 2
    ok = C.compat_rows(a, b, rows, thr, edge)
    assert ok[on_thr].all() and ok[on_edge].all() and not ok[off & (np.minimum(dp, dq) == 0)].any()  # "<=" and ">=" include the edge
    assert np.array_equal(ok, ok.T)
    # the tie: rows 5 .. 39 share the maximum and the lowest of them is the seed
    a, b, thr, edge = SMALL["tie"]
    out = C.group(a, b, thr, edge)
    assert (out["degree"][5:] == 34).all() and out["degree"][:5].max() < 34 and out["seed"] == 5 and list(out["keep"]) == list(range(5, 40))
    # a row that is not finite is compatible with nothing and changes nobody else's count
    a, b, thr, edge = SMALL["nan row"]
    deg = C.degree(a, b, thr, edge)
    rest = np.delete(np.arange(40), 5)
    assert deg[5] == 0 and np.array_equal(deg[rest], C.degree(a[rest], b[rest], thr, edge))
    # matches that share a keypoint do not vote for each other unless min_edge is 0
    a, b, thr, edge = SMALL["shared keypoint"]
    same = np.flatnonzero((b == b[7]).all(axis=1))
    assert same.size >= 8 and not C.compat_rows(a, b, same, thr, edge)[:, same].any()


def test_corners_of_the_statement():
    one = np.zeros((1, 3))
    assert C.group(one, one, THR)["status"] == C.STATUS_TOO_FEW and C.group(one[:0], one[:0], THR)["keep"].size == 0
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0]])
    out = C.group(a, a * 3.0, THR)  # no two lengths agree
    assert out["status"] == C.STATUS_NO_PAIR and out["seed"] == -1 and out["keep"].size == 0 and not out["member"].any()
    out = C.group(a, a + 1.0, THR)
    assert out["status"] == C.STATUS_OK and out["seed"] == 0 and out["g"] == 3 and list(out["keep"]) == [0, 1, 2]


# ---- 2. what it is for ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PURPOSE_SETS, ids=str)
def test_statement_keeps_exactly_the_true_matches(case):
    m, share, seed = case
    sk, rk, si, ri, r0, t0 = N.synthetic_matches(m, share, seed=seed)
    true, replayed = C.synthetic_truth(m, share, seed)
    assert np.array_equal(replayed, sk)
    kept_s, kept_r, out = C.geometric_consistency_filter(si, ri, sk, rk, THR)
    is_true = np.zeros(m, dtype=bool)
    is_true[true] = True
    member = out["member"].astype(bool)
    in_group = out["group_degree"] / (out["g"] - 1)
    print(f"{case}: {true.size} true; degree of true min {out['degree'][is_true].min()}, of false max {out['degree'][~is_true].max()}; "
          f"group {out['g']}, kept {out['keep'].size}; share inside the group: true min {in_group[is_true].min():.3f}, "
          f"false max {in_group[member & ~is_true].max(initial=0):.3f}")
    assert np.array_equal(out["keep"], true)
    assert np.array_equal(kept_s, si[true]) and np.array_equal(kept_r, ri[true])


# ---- 3. the public call on a stand-in engine ----------------------------------------------------------------------------------------
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
    """FakeEngine + the call geometric_consistency_filter makes, answered by the NumPy statement."""

    def __init__(self, fail=None):
        self.fail, self.calls = fail, []

    def empty(self, shape, dtype=np.float64):
        if self.fail == "empty" and np.dtype(dtype) == np.uint8:
            raise MemoryError("no room for the members")
        return _Tracked(shape, dtype)

    def consistency_group_device(self, a, b, m, thr, edge, degree, member, group_degree):
        if self.fail == "group":
            raise RuntimeError("device call failed")
        self.calls.append((m, thr, edge))
        out = C.group(a.a[:m], b.a[:m], thr, edge)
        degree.a[:m], member.a[:m], group_degree.a[:m] = out["degree"], out["member"], out["group_degree"]
        info = np.array([out["seed"], out["seed_degree"], out["g"], 0 if out["status"] == C.STATUS_OK else 1], dtype=np.int64)
        return degree, member, group_degree, info


@pytest.fixture(scope="module")
def matches():
    return N.synthetic_matches(600, 0.3, seed=5)


def test_exports_signature_and_abi_table():
    assert shot_fpfh_amd.geometric_consistency_filter is G.geometric_consistency_filter is matching.geometric_consistency_filter
    assert matching.ConsistencyRecord is G.ConsistencyRecord
    assert "geometric_consistency_filter" in shot_fpfh_amd.__all__ and "geometric_consistency_filter" in matching.__all__
    assert "ConsistencyRecord" in matching.__all__ and set(G.__all__) == {"geometric_consistency_filter", "ConsistencyRecord"}
    p = inspect.signature(G.geometric_consistency_filter).parameters
    names = list(p)
    assert names[:4] == ["scan_descriptors_indices", "ref_descriptors_indices", "scan_keypoints", "ref_keypoints"]
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:4])
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[4:])
    assert p["distance_threshold"].default is inspect.Parameter.empty
    assert tuple(p[n].default for n in ("min_edge", "group_share", "verbose", "engine")) == (None, 0.4, False, None)
    assert set(G.ConsistencyRecord.__dataclass_fields__) == {"status", "seed", "group_size", "keep", "degree", "group_degree"}
    header = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name in ("sf_consistency_degree", "sf_consistency_group"):
        assert name in _ffi.SIGNATURES and f"int {name}(" in header
    assert len(_ffi.SIGNATURES["sf_consistency_degree"][1]) == 8 and len(_ffi.SIGNATURES["sf_consistency_group"][1]) == 10
    for method in ("consistency_degree", "consistency_group_device"):
        assert callable(getattr(shot_fpfh_amd.Engine, method))
    assert "consistency.hip" in open(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "Makefile")).read()
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "consistency" in open(os.path.join(ROOT, doc)).read()


@pytest.mark.parametrize("kw", [dict(distance_threshold=-1e-3), dict(distance_threshold=float("nan")), dict(distance_threshold=float("inf")),
                                dict(min_edge=-1.0), dict(min_edge=float("nan")), dict(min_edge=float("inf")), dict(group_share=0.0),
                                dict(group_share=1.5), dict(group_share=-0.1), dict(group_share=float("nan"))])
def test_bad_arguments_raise_before_any_device_work(matches, kw):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    eng = _Engine()
    with pytest.raises(ValueError):
        G.geometric_consistency_filter(si, ri, sk, rk, **{"distance_threshold": THR, "engine": eng, **kw})
    assert _Tracked.live == before and not eng.calls
    with pytest.raises(TypeError):
        G.geometric_consistency_filter(si, ri, sk, rk, THR, engine=eng)  # the threshold is keyword-only
    with pytest.raises(ValueError):
        G.geometric_consistency_filter(si, ri[:-1], sk, rk, distance_threshold=THR, engine=eng)


def test_result_follows_the_numpy_statement(matches):
    sk, rk, si, ri = matches[:4]
    eng = _Engine()
    kept_s, kept_r, rec = G.geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    want = C.geometric_consistency_filter(si, ri, sk, rk, THR)
    assert eng.calls == [(600, THR, THR)]  # min_edge defaults to the threshold
    assert np.array_equal(kept_s, want[0]) and np.array_equal(kept_r, want[1]) and kept_s.dtype == si.dtype
    assert rec.status == "done" and rec.seed == want[2]["seed"] and rec.group_size == want[2]["g"]
    assert np.array_equal(rec.keep, want[2]["keep"]) and rec.keep.dtype == np.int64 and np.all(np.diff(rec.keep) > 0)
    assert np.array_equal(rec.degree, want[2]["degree"]) and np.array_equal(rec.group_degree, want[2]["group_degree"])
    assert np.array_equal(rec.keep, C.synthetic_truth(600, 0.3, 5)[0])
    # a stricter share keeps a subset, min_edge reaches the engine
    strict = G.geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, min_edge=0.05, group_share=1.0, engine=eng)
    assert eng.calls[-1] == (600, THR, 0.05) and set(strict[2].keep) <= set(C.group(*N.matched_points(si, ri, sk, rk), THR, 0.05)["keep"])
    assert np.array_equal(strict[2].keep, C.geometric_consistency_filter(si, ri, sk, rk, THR, 0.05, 1.0)[2]["keep"])


def test_too_few_matches_and_no_pair_return_empty(matches):
    sk, rk, si, ri = matches[:4]
    for n in (0, 1):
        eng = _Engine()
        kept_s, kept_r, rec = G.geometric_consistency_filter(si[:n], ri[:n], sk, rk, distance_threshold=THR, engine=eng)
        assert kept_s.size == kept_r.size == rec.keep.size == 0 and rec.status == "fewer than two matches" and not eng.calls
        assert rec.degree.shape == (n,) and rec.seed == -1 and rec.group_size == 0
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0]])
    kept_s, kept_r, rec = G.geometric_consistency_filter(np.arange(3), np.arange(3), a, 3.0 * a, distance_threshold=THR, engine=_Engine())
    assert kept_s.size == kept_r.size == 0 and rec.status == "no consistent pair" and rec.seed == -1 and not rec.degree.any()


@pytest.mark.parametrize("fail", ["empty", "group", "index"])
def test_device_buffers_are_freed_on_every_error_path(matches, fail):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    if fail == "index":
        with pytest.raises(IndexError):
            G.geometric_consistency_filter(si + 600, ri, sk, rk, distance_threshold=THR, engine=_Engine())
    else:
        with pytest.raises((MemoryError, RuntimeError)):
            G.geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=_Engine(fail))
    assert _Tracked.live == before
    G.geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=_Engine())
    assert _Tracked.live == before


# ---- 4. pipeline and command line ---------------------------------------------------------------------------------------------------
def test_pipeline_stage_replaces_the_matches(monkeypatch, caplog):
    import shot_fpfh_amd.pipeline as P

    calls = []

    def fake(*args, **kw):
        calls.append((args, kw))
        return args[0][1:3], args[1][1:3], G.ConsistencyRecord(group_size=3, keep=np.array([1, 2]))

    monkeypatch.setattr(P, "geometric_consistency_filter", fake)
    pipe = P.RegistrationPipeline.__new__(P.RegistrationPipeline)
    pipe.scan, pipe.ref = np.zeros((4, 3)), np.ones((4, 3))
    pipe.scan_keypoints = pipe.ref_keypoints = np.arange(4)
    pipe.matches = (np.arange(4), np.arange(4)[::-1])
    with caplog.at_level("INFO"):
        assert pipe.filter_matches_by_consistency(0.02) is None
    args, kw = calls[-1]
    assert len(args) == 4 and np.array_equal(args[1], np.arange(4)[::-1]) and np.array_equal(args[3], np.ones((4, 3)))
    assert kw == dict(distance_threshold=0.02, min_edge=None, group_share=0.4)
    assert np.array_equal(pipe.matches[0], [1, 2]) and np.array_equal(pipe.matches[1], [2, 1])
    assert "2 matches kept out of 4" in caplog.text
    pipe.filter_matches_by_consistency(0.03, min_edge=0.1, group_share=0.6)
    assert calls[-1][1] == dict(distance_threshold=0.03, min_edge=0.1, group_share=0.6)
    p = inspect.signature(P.RegistrationPipeline.filter_matches_by_consistency).parameters
    assert (p["min_edge"].default, p["group_share"].default) == (None, 0.4)


def test_command_line_flag_reaches_the_stage_and_is_off_by_default(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import register_point_clouds as cli
    finally:
        sys.path.pop(0)
    base = ["scan.ply", "ref.ply", "--radius", "0.1", "--icp", "none"]
    assert cli.parse_args(base).consistency is None
    assert cli.parse_args(base + ["--consistency", "0.02"]).consistency == 0.02
    order = []

    class Bare:
        """A pipeline WITHOUT the stage: main() must not touch it unless the flag is given."""

        def __init__(self, **kw):
            self.matches = (np.arange(3), np.arange(3))

        def select_keypoints(self, *a, **kw):
            pass

        compute_descriptors = select_keypoints

        def find_descriptors_matches(self, *a, **kw):
            order.append("match")

        def run_ransac(self, **kw):
            order.append(("ransac", kw))
            return shot_fpfh_amd.core.RigidTransform(), 0.5

        def compute_metrics_post_icp(self, *a):
            return 1.0, 1.0

    class Full(Bare):
        def filter_matches_by_consistency(self, *a, **kw):
            order.append(("consistency", a, kw))

    monkeypatch.setattr(cli, "get_data", lambda *a, **kw: (np.zeros((3, 3)), np.zeros((3, 3))))
    monkeypatch.setattr(cli, "RegistrationPipeline", Bare)
    assert cli.main(base) == 0
    assert [o if isinstance(o, str) else o[0] for o in order] == ["match", "ransac"]
    plain = order[-1][1]
    with pytest.raises(AttributeError):
        cli.main(base + ["--consistency", "0.02"])
    monkeypatch.setattr(cli, "RegistrationPipeline", Full)
    del order[:]
    assert cli.main(base) == 0
    assert [o if isinstance(o, str) else o[0] for o in order] == ["match", "ransac"]
    del order[:]
    assert cli.main(base + ["--consistency", "0.02"]) == 0
    assert [o if isinstance(o, str) else o[0] for o in order] == ["match", "consistency", "ransac"]
    assert order[1][1:] == ((0.02,), {}) and order[2][1] == plain  # run_ransac gets what it got without the flag
