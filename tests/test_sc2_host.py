"""Host side of second_order_consistency_filter: the NumPy statement of the definition (tests/sc2_numpy.py) against plain loops
over the triples, and the public call's results, arguments, cap, exports, pipeline stage and command-line flag -- on a stand-in
engine that answers the K14 call from the statement."""
import inspect
import math
import os
import sys

import numpy as np
import pytest

import consistency_numpy as C
import ransac_numpy as N
import sc2_numpy as S
from fake_engine import FakeArray, FakeEngine

import shot_fpfh_amd
import shot_fpfh_amd.matching as matching
import shot_fpfh_amd.matching.sc2 as G
from shot_fpfh_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.01


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


def _brute_group(a, b, thr, edge, share):
    m = a.shape[0]
    c = [[1 if _brute_compat(a, b, i, j, thr, edge) else 0 for j in range(m)] for i in range(m)]
    sc2 = [[c[i][j] * sum(c[i][k] * c[j][k] for k in range(m)) for j in range(m)] for i in range(m)]
    s2 = [sum(sc2[i]) for i in range(m)]
    triangles = [sum(1 for j in range(m) for k in range(m) if c[i][j] and c[i][k] and c[j][k]) for i in range(m)]
    assert s2 == triangles  # the pairs (j, k) compatible with i and with each other
    out = dict(c=np.array(c, dtype=np.uint8), s2=np.array(s2, dtype=np.uint32))
    if m < 3:
        return dict(out, status=S.STATUS_TOO_FEW, seed=-1, keep=[])
    seed = min(i for i in range(m) if s2[i] == max(s2))
    if s2[seed] == 0:
        return dict(out, status=S.STATUS_NO_TRIPLE, seed=-1, keep=[])
    member = [1 if j == seed or c[seed][j] else 0 for j in range(m)]
    row = sc2[seed]
    top = max(row)
    keep = [j for j in range(m) if j == seed or (row[j] >= 1 and float(row[j]) >= share * float(top))]
    gdeg = [sum(c[i][j] for j in range(m) if member[j]) for i in range(m)]
    return dict(out, status=S.STATUS_OK, seed=seed, member=np.array(member, dtype=np.uint8), g=sum(member),
                row=np.array(row, dtype=np.uint32), gdeg=np.array(gdeg, dtype=np.uint32), keep=keep)


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
    out["three"] = (a[:3], a[:3] + 1.0, THR, THR)
    return out


SMALL = _small_sets()


@pytest.mark.parametrize("share", [0.5, 1.0])
@pytest.mark.parametrize("name", list(SMALL), ids=str)
def test_statement_equals_loops_over_the_triples(name, share):
    a, b, thr, edge = SMALL[name]
    want = _brute_group(a, b, thr, edge, share)
    got = S.group(a, b, thr, edge, share)
    cmat = S.compat_matrix(a, b, thr, edge, chunk=7)
    assert np.array_equal(cmat, want["c"]) and np.array_equal(cmat, cmat.T) and not np.diagonal(cmat).any()
    assert np.array_equal(S.second_order(cmat)[0], want["s2"])
    assert got["status"] == want["status"] == S.STATUS_OK and got["seed"] == want["seed"] and list(got["keep"]) == want["keep"]
    assert got["seed_score"] == int(want["s2"][want["seed"]]) and got["g"] == want["g"]
    for key, other in (("second_degree", "s2"), ("member", "member"), ("seed_row", "row"), ("group_degree", "gdeg")):
        assert got[key].dtype == want[other].dtype and np.array_equal(got[key], want[other]), key
    # group_degree is K13's, and the seed's row is one less inside the group: what the public call relies on
    assert np.array_equal(got["group_degree"], C.degree(a, b, thr, edge, member=got["member"]))
    inside = got["member"].astype(bool)
    inside[got["seed"]] = False
    assert np.array_equal(got["seed_row"][inside], got["group_degree"][inside] - 1) and not got["seed_row"][~inside].any()
    if name == "nan row":
        assert got["second_degree"][5] == 0 and not cmat[5].any() and not cmat[:, 5].any()
    if name == "tie":  # rows 5 .. 39 are a clique of 35: (35 - 1)(35 - 2) each, the lowest is the seed
        assert (got["second_degree"][5:] == 34 * 33).all() and got["seed"] == 5 and list(got["keep"]) == list(range(5, 40))


def test_second_order_of_a_matrix_that_is_not_symmetric():
    cmat = (np.random.default_rng(3).random((23, 23)) < 0.5).astype(np.uint8)
    want = [sum(int(cmat[i, j]) * sum(int(cmat[i, k]) * int(cmat[j, k]) for k in range(23)) for j in range(23)) for i in range(23)]
    s2, sc2 = S.second_order(cmat)
    assert s2.dtype == np.uint32 and list(s2) == want and sc2.shape == (23, 23)
    with pytest.raises(AssertionError):
        S.second_order(cmat * 2)  # 0 / 1 only


def test_corners_of_the_statement():
    one = np.zeros((2, 3))
    for n in (0, 1, 2):
        out = S.group(one[:n], one[:n], THR)
        assert out["status"] == S.STATUS_TOO_FEW and out["keep"].size == 0 and out["second_degree"].shape == (n,)
    # two compatible pairs that no third match joins: K13 finds a group, there is no triangle
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    b = a.copy()
    b[2:] += [0.0, 5.0, 0.0]
    out = S.group(a, b, THR)
    assert C.group(a, b, THR)["status"] == C.STATUS_OK
    assert out["status"] == S.STATUS_NO_TRIPLE and out["seed"] == -1 and out["keep"].size == 0 and not out["member"].any()
    out = S.group(a, a + 1.0, THR)  # a clique of four: (4 - 1)(4 - 2) each
    assert out["status"] == S.STATUS_OK and out["seed"] == 0 and out["g"] == 4 and list(out["second_degree"]) == [6] * 4
    assert list(out["keep"]) == [0, 1, 2, 3] and list(out["seed_row"]) == [0, 2, 2, 2]


def test_statement_keeps_exactly_the_true_matches_where_the_first_order_filter_has_to_be_lucky():
    """(2000, 0.05, 2) of the issue's table: 87 true matches, s2 of the true ones at least 7490, of the false ones at most 1042."""
    m, share, seed = 2000, 0.05, 2
    sk, rk, si, ri = N.synthetic_matches(m, share, seed=seed)[:4]
    true, replayed = C.synthetic_truth(m, share, seed)
    assert np.array_equal(replayed, sk)
    kept_s, kept_r, out = S.second_order_consistency_filter(si, ri, sk, rk, THR)
    is_true = np.zeros(m, dtype=bool)
    is_true[true] = True
    s2 = out["second_degree"]
    assert (true.size, int(s2[is_true].min()), int(s2[~is_true].max())) == (87, 7490, 1042)
    assert np.array_equal(out["keep"], true) and np.array_equal(kept_s, si[true]) and np.array_equal(kept_r, ri[true])


# ---- 2. the public call on a stand-in engine ----------------------------------------------------------------------------------------
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
    """FakeEngine + the call second_order_consistency_filter makes, answered by the NumPy statement."""

    def __init__(self, fail=None):
        self.fail, self.calls = fail, []

    def empty(self, shape, dtype=np.float64):
        if self.fail == "empty" and np.dtype(dtype) == np.uint8:
            raise MemoryError("no room for the members")
        return _Tracked(shape, dtype)

    def consistency_sc2_group_device(self, a, b, m, thr, edge, s2, member, group_degree):
        if self.fail == "group":
            raise RuntimeError("device call failed")
        self.calls.append((m, thr, edge))
        out = S.group(a.a[:m], b.a[:m], thr, edge)
        s2.a[:m], member.a[:m], group_degree.a[:m] = out["second_degree"], out["member"], out["group_degree"]
        info = np.array([out["seed"], out["seed_score"], out["g"], 0 if out["status"] == S.STATUS_OK else 1], dtype=np.int64)
        return s2, member, group_degree, info


@pytest.fixture(scope="module")
def matches():
    return N.synthetic_matches(600, 0.1, seed=5)


def test_exports_signature_and_abi_table():
    assert shot_fpfh_amd.second_order_consistency_filter is G.second_order_consistency_filter is matching.second_order_consistency_filter
    assert shot_fpfh_amd.SecondOrderRecord is matching.SecondOrderRecord is G.SecondOrderRecord
    for name in ("second_order_consistency_filter", "SecondOrderRecord"):
        assert name in shot_fpfh_amd.__all__ and name in matching.__all__ and name in G.__all__
    assert G.SC2_MAX_MATCHES == shot_fpfh_amd.Engine.SC2_MAX_MATCHES == S.MAX_MATCHES == 32768
    assert shot_fpfh_amd.Engine.SC2_TILE == S.TILE and [shot_fpfh_amd.Engine.sc2_padded(m) for m in (0, 1, 256, 257)] == [0, 256, 256, 512]
    p = inspect.signature(G.second_order_consistency_filter).parameters
    names = list(p)
    assert names == ["scan_descriptors_indices", "ref_descriptors_indices", "scan_keypoints", "ref_keypoints", "distance_threshold",
                     "min_edge", "group_share", "verbose", "engine"]
    assert all(p[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:4])
    assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[4:])
    assert p["distance_threshold"].default is inspect.Parameter.empty
    assert tuple(p[n].default for n in ("min_edge", "group_share", "verbose", "engine")) == (None, 0.5, False, None)
    assert set(G.SecondOrderRecord.__dataclass_fields__) == {"status", "seed", "seed_score", "group_size", "keep", "second_degree", "seed_row"}
    header = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    for name, n_args in (("sf_consistency_matrix", 7), ("sf_consistency_sc2", 4), ("sf_consistency_sc2_group", 10)):
        assert name in _ffi.SIGNATURES and f"int {name}(" in header and len(_ffi.SIGNATURES[name][1]) == n_args
    assert "#define SF_SC2_MAX_MATCHES 32768" in header and f"#define SF_SC2_TILE {S.TILE}" in header
    for method in ("consistency_matrix", "consistency_sc2", "consistency_sc2_group_device"):
        assert callable(getattr(shot_fpfh_amd.Engine, method))
    source = open(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "consistency.hip")).read()
    assert "__builtin_amdgcn_mfma_i32_32x32x32_i8" in source and "k14_sc2" in source and "k14_matrix" in source
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "sf_consistency_sc2" in text and "K14" in text, doc
    # the stage that was there keeps its shape
    assert inspect.signature(matching.geometric_consistency_filter).parameters["group_share"].default == 0.4


@pytest.mark.parametrize("kw", [dict(distance_threshold=-1e-3), dict(distance_threshold=float("nan")), dict(distance_threshold=float("inf")),
                                dict(min_edge=-1.0), dict(min_edge=float("nan")), dict(min_edge=float("inf")), dict(group_share=0.0),
                                dict(group_share=1.5), dict(group_share=-0.1), dict(group_share=float("nan"))])
def test_bad_arguments_raise_before_any_device_work(matches, kw):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    eng = _Engine()
    with pytest.raises(ValueError):
        G.second_order_consistency_filter(si, ri, sk, rk, **{"distance_threshold": THR, "engine": eng, **kw})
    assert _Tracked.live == before and not eng.calls
    with pytest.raises(TypeError):
        G.second_order_consistency_filter(si, ri, sk, rk, THR, engine=eng)  # the threshold is keyword-only
    with pytest.raises(ValueError):
        G.second_order_consistency_filter(si, ri[:-1], sk, rk, distance_threshold=THR, engine=eng)


def test_more_matches_than_the_cap_are_refused_before_any_device_work(matches):
    sk, rk = matches[:2]
    eng = _Engine()
    before = _Tracked.live
    idx = np.zeros(G.SC2_MAX_MATCHES + 1, dtype=np.int64)
    with pytest.raises(ValueError, match="ratio_test_matching|geometric_consistency_filter") as err:
        G.second_order_consistency_filter(idx, idx, sk, rk, distance_threshold=THR, engine=eng)
    assert "32768" in str(err.value) and _Tracked.live == before and not eng.calls


def test_result_follows_the_numpy_statement(matches):
    sk, rk, si, ri = matches[:4]
    eng = _Engine()
    kept_s, kept_r, rec = G.second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    want = S.second_order_consistency_filter(si, ri, sk, rk, THR)
    assert eng.calls == [(600, THR, THR)]  # min_edge defaults to the threshold
    assert np.array_equal(kept_s, want[0]) and np.array_equal(kept_r, want[1]) and kept_s.dtype == si.dtype
    assert (rec.status, rec.seed, rec.seed_score, rec.group_size) == ("done", want[2]["seed"], want[2]["seed_score"], want[2]["g"])
    assert np.array_equal(rec.keep, want[2]["keep"]) and rec.keep.dtype == np.int64 and np.all(np.diff(rec.keep) > 0)
    assert rec.second_degree.dtype == rec.seed_row.dtype == np.uint32
    assert np.array_equal(rec.second_degree, want[2]["second_degree"]) and np.array_equal(rec.seed_row, want[2]["seed_row"])
    assert np.array_equal(rec.keep, C.synthetic_truth(600, 0.1, 5)[0])
    # every share follows the statement, a stricter one keeps a subset, min_edge reaches the engine
    for share in (0.05, 0.4, 0.9, 1.0):
        got = G.second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, min_edge=0.05, group_share=share, engine=eng)
        assert eng.calls[-1] == (600, THR, 0.05)
        assert np.array_equal(got[2].keep, S.second_order_consistency_filter(si, ri, sk, rk, THR, 0.05, share)[2]["keep"])
        assert got[2].seed in got[2].keep
    loose = G.second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, group_share=0.05, engine=eng)[2].keep
    strict = G.second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, group_share=1.0, engine=eng)[2].keep
    assert set(strict) <= set(rec.keep) <= set(loose)


def test_too_few_matches_and_no_triple_return_empty(matches):
    sk, rk, si, ri = matches[:4]
    for n in (0, 1, 2):
        eng = _Engine()
        kept_s, kept_r, rec = G.second_order_consistency_filter(si[:n], ri[:n], sk, rk, distance_threshold=THR, engine=eng)
        assert kept_s.size == kept_r.size == rec.keep.size == 0 and rec.status == "fewer than three matches" and not eng.calls
        assert rec.second_degree.shape == rec.seed_row.shape == (n,) and rec.seed == -1 and rec.group_size == 0
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    b = a.copy()
    b[2:] += [0.0, 5.0, 0.0]
    kept_s, kept_r, rec = G.second_order_consistency_filter(np.arange(4), np.arange(4), a, b, distance_threshold=THR, engine=_Engine())
    assert kept_s.size == kept_r.size == 0 and rec.status == "no consistent triple" and rec.seed == -1
    assert not rec.second_degree.any() and not rec.seed_row.any() and rec.group_size == 0


@pytest.mark.parametrize("fail", ["empty", "group", "index"])
def test_device_buffers_are_freed_on_every_error_path(matches, fail):
    sk, rk, si, ri = matches[:4]
    before = _Tracked.live
    if fail == "index":
        with pytest.raises(IndexError):
            G.second_order_consistency_filter(si + 600, ri, sk, rk, distance_threshold=THR, engine=_Engine())
    else:
        with pytest.raises((MemoryError, RuntimeError)):
            G.second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=_Engine(fail))
    assert _Tracked.live == before
    G.second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=_Engine())
    assert _Tracked.live == before


# ---- 3. pipeline and command line ---------------------------------------------------------------------------------------------------
def test_pipeline_stage_replaces_the_matches(monkeypatch, caplog):
    import shot_fpfh_amd.pipeline as P

    calls = []

    def fake(*args, **kw):
        calls.append((args, kw))
        return args[0][1:3], args[1][1:3], G.SecondOrderRecord(group_size=3, keep=np.array([1, 2]))

    monkeypatch.setattr(P, "second_order_consistency_filter", fake)
    pipe = P.RegistrationPipeline.__new__(P.RegistrationPipeline)
    pipe.scan, pipe.ref = np.zeros((4, 3)), np.ones((4, 3))
    pipe.scan_keypoints = pipe.ref_keypoints = np.arange(4)
    pipe.matches = (np.arange(4), np.arange(4)[::-1])
    with caplog.at_level("INFO"):
        assert pipe.filter_matches_by_second_order_consistency(0.02) is None
    args, kw = calls[-1]
    assert len(args) == 4 and np.array_equal(args[1], np.arange(4)[::-1]) and np.array_equal(args[3], np.ones((4, 3)))
    assert kw == dict(distance_threshold=0.02, min_edge=None, group_share=0.5)
    assert np.array_equal(pipe.matches[0], [1, 2]) and np.array_equal(pipe.matches[1], [2, 1])
    assert "2 matches kept out of 4" in caplog.text
    pipe.filter_matches_by_second_order_consistency(0.03, min_edge=0.1, group_share=0.6)
    assert calls[-1][1] == dict(distance_threshold=0.03, min_edge=0.1, group_share=0.6)
    p = inspect.signature(P.RegistrationPipeline.filter_matches_by_second_order_consistency).parameters
    assert (p["min_edge"].default, p["group_share"].default) == (None, 0.5)


def test_command_line_flag_reaches_the_stage_and_is_off_by_default(monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import register_point_clouds as cli
    finally:
        sys.path.pop(0)
    base = ["scan.ply", "ref.ply", "--radius", "0.1", "--icp", "none"]
    assert cli.parse_args(base).consistency_sc2 is None and cli.parse_args(base).consistency is None
    args = cli.parse_args(base + ["--consistency-sc2", "0.02"])
    assert args.consistency_sc2 == 0.02 and args.consistency is None
    with pytest.raises(SystemExit):  # one filter or the other
        cli.parse_args(base + ["--consistency", "0.02", "--consistency-sc2", "0.02"])
    assert "not allowed with" in capsys.readouterr().err
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

        def filter_matches_by_second_order_consistency(self, *a, **kw):
            order.append(("sc2", a, kw))

    monkeypatch.setattr(cli, "get_data", lambda *a, **kw: (np.zeros((3, 3)), np.zeros((3, 3))))
    monkeypatch.setattr(cli, "RegistrationPipeline", Bare)
    assert cli.main(base) == 0
    assert [o if isinstance(o, str) else o[0] for o in order] == ["match", "ransac"]
    plain = order[-1][1]
    with pytest.raises(AttributeError):
        cli.main(base + ["--consistency-sc2", "0.02"])
    monkeypatch.setattr(cli, "RegistrationPipeline", Full)
    del order[:]
    assert cli.main(base + ["--consistency-sc2", "0.02"]) == 0
    assert [o if isinstance(o, str) else o[0] for o in order] == ["match", "sc2", "ransac"]
    assert order[1][1:] == ((0.02,), {}) and order[2][1] == plain  # run_ransac gets what it got without the flag
    del order[:]
    assert cli.main(base + ["--consistency", "0.02"]) == 0
    assert [o if isinstance(o, str) else o[0] for o in order] == ["match", "consistency", "ransac"]
