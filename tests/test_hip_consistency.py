"""The geometric-consistency filter on the MI355X (K13, csrc/consistency.hip) against the NumPy statement of the definition
(tests/consistency_numpy.py).  Every output is an integer or a boolean decided in float64, so every comparison here is exact."""
import numpy as np
import pytest

import consistency_numpy as C
import ransac_numpy as N
from shot_fpfh_amd import ShotFpfhError, _ffi
from shot_fpfh_amd.matching import fast_global_registration, geometric_consistency_filter

pytestmark = pytest.mark.gpu

THR = 0.01
CAP = 2e-3  # test_hip_fgr.CAP: what fast_global_registration is held to on the sets it recovers
TILE, BLOCK = 128, 256  # K13_TILE columns per LDS tile, K13_BLOCK rows per block (csrc/consistency.hip)
FGR_FAILS = (5000, 0.10, 5010)  # the set fast_global_registration does not converge on (m + 100 share as the seed)
SETS = [(2000, 0.05, 2), (2000, 0.30, 3), FGR_FAILS, "duplicates", "lattice", "tie", "nan row", "float32"]
_sets, _groups = {}, {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _set(name):
    """(a, b, distance_threshold, min_edge) of a named set."""
    if name not in _sets:
        if isinstance(name, tuple):
            sk, rk, si, ri = N.synthetic_matches(name[0], name[1], seed=name[2])[:4]
            _sets[name] = (*N.matched_points(si, ri, sk, rk), THR, THR)
        elif name == "duplicates":  # test_hip_fgr's: 40 distinct reference keypoints for 4000 matches, dq = 0 for many pairs
            sk, rk, si, ri = N.synthetic_matches(4000, 0.5, seed=11)[:4]
            ri = ri[np.random.default_rng(3).integers(0, 40, 4000)]
            _sets[name] = (*N.matched_points(si[:1500], ri[:1500], sk, rk), THR, THR)
        elif name == "lattice":
            _sets[name] = C.lattice_set(700, seed=3)
        elif name == "tie":
            _sets[name] = C.tie_set(600, junk=130, seed=4)  # the tied rows start in the second tile
        elif name == "nan row":
            a, b = (x.copy() for x in _set((2000, 0.30, 3))[:2])
            a[1234, 2], b[77] = np.nan, np.inf
            _sets[name] = (a[:1500], b[:1500], THR, THR)
        elif name == "float32":
            a, b = _set((2000, 0.05, 2))[:2]
            _sets[name] = (a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64), THR, THR)
    return _sets[name]


def _group(name):
    """The statement's group of a named set, computed once."""
    if name not in _groups:
        _groups[name] = C.group(*_set(name))
    return _groups[name]


class _Resident:
    def __init__(self, eng, a, b):
        self.m = a.shape[0]
        self.eng, self.held = eng, [eng.empty((max(self.m, 1), 3)), eng.empty((max(self.m, 1), 3))]
        self.da, self.db = self.held
        if self.m:
            self.da.from_host(a), self.db.from_host(b)

    def array(self, dtype, values=None):
        d = self.eng.empty((max(self.m, 1),), dtype)
        self.held.append(d)
        return d if values is None else d.from_host(np.asarray(values, dtype=dtype))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in self.held:
            h.free()


# ---- degree -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, TILE - 1, TILE, TILE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + TILE + 5])
def test_degree_is_exact_at_the_tile_and_block_sizes(eng, m):
    """One column, a ragged tile, a full tile and one column into the next slice; one row into the second row block; a ragged
    last row block together with a ragged last column slice."""
    a, b = (x[:m] for x in _set((2000, 0.30, 3))[:2])
    with _Resident(eng, a, b) as dev:
        got = eng.consistency_degree(dev.da, dev.db, m, THR, THR)
    assert got.dtype == np.uint32 and got.shape == (m,)
    assert np.array_equal(got, C.degree(a, b, THR, THR))
    assert m < 3 * BLOCK or got.max() > 10


def test_degree_is_exact_where_a_slice_holds_several_tiles(eng):
    """m = 11 600 is past the size at which row blocks x tiles exceeds the grid's target: a slice then loops over two tiles and the
    last slice ends early.  The statement is evaluated on the whole ragged last row block and on 256 other rows."""
    m = 11600
    sk, rk, si, ri = N.synthetic_matches(m, 0.2, seed=21)[:4]
    a, b = N.matched_points(si, ri, sk, rk)
    rows = np.unique(np.concatenate([np.arange((m // BLOCK) * BLOCK, m), np.random.default_rng(1).integers(0, m, 256), [0, TILE, BLOCK]]))
    with _Resident(eng, a, b) as dev:
        got = eng.consistency_degree(dev.da, dev.db, m, THR, THR)
        mask = np.random.default_rng(2).random(m) < 0.5
        got_masked = eng.consistency_degree(dev.da, dev.db, m, THR, THR, member=dev.array(np.uint8, mask))
    ok = C.compat_rows(a, b, rows, THR, THR)
    assert np.array_equal(got[rows], np.count_nonzero(ok, axis=1))
    assert np.array_equal(got_masked[rows], np.count_nonzero(ok & mask[None, :], axis=1))
    assert int(got.sum(dtype=np.int64)) % 2 == 0 and got.max() > 2000  # compat is symmetric


@pytest.mark.parametrize("name", SETS, ids=str)
def test_degree_is_exact_on_the_sets(eng, name):
    a, b, thr, edge = _set(name)
    want = _group(name)
    m = a.shape[0]
    with _Resident(eng, a, b) as dev:
        got = eng.consistency_degree(dev.da, dev.db, m, thr, edge)
        assert np.array_equal(got, want["degree"])
        assert np.array_equal(got, eng.consistency_degree(dev.da, dev.db, m, thr, edge))  # two calls, bit for bit
        # the statement's own member mask, and an all-zero mask
        assert np.array_equal(eng.consistency_degree(dev.da, dev.db, m, thr, edge, member=dev.array(np.uint8, want["member"])),
                              want["group_degree"])
        assert not eng.consistency_degree(dev.da, dev.db, m, thr, edge, member=dev.array(np.uint8, np.zeros(m))).any()
    if name == "nan row":
        assert got[1234] == 0 and got[77] == 0 and got.max() > 100
    if name == "duplicates":  # matches that share their reference keypoint never vote for each other
        assert np.count_nonzero(C.lengths(b, np.arange(50)) == 0) > 1000


def test_degree_with_a_random_mask_and_another_min_edge(eng):
    a, b, thr, _ = _set("duplicates")
    m = a.shape[0]
    mask = np.random.default_rng(8).random(m) < 0.3
    with _Resident(eng, a, b) as dev:
        dmask = dev.array(np.uint8, mask * 255)  # any non-zero byte is a member
        for edge in (0.0, thr, 0.2):
            assert np.array_equal(eng.consistency_degree(dev.da, dev.db, m, thr, edge, member=dmask), C.degree(a, b, thr, edge, member=mask))


# ---- the chain --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS, ids=str)
def test_chain_equals_the_statement(eng, name):
    a, b, thr, edge = _set(name)
    want = _group(name)
    m = a.shape[0]
    with _Resident(eng, a, b) as dev:
        out = [dev.array(np.uint32), dev.array(np.uint8), dev.array(np.uint32)]
        before = eng.lib.sf_sync_count()
        ddeg, dmem, dgdeg, info = eng.consistency_group_device(dev.da, dev.db, m, thr, edge, *out)
        assert eng.lib.sf_sync_count() - before == 1  # five launches, ONE host wait
        first = (ddeg.to_host(), dmem.to_host(), dgdeg.to_host(), info.copy())
        eng.consistency_group_device(dev.da, dev.db, m, thr, edge, *out)
        for x, y in zip(first, (ddeg.to_host(), dmem.to_host(), dgdeg.to_host(), info)):
            assert np.array_equal(x, y)  # a second call, bit for bit
    assert want["status"] == C.STATUS_OK
    assert list(first[3]) == [want["seed"], want["seed_degree"], want["g"], 0]
    for got, key in zip(first[:3], ("degree", "member", "group_degree")):
        assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), key
    idx = np.arange(m)
    kept_s, kept_r, rec = geometric_consistency_filter(idx, idx[::-1], a, b[::-1], distance_threshold=thr, min_edge=edge, engine=eng)
    assert np.array_equal(rec.keep, want["keep"]) and np.array_equal(kept_s, want["keep"]) and np.array_equal(kept_r, m - 1 - want["keep"])
    assert (rec.status, rec.seed, rec.group_size) == ("done", want["seed"], want["g"])
    assert np.array_equal(rec.degree, want["degree"]) and np.array_equal(rec.group_degree, want["group_degree"])
    if name == "tie":  # rows 130 .. 599 share the maximum: the lowest of them is the seed
        assert want["seed"] == 130 and np.count_nonzero(want["degree"] == want["seed_degree"]) == 470


def test_no_compatible_pair_and_fewer_than_two_matches(eng):
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [0, 2.0, 0]])
    with _Resident(eng, a, 3.0 * a) as dev:
        out = [dev.array(np.uint32, [7, 7, 7]), dev.array(np.uint8, [7, 7, 7]), dev.array(np.uint32, [7, 7, 7])]
        ddeg, dmem, dgdeg, info = eng.consistency_group_device(dev.da, dev.db, 3, THR, THR, *out)
        assert list(info) == [-1, 0, 0, 1] and not ddeg.to_host().any() and not dmem.to_host().any() and not dgdeg.to_host().any()
        ddeg, dmem, dgdeg, info = eng.consistency_group_device(dev.da, dev.db, 1, THR, THR, *out)  # one match: no pair either
        assert list(info) == [-1, 0, 0, 1]
        assert eng.consistency_degree(dev.da, dev.db, 0, THR, THR).shape == (0,)
        assert list(eng.consistency_group_device(dev.da, dev.db, 0, THR, THR, *out)[3]) == [-1, 0, 0, 1]
    idx = np.arange(3)
    kept_s, kept_r, rec = geometric_consistency_filter(idx, idx, a, 3.0 * a, distance_threshold=THR, engine=eng)
    assert kept_s.size == kept_r.size == 0 and rec.status == "no consistent pair" and rec.seed == -1
    for n in (0, 1):
        kept_s, kept_r, rec = geometric_consistency_filter(idx[:n], idx[:n], a, a, distance_threshold=THR, engine=eng)
        assert kept_s.size == kept_r.size == 0 and rec.status == "fewer than two matches"


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------
def test_filter_keeps_the_true_matches_and_fgr_then_converges(eng):
    m, share, seed = FGR_FAILS
    sk, rk, si, ri, r0, t0 = N.synthetic_matches(m, share, seed=seed)
    true, replayed = C.synthetic_truth(m, share, seed)
    assert np.array_equal(replayed, sk)
    kept_s, kept_r, rec = geometric_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    assert np.array_equal(rec.keep, true) and np.array_equal(kept_s, si[true]) and np.array_equal(kept_r, ri[true])
    _, tf, _ = fast_global_registration(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    print(f"{FGR_FAILS}: all {m} matches: |R - R0| = {np.linalg.norm(tf.rotation - r0):.3e}, |t - t0| = {np.linalg.norm(tf.translation - t0):.3e}")
    ratio, tf, _ = fast_global_registration(kept_s, kept_r, sk, rk, distance_threshold=THR, engine=eng)
    er, et = float(np.linalg.norm(tf.rotation - r0)), float(np.linalg.norm(tf.translation - t0))
    print(f"{FGR_FAILS}: the {kept_s.size} kept: |R - R0| = {er:.3e}, |t - t0| = {et:.3e}, inlier ratio {ratio:.4f}")
    assert er <= CAP and et <= CAP


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    a, b = (x[:300] for x in _set((2000, 0.30, 3))[:2])
    nan, inf = float("nan"), float("inf")
    with _Resident(eng, a, b) as dev:
        out = [dev.array(np.uint32), dev.array(np.uint8), dev.array(np.uint32)]
        for thr, edge in ((-1e-3, THR), (nan, THR), (inf, THR), (THR, -1e-3), (THR, nan), (THR, inf)):
            with pytest.raises(ShotFpfhError, match="sf_consistency_degree"):
                eng.consistency_degree(dev.da, dev.db, 300, thr, edge)
            with pytest.raises(ShotFpfhError, match="sf_consistency_group"):
                eng.consistency_group_device(dev.da, dev.db, 300, thr, edge, *out)
        info = np.zeros(4, dtype=np.int64)
        ip = info.ctypes.data
        deg, mem, gdeg = (x.ptr for x in out)
        for m in (-1, 2**31):  # refused before anything is read
            assert eng.lib.sf_consistency_degree(eng.h, dev.da.ptr, dev.db.ptr, m, None, THR, THR, deg) == -1
            assert "sf_consistency_degree" in _ffi.last_error()
            assert eng.lib.sf_consistency_group(eng.h, dev.da.ptr, dev.db.ptr, m, THR, THR, deg, mem, gdeg, ip) == -1
        for args in ((None, dev.db.ptr, 300, None, THR, THR, deg), (dev.da.ptr, None, 300, None, THR, THR, deg),
                     (dev.da.ptr, dev.db.ptr, 300, None, THR, THR, None)):
            with pytest.raises(ShotFpfhError):
                _ffi.check(eng.lib.sf_consistency_degree(eng.h, *args), "sf_consistency_degree")
        full = [dev.da.ptr, dev.db.ptr, 300, THR, THR, deg, mem, gdeg, ip]
        for hole in (0, 1, 5, 6, 7, 8):
            args = list(full)
            args[hole] = None
            with pytest.raises(ShotFpfhError):
                _ffi.check(eng.lib.sf_consistency_group(eng.h, *args), "sf_consistency_group")
        with pytest.raises(ShotFpfhError):
            _ffi.check(eng.lib.sf_consistency_degree(None, dev.da.ptr, dev.db.ptr, 300, None, THR, THR, deg), "sf_consistency_degree")
        # the engine checks the buffers it is handed
        with pytest.raises(ValueError):
            eng.consistency_degree(dev.da, dev.db, 301, THR, THR)
        with pytest.raises(ValueError):
            eng.consistency_group_device(dev.da, dev.db, 300, THR, THR, out[0], out[2], out[2])
        assert not info.any()
