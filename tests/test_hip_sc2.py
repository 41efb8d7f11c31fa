"""Second-order consistency on the MI355X (K14, csrc/consistency.hip) against the NumPy statement of the definition
(tests/sc2_numpy.py).  Every output is an integer, so every comparison here is exact: there is no tolerance anywhere."""
import numpy as np
import pytest

import consistency_numpy as C
import ransac_numpy as N
import sc2_numpy as S
from shot_fpfh_amd import ShotFpfhError, _ffi
from shot_fpfh_amd.matching import fast_global_registration, second_order_consistency_filter

pytestmark = pytest.mark.gpu

THR = 0.01
CAP = 2e-3  # test_hip_fgr.CAP: what fast_global_registration is held to on the sets it recovers
T = 256     # K14_T = SF_SC2_TILE: outputs of a workgroup of k14_sc2 along either axis, and the padding of the matrix
KC = 64     # K14_KC: bytes of K per step of its main loop
SIZES = [1, 2, 3, 31, 32, 33, KC - 1, KC, KC + 1, T - 1, T, T + 1, 2 * T + 37]
CHAIN_SETS = [(2000, 0.05, 2), (5000, 0.01, 4), "lattice", "tie", "nan row", "float32"]
_sets, _groups = {}, {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _set(name):
    """(a, b, distance_threshold, min_edge) of a named set (the sets of test_hip_consistency)."""
    if name not in _sets:
        if isinstance(name, tuple):
            sk, rk, si, ri = N.synthetic_matches(name[0], name[1], seed=name[2])[:4]
            _sets[name] = (*N.matched_points(si, ri, sk, rk), THR, THR)
        elif name == "duplicates":  # 40 distinct reference keypoints for the matches: dq = 0 for many pairs
            sk, rk, si, ri = N.synthetic_matches(4000, 0.5, seed=11)[:4]
            ri = ri[np.random.default_rng(3).integers(0, 40, 4000)]
            _sets[name] = (*N.matched_points(si[:1500], ri[:1500], sk, rk), THR, THR)
        elif name == "lattice":
            _sets[name] = C.lattice_set(700, seed=3)
        elif name == "tie":
            _sets[name] = C.tie_set(600, junk=130, seed=4)
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
        _groups[name] = S.group(*_set(name))
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


def _padded_on_device(eng, cmat):
    """A host (m, m) 0/1 matrix in the device's layout: sc2_padded(m) on either edge, the padding zero."""
    m = cmat.shape[0]
    pad = eng.sc2_padded(m)
    host = np.zeros((pad, pad), dtype=np.uint8)
    host[:m, :m] = cmat
    return eng.empty((pad, pad), np.uint8).from_host(host)


# ---- sf_consistency_sc2 alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", SIZES)
def test_sc2_of_a_random_matrix_that_is_not_symmetric(eng, m):
    """One row, one MFMA block and its neighbours, the K-chunk and the workgroup tile with one less and one more, several tiles
    with ragged edges.  A matrix that is not symmetric tells C C^T from C^T C and C C, and a transposed accumulator layout from
    the right one."""
    assert eng.sc2_padded(1) == T and eng.sc2_padded(T + 1) == 2 * T and eng.sc2_padded(0) == 0
    cmat = (np.random.default_rng(100 + m).random((m, m)) < 0.5).astype(np.uint8)
    assert m < 3 or not np.array_equal(cmat, cmat.T)
    c64 = cmat.astype(np.int64)
    want = ((c64 @ c64.T) * c64).sum(axis=1)
    dev = _padded_on_device(eng, cmat)
    try:
        got = eng.consistency_sc2(dev, m)
        again = eng.consistency_sc2(dev, m)
    finally:
        dev.free()
    assert got.dtype == np.uint32 and got.shape == (m,)
    assert np.array_equal(got.astype(np.int64), want)
    assert np.array_equal(got, again)
    assert np.array_equal(want, S.second_order(cmat)[0])  # the statement's own form of the same sum


def test_sc2_of_all_ones_at_300(eng):
    m = 300
    dev = _padded_on_device(eng, np.ones((m, m), dtype=np.uint8))
    try:
        got = eng.consistency_sc2(dev, m)
    finally:
        dev.free()
    assert np.array_equal(got, np.full(m, m * m, dtype=np.uint32))


def test_sc2_of_all_ones_at_the_cap(eng):
    """m = 32 768: a 1 GiB matrix filled on the device (1 MiB of ones, doubled ten times), every s2 = m^2 = 2^30 in closed form."""
    m = eng.SC2_MAX_MATCHES
    assert m == S.MAX_MATCHES == 32768 and eng.sc2_padded(m) == m
    piece = 1 << 20
    dev = eng.empty((m, m), np.uint8)
    ones = eng.empty((piece,), np.uint8).from_host(np.ones(piece, dtype=np.uint8))
    try:
        dev.copy_from_device(ones)
        n = piece
        while n < m * m:
            dev.copy_from_device(dev, dst_byte_offset=n, nbytes=n)
            n *= 2
        got = eng.consistency_sc2(dev, m)
        probe = dev.rows_to_host(m - 1, 1)
    finally:
        dev.free()
        ones.free()
    assert probe.min() == 1 and probe.max() == 1
    assert got.shape == (m,) and got.min() == got.max() == 2 ** 30


# ---- sf_consistency_matrix ------------------------------------------------------------------------------------------------------------
def _check_matrix(eng, a, b, thr, edge):
    m = a.shape[0]
    pad = eng.sc2_padded(m)
    with _Resident(eng, a, b) as dev:
        poison = eng.empty((pad, pad), np.uint8).from_host(np.full((pad, pad), 7, dtype=np.uint8))  # every byte must be written
        try:
            got = eng.consistency_matrix(dev.da, dev.db, m, thr, edge, out=poison).to_host()
        finally:
            poison.free()
    want = S.compat_matrix(a, b, thr, edge)
    assert got.shape == (pad, pad) and got.dtype == np.uint8
    assert np.array_equal(got[:m, :m], want)
    assert not got[m:].any() and not got[:, m:].any()
    assert np.array_equal(got, got.T) and not np.diagonal(got).any()
    return got


@pytest.mark.parametrize("m", SIZES)
def test_matrix_is_exact_at_the_ragged_sizes(eng, m):
    a, b = (x[:m] for x in _set((2000, 0.30, 3))[:2])
    got = _check_matrix(eng, a, b, THR, THR)
    assert m < 2 * T or got.sum() > 1000


@pytest.mark.parametrize("name", ["nan row", "duplicates", "lattice"])
def test_matrix_is_exact_on_the_sets(eng, name):
    a, b, thr, edge = _set(name)
    got = _check_matrix(eng, a, b, thr, edge)
    if name == "nan row":
        assert not got[1234].any() and not got[77].any() and got.sum() > 10000
    if name == "lattice":  # min_edge 0: matches on top of each other are compatible, the diagonal still is not
        _check_matrix(eng, a, b, thr, 0.0)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CHAIN_SETS, ids=str)
def test_chain_equals_the_statement(eng, name):
    a, b, thr, edge = _set(name)
    want = _group(name)
    m = a.shape[0]
    with _Resident(eng, a, b) as dev:
        out = [dev.array(np.uint32), dev.array(np.uint8), dev.array(np.uint32)]
        before = eng.lib.sf_sync_count()
        ds2, dmem, dgdeg, info = eng.consistency_sc2_group_device(dev.da, dev.db, m, thr, edge, *out)
        assert eng.lib.sf_sync_count() - before == 1  # six launches, ONE host wait
        first = (ds2.to_host(), dmem.to_host(), dgdeg.to_host(), info.copy())
        eng.consistency_sc2_group_device(dev.da, dev.db, m, thr, edge, *out)
        for x, y in zip(first, (ds2.to_host(), dmem.to_host(), dgdeg.to_host(), info)):
            assert np.array_equal(x, y)  # a second call, bit for bit
    assert want["status"] == S.STATUS_OK
    assert list(first[3]) == [want["seed"], want["seed_score"], want["g"], 0]
    for got, key in zip(first[:3], ("second_degree", "member", "group_degree")):
        assert got.dtype == want[key].dtype and np.array_equal(got, want[key]), key
    idx = np.arange(m)
    kept_s, kept_r, rec = second_order_consistency_filter(idx, idx[::-1], a, b[::-1], distance_threshold=thr, min_edge=edge, engine=eng)
    assert np.array_equal(rec.keep, want["keep"]) and np.array_equal(kept_s, want["keep"]) and np.array_equal(kept_r, m - 1 - want["keep"])
    assert (rec.status, rec.seed, rec.seed_score, rec.group_size) == ("done", want["seed"], want["seed_score"], want["g"])
    assert np.array_equal(rec.second_degree, want["second_degree"]) and np.array_equal(rec.seed_row, want["seed_row"])
    ties = np.count_nonzero(want["second_degree"] == want["seed_score"])
    if name == "lattice":  # six rows share the maximum: the lowest of them is the seed
        assert (want["seed"], ties) == (81, 6)
    if name == "tie":
        assert (want["seed"], ties) == (130, 470)
    if name == (5000, 0.01, 4):  # the set on which the first-order seed is a false match
        assert np.array_equal(rec.keep, C.synthetic_truth(5000, 0.01, 4)[0])


def test_no_consistent_triple_and_fewer_than_three_matches(eng):
    # two compatible pairs, (0, 1) and (2, 3), that no third match joins: K13 finds a group here, there is no triangle
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    b = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    b[2:] += [0.0, 5.0, 0.0]  # every length between the two pairs changes, |b2 b3| = 4 stays
    want = S.group(a, b, THR)
    assert want["status"] == S.STATUS_NO_TRIPLE and S.compat_matrix(a, b, THR).sum() == 4
    with _Resident(eng, a, b) as dev:
        out = [dev.array(np.uint32, [7] * 4), dev.array(np.uint8, [7] * 4), dev.array(np.uint32, [7] * 4)]
        ds2, dmem, dgdeg, info = eng.consistency_sc2_group_device(dev.da, dev.db, 4, THR, THR, *out)
        assert list(info) == [-1, 0, 0, 1] and not ds2.to_host().any() and not dmem.to_host().any() and not dgdeg.to_host().any()
        for n in (2, 1, 0):  # fewer than three matches: no triple either; m = 0 writes nothing
            assert list(eng.consistency_sc2_group_device(dev.da, dev.db, n, THR, THR, *out)[3]) == [-1, 0, 0, 1]
    idx = np.arange(4)
    kept_s, kept_r, rec = second_order_consistency_filter(idx, idx, a, b, distance_threshold=THR, engine=eng)
    assert kept_s.size == kept_r.size == 0 and rec.status == "no consistent triple" and rec.seed == -1 and not rec.second_degree.any()
    for n in (0, 1, 2):
        kept_s, kept_r, rec = second_order_consistency_filter(idx[:n], idx[:n], a, a, distance_threshold=THR, engine=eng)
        assert kept_s.size == kept_r.size == 0 and rec.status == "fewer than three matches" and rec.second_degree.shape == (n,)


# ---- what it is for -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(5000, 0.01, 4), (5000, 0.006, 5)], ids=str)
def test_filter_keeps_exactly_the_true_matches_at_one_per_cent(eng, case):
    m, share, seed = case
    sk, rk, si, ri = N.synthetic_matches(m, share, seed=seed)[:4]
    true, replayed = C.synthetic_truth(m, share, seed)
    assert np.array_equal(replayed, sk)
    kept_s, kept_r, rec = second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    print(f"{case}: {true.size} true, seed {rec.seed} of score {rec.seed_score}, group {rec.group_size}, kept {rec.keep.size}")
    assert np.array_equal(rec.keep, true) and np.array_equal(kept_s, si[true]) and np.array_equal(kept_r, ri[true])


def test_filter_keeps_the_true_matches_and_fgr_then_converges(eng):
    m, share, seed = 5000, 0.02, 3
    sk, rk, si, ri, r0, t0 = N.synthetic_matches(m, share, seed=seed)
    true, replayed = C.synthetic_truth(m, share, seed)
    assert np.array_equal(replayed, sk)
    kept_s, kept_r, rec = second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    assert np.array_equal(rec.keep, true) and np.array_equal(kept_s, si[true]) and np.array_equal(kept_r, ri[true])
    ratio, tf, _ = fast_global_registration(kept_s, kept_r, sk, rk, distance_threshold=THR, engine=eng)
    er, et = float(np.linalg.norm(tf.rotation - r0)), float(np.linalg.norm(tf.translation - t0))
    print(f"{(m, share, seed)}: the {kept_s.size} kept: |R - R0| = {er:.3e}, |t - t0| = {et:.3e}, inlier ratio {ratio:.4f}")
    assert er <= CAP and et <= CAP


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(eng):
    a, b = (x[:300] for x in _set((2000, 0.30, 3))[:2])
    nan, inf = float("nan"), float("inf")
    pad = eng.sc2_padded(300)
    with _Resident(eng, a, b) as dev:
        out = [dev.array(np.uint32), dev.array(np.uint8), dev.array(np.uint32)]
        cmat = eng.empty((pad, pad), np.uint8)
        dev.held.append(cmat)
        for thr, edge in ((-1e-3, THR), (nan, THR), (inf, THR), (THR, -1e-3), (THR, nan), (THR, inf)):
            with pytest.raises(ShotFpfhError, match="sf_consistency_matrix"):
                eng.consistency_matrix(dev.da, dev.db, 300, thr, edge, out=cmat)
            with pytest.raises(ShotFpfhError, match="sf_consistency_sc2_group"):
                eng.consistency_sc2_group_device(dev.da, dev.db, 300, thr, edge, *out)
        info = np.zeros(4, dtype=np.int64)
        ip = info.ctypes.data
        s2, mem, gdeg = (x.ptr for x in out)
        for m in (-1, 32769, 2 ** 31):  # refused before anything is read or allocated
            assert eng.lib.sf_consistency_matrix(eng.h, dev.da.ptr, dev.db.ptr, m, THR, THR, cmat.ptr) == -1
            assert "sf_consistency_matrix" in _ffi.last_error()
            assert eng.lib.sf_consistency_sc2(eng.h, cmat.ptr, m, s2) == -1
            assert "sf_consistency_sc2" in _ffi.last_error()
            assert eng.lib.sf_consistency_sc2_group(eng.h, dev.da.ptr, dev.db.ptr, m, THR, THR, s2, mem, gdeg, ip) == -1
            assert "sf_consistency_sc2_group" in _ffi.last_error()
        full = [dev.da.ptr, dev.db.ptr, 300, THR, THR, cmat.ptr]
        for hole in (0, 1, 5):
            args = list(full)
            args[hole] = None
            with pytest.raises(ShotFpfhError):
                _ffi.check(eng.lib.sf_consistency_matrix(eng.h, *args), "sf_consistency_matrix")
        for args in ((None, 300, s2), (cmat.ptr, 300, None)):
            with pytest.raises(ShotFpfhError):
                _ffi.check(eng.lib.sf_consistency_sc2(eng.h, *args), "sf_consistency_sc2")
        full = [dev.da.ptr, dev.db.ptr, 300, THR, THR, s2, mem, gdeg, ip]
        for hole in (0, 1, 5, 6, 7, 8):
            args = list(full)
            args[hole] = None
            with pytest.raises(ShotFpfhError):
                _ffi.check(eng.lib.sf_consistency_sc2_group(eng.h, *args), "sf_consistency_sc2_group")
        with pytest.raises(ShotFpfhError):
            _ffi.check(eng.lib.sf_consistency_sc2(None, cmat.ptr, 300, s2), "sf_consistency_sc2")
        # the engine checks the buffers it is handed
        with pytest.raises(ValueError):
            eng.consistency_matrix(dev.da, dev.db, 301, THR, THR, out=cmat)
        with pytest.raises(ValueError):
            eng.consistency_sc2(cmat, 300 + T)  # a matrix too small for the count
        with pytest.raises(ValueError):
            eng.consistency_sc2(out[0], 300)  # not bytes
        with pytest.raises(ValueError):
            eng.consistency_sc2_group_device(dev.da, dev.db, 300, THR, THR, out[0], out[2], out[2])
        assert not info.any()
    with pytest.raises(ValueError, match="ratio_test_matching"):
        idx = np.zeros(32769, dtype=np.int64)
        second_order_consistency_filter(idx, idx, a, b, distance_threshold=THR, engine=eng)
