"""SC2 registration on the MI355X (K15, csrc/consistency.hip) against the NumPy statement of the definition
(tests/sc2_registration_numpy.py).  Integers -- seeds, rows, members, sizes, statuses, counts, the winner -- are held by exact
equality; the sums of a fit by size x 2^-52 relative to the sums of absolute terms, the transforms by the polar-factor bound
64 x 2^-52 x s1 / gap that K11 is held to."""
import numpy as np
import pytest

import consistency_numpy as C
import ransac_numpy as N
import sc2_numpy as S
import sc2_registration_numpy as R
from shot_fpfh_amd import ShotFpfhError, _ffi
from shot_fpfh_amd.matching import sc2_registration, second_order_consistency_filter

pytestmark = pytest.mark.gpu

THR = 0.01
EPS = 2.0 ** -52
TS = R.SEED_TILE   # K15_TS: seeds of a workgroup of k15_seed_rows
T = S.TILE         # the column tile, and the padding of the matrix
FIT_SEEDS = 64
FIT_SETS = [(2000, 0.05, 2), "lattice", "tie", "nan row", "float32", (5000, 0.004, 1)]
_sets, _hyps, _staged = {}, {}, {}
_worst = {}


@pytest.fixture(scope="module")
def eng():
    from shot_fpfh_amd.engine import default_engine

    return default_engine()


def _set(name):
    """(a, b, distance_threshold, min_edge) of a named set (the chain sets of test_hip_sc2)."""
    if name not in _sets:
        if isinstance(name, tuple):
            sk, rk, si, ri = N.synthetic_matches(name[0], name[1], seed=name[2])[:4]
            _sets[name] = (*N.matched_points(si, ri, sk, rk), THR, THR)
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


def _hyp(name):
    """The statement's hypotheses of a named set at FIT_SEEDS seeds, computed once."""
    if name not in _hyps:
        a, b, thr, edge = _set(name)
        _hyps[name] = R.hypotheses(a, b, thr, edge, n_seeds=FIT_SEEDS)
    return _hyps[name]


class _Held:
    """Device arrays freed together."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def new(self, shape, dtype=np.float64, values=None):
        d = self.eng.empty(shape, dtype)
        self.held.append(d)
        return d if values is None else d.from_host(np.ascontiguousarray(values, dtype=dtype))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in self.held:
            h.free()


def _padded(cmat, pad):
    host = np.zeros((pad, pad), dtype=np.uint8)
    host[:cmat.shape[0], :cmat.shape[0]] = cmat
    return host


# ---- sf_sc2_seeds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 3, 255, 256, 257, 549])
def test_seeds_are_the_statements(eng, m):
    """One thread block, its edge with one less and one more, three blocks with a ragged one; vectors with many ties, all zero,
    and fewer positives than seeds; one seed, two, as many as matches, the cap."""
    rng = np.random.default_rng(200 + m)
    vectors = [rng.integers(0, 7, m), rng.integers(0, 2 ** 32, m, dtype=np.uint64), np.zeros(m), np.full(m, 2 ** 32 - 1),
               np.where(rng.random(m) < 0.02, rng.integers(1, 4, m), 0)]
    with _Held(eng) as dev:
        ds2 = dev.new((m,), np.uint32)
        for n_seeds in sorted({1, 2, m, R.MAX_SEEDS}):
            dseeds = dev.new((n_seeds,), np.int32)
            for v in vectors:
                s2 = np.asarray(v).astype(np.uint32)
                ds2.from_host(s2)
                dseeds.from_host(np.full(n_seeds, 7, dtype=np.int32))  # every slot must be written
                got = eng.sc2_seeds_device(ds2, m, n_seeds, dseeds).to_host()
                want = R.seeds_of(s2, n_seeds)
                assert got.dtype == np.int32 and np.array_equal(got, want), (m, n_seeds)
                found = got[got >= 0]
                assert np.all(s2[found] > 0) and found.size == min(n_seeds, int(np.count_nonzero(s2)))
    assert list(R.seeds_of(np.array([5, 9, 0, 9, 5, 1]), 4)) == [1, 3, 0, 4]  # the order itself: score down, position up


# ---- sf_sc2_seed_rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 33, 63, 64, 65, 255, 256, 257, 2 * T + 37])
def test_seed_rows_of_random_matrices(eng, m):
    """One MFMA block and its neighbours, the K-chunk, the column tile with one less and one more, three tiles with a ragged one;
    one seed tile, its edge, several; symmetric and not (which tells C C^T from C^T C and a transposed accumulator layout);
    seeds out of order, repeated, with -1 among them."""
    rng = np.random.default_rng(300 + m)
    pad = eng.sc2_padded(m)
    counts = sorted({min(n, R.MAX_SEEDS) for n in (1, 2, TS - 1, TS, TS + 1, 2 * TS + 5)})
    with _Held(eng) as dev:
        dmat = dev.new((pad, pad), np.uint8)
        drows = dev.new((max(counts), pad), np.uint32)
        dseeds = dev.new((max(counts),), np.int32)
        for density in (0.05, 0.5):
            for symmetric in (True, False):
                cmat = (rng.random((m, m)) < density).astype(np.uint8)
                if symmetric:
                    cmat = np.triu(cmat, 1) + np.triu(cmat, 1).T
                dmat.from_host(_padded(cmat, pad))
                for n_seeds in counts:
                    seeds = rng.integers(-1, m, n_seeds)
                    seeds[rng.integers(0, n_seeds)] = -1
                    if n_seeds > 2:
                        seeds[0] = seeds[n_seeds - 1] = m - 1  # a repeat, and the last row
                    dseeds.from_host(np.concatenate([seeds, np.zeros(max(counts) - n_seeds)]).astype(np.int32))
                    drows.from_host(np.full((max(counts), pad), 0xABCDEF, dtype=np.uint32))
                    got = eng.sc2_seed_rows_device(dmat, m, dseeds, n_seeds, drows).to_host()
                    want = R.seed_rows(cmat, seeds)
                    assert np.array_equal(got[:n_seeds, :m].astype(np.int64), want), (m, density, symmetric, n_seeds)
                    assert not got[:n_seeds, m:].any()                    # the padding columns
                    assert not got[:n_seeds][seeds < 0].any()             # a seed of -1: a zero row
                    assert (got[n_seeds:] == 0xABCDEF).all()              # nothing past the rows asked for
                    c64 = cmat.astype(np.int64)
                    brute = (c64[np.maximum(seeds, 0)] @ c64.T) * c64[np.maximum(seeds, 0)] * (seeds >= 0)[:, None]
                    assert np.array_equal(want, brute)                    # the statement's float32 product is exact


def test_seed_rows_of_k14s_matrix_sum_to_s2(eng):
    a, b, thr, edge = _set((2000, 0.05, 2))
    m, pad, n_seeds = a.shape[0], eng.sc2_padded(a.shape[0]), 2 * TS + 5
    with _Held(eng) as dev:
        da, db = dev.new((m, 3), values=a), dev.new((m, 3), values=b)
        dmat = dev.new((pad, pad), np.uint8)
        eng.consistency_matrix(da, db, m, thr, edge, out=dmat)
        s2 = eng.consistency_sc2(dmat, m)
        ds2 = dev.new((m,), np.uint32, s2)
        seeds = eng.sc2_seeds_device(ds2, m, n_seeds, dev.new((n_seeds,), np.int32))
        rows = eng.sc2_seed_rows_device(dmat, m, seeds, n_seeds, dev.new((n_seeds, pad), np.uint32)).to_host()
        seeds = seeds.to_host()
    assert (seeds >= 0).all() and np.array_equal(seeds, R.seeds_of(s2, n_seeds))
    assert np.array_equal(rows.sum(axis=1, dtype=np.int64), s2[seeds].astype(np.int64))
    assert not rows[np.arange(n_seeds), seeds].any()  # the diagonal of C is zero


# ---- sf_sc2_seed_fits -------------------------------------------------------------------------------------------------------------------
def _stages(eng, name):
    """The staged calls on a named set at FIT_SEEDS seeds, run once: matrix, s2, seeds, rows, fits (twice)."""
    if name in _staged:
        return _staged[name]
    a, b, thr, edge = _set(name)
    m, pad, n = a.shape[0], eng.sc2_padded(a.shape[0]), FIT_SEEDS
    with _Held(eng) as dev:
        da, db = dev.new((m, 3), values=a), dev.new((m, 3), values=b)
        dmat = dev.new((pad, pad), np.uint8)
        eng.consistency_matrix(da, db, m, thr, edge, out=dmat)
        s2 = eng.consistency_sc2(dmat, m)
        dseeds = eng.sc2_seeds_device(dev.new((m,), np.uint32, s2), m, n, dev.new((n,), np.int32))
        drows = eng.sc2_seed_rows_device(dmat, m, dseeds, n, dev.new((n, pad), np.uint32))
        runs = []
        for _ in range(2):
            out = [dev.new((n,), np.uint8, np.full(n, 9)), dev.new((n,), np.int32), dev.new((n, 12)), dev.new((n, 24)),
                   dev.new((n, m), np.uint8, np.full((n, m), 9))]
            eng.sc2_seed_fits_device(da, db, m, dseeds, drows, n, 0.5, *out)
            runs.append([x.to_host() for x in out])
        _staged[name] = dict(s2=s2, seeds=dseeds.to_host(), rows=drows.to_host(), fits=runs[0], again=runs[1])
    return _staged[name]


@pytest.mark.parametrize("name", FIT_SETS, ids=str)
def test_fits_equal_the_statement(eng, name):
    a, b, thr, edge = _set(name)
    m = a.shape[0]
    want, got = _hyp(name), _stages(eng, name)
    status, size, rt, sums, member = got["fits"]
    for x, y in zip(got["fits"], got["again"]):
        assert np.array_equal(x, y, equal_nan=True)  # two runs, bit for bit
    assert np.array_equal(got["s2"], want["second_degree"]) and np.array_equal(got["seeds"], want["seeds"])
    assert np.array_equal(got["rows"][:, :m].astype(np.int64), want["rows"]) and not got["rows"][:, m:].any()
    assert np.array_equal(member, want["member"]) and np.array_equal(size, want["size"]) and size.dtype == np.int32
    assert np.array_equal(status, want["status"]), (status, want["status"])
    assert not rt[status != 0].any() and np.isfinite(rt).all()
    worst_sum = worst_r = worst_t = 0.0
    for s in np.flatnonzero(want["seeds"] >= 0):
        ws, tol = want["sums"][s], float(size[s]) * EPS
        assert int(sums[s, 0]) == ws["count"] == size[s] and sums[s, 16] == 0.0 and sums[s, 23] == 0.0
        if not np.isfinite(ws["h"]).all():
            continue
        pairs = [(sums[s, 17:20], ws["sum_a"], ws["sum_a_abs"]), (sums[s, 20:23], ws["sum_b"], ws["sum_b_abs"]),
                 (sums[s, 1:4], ws["abar"], ws["sum_a_abs"] / size[s]), (sums[s, 4:7], ws["bbar"], ws["sum_b_abs"] / size[s]),
                 (sums[s, 7:16].reshape(3, 3), ws["h"], ws["h_abs"])]
        for mine, ref, scale in pairs:
            with np.errstate(divide="ignore", invalid="ignore"):
                worst_sum = max(worst_sum, float(np.nanmax(np.where(scale > 0, np.abs(mine - ref) / (tol * scale), 0.0))))
            assert np.all(np.abs(mine - ref) <= tol * scale), (name, s, mine, ref)
        if status[s] == 0:
            unit = EPS * want["cond"][s]
            r = rt[s, :9].reshape(3, 3)
            assert np.abs(r.T @ r - np.eye(3)).max() <= 8 * EPS and np.linalg.det(r) > 0.5
            worst_r = max(worst_r, float(np.abs(rt[s, :9] - want["rt"][s, :9]).max() / unit))
            worst_t = max(worst_t, float(np.abs(rt[s, 9:] - want["rt"][s, 9:]).max() / (unit * (1 + np.linalg.norm(ws["abar"])))))
    _worst[str(name)] = (worst_sum, worst_r, worst_t)
    print(f"{name}: {int((status == 0).sum())} fits of {int((want['seeds'] >= 0).sum())} seeds; worst sum = {worst_sum:.3f} x size 2^-52, "
          f"worst |R - R_numpy| = {worst_r:.2f}, worst |t - t_numpy| = {worst_t:.2f} x 2^-52 s1/gap (x (1 + |abar|) for t)")
    assert worst_r <= 64 and worst_t <= 64
    if name == "lattice":  # every point on one axis: no consensus set has a unique rotation
        assert (status[want["seeds"] >= 0] == 2).all()
    if name == "tie":  # 470 rows share the maximum: the seeds are the lowest 64 of them, each with the whole clique
        assert np.array_equal(want["seeds"], np.arange(130, 130 + FIT_SEEDS)) and (size == 470).all() and (status == 0).all()
    if name == "nan row":
        assert not member[:, 1234].any() and not member[:, 77].any() and 1234 not in want["seeds"]


def test_a_slot_without_a_seed_and_a_set_of_two(eng):
    """Status 3 and status 1 on hand-made rows: the fit call is defined for any seeds and rows."""
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 2, 0], [0.0, 0, 3], [5.0, 5, 5]])
    b = a + 1.0
    m, pad = 5, eng.sc2_padded(5)
    rows = np.zeros((3, pad), dtype=np.uint32)
    rows[0, :4] = [0, 2, 2, 2]   # seed 0 with 1, 2, 3: a fit
    rows[1, :4] = [4, 0, 1, 1]   # seed 1 with 0 only at share 0.5: two members
    with _Held(eng) as dev:
        da, db = dev.new((m, 3), values=a), dev.new((m, 3), values=b)
        out = [dev.new((3,), np.uint8), dev.new((3,), np.int32), dev.new((3, 12)), dev.new((3, 24)), dev.new((3, m), np.uint8)]
        eng.sc2_seed_fits_device(da, db, m, dev.new((3,), np.int32, [0, 1, -1]), dev.new((3, pad), np.uint32, rows), 3, 0.5, *out)
        status, size, rt, sums, member = (x.to_host() for x in out)
    assert list(status) == [0, 1, 3] and list(size) == [4, 2, 0]
    assert member.tolist() == [[1, 1, 1, 1, 0], [1, 1, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert np.abs(rt[0, :9].reshape(3, 3) - np.eye(3)).max() <= 8 * EPS and np.abs(rt[0, 9:] - 1.0).max() <= 8 * EPS
    assert not rt[1:].any() and not sums[2].any()


# ---- sf_sc2_registration ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [(2000, 0.05, 2), "lattice", "tie", "nan row", (5000, 0.004, 1)], ids=str)
def test_chain_compaction_counts_and_winner(eng, name):
    a, b, thr, edge = _set(name)
    m, n = a.shape[0], FIT_SEEDS
    staged = _stages(eng, name)
    status0, size0, rt0 = staged["fits"][:3]
    with _Held(eng) as dev:
        da, db = dev.new((m, 3), values=a), dev.new((m, 3), values=b)
        out = dict(s2=dev.new((m,), np.uint32), seeds=dev.new((n,), np.int32), status=dev.new((n,), np.uint8),
                   size=dev.new((n,), np.int32), rt=dev.new((n, 12)), slot_seed=dev.new((n,), np.int64), counts=dev.new((n,), np.int64))
        before = eng.lib.sf_sync_count()
        result, best = eng.sc2_registration_device(da, db, m, thr, edge, n, 0.5, **out)
        assert eng.lib.sf_sync_count() - before == 1  # ONE host wait
        host = {k: v.to_host() for k, v in out.items()}
        bare, bare_best = eng.sc2_registration_device(da, db, m, thr, edge, n, 0.5)  # no optional output: the same answer
    assert np.array_equal(result, bare) and np.array_equal(best, bare_best)
    # the optional outputs are the staged calls'
    assert np.array_equal(host["s2"], staged["s2"]) and np.array_equal(host["seeds"], staged["seeds"])
    assert np.array_equal(host["status"], status0) and np.array_equal(host["size"], size0)
    slot_seed = np.flatnonzero(status0 == 0)
    ns = slot_seed.size
    assert np.array_equal(host["slot_seed"][:ns], slot_seed) and (host["slot_seed"][ns:] == -1).all()  # seed order, nothing lost
    assert np.array_equal(host["rt"][:ns], rt0[slot_seed]) and not host["rt"][ns:].any()
    counts = host["counts"]
    assert np.array_equal(counts[:ns], N.score(a, b, host["rt"][:ns], thr)) and (counts[ns:] == -1).all()
    found = int((staged["seeds"] >= 0).sum())
    assert list(result[:4]) == [found, int((status0 == 1).sum()), int((status0 == 2).sum()), ns]
    if ns == 0:
        assert list(result[4:]) == [-1, 0, -1, 0] and not best.any()
        assert name == "lattice"
        return
    w = N.first_max(counts[:ns])
    rank = int(slot_seed[w])
    assert list(result[4:]) == [int(staged["seeds"][rank]), int(counts[w]), rank, int(size0[rank])]
    assert np.array_equal(best, host["rt"][w])


def test_chain_on_fewer_than_three_matches_and_no_triple(eng):
    a = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0]])
    b = a.copy()
    b[2:] += [0.0, 5.0, 0.0]  # two compatible pairs that no third match joins
    with _Held(eng) as dev:
        da, db = dev.new((4, 3), values=a), dev.new((4, 3), values=b)
        seeds = dev.new((8,), np.int32, np.full(8, 7))
        for m in (4, 2, 1):
            result, best = eng.sc2_registration_device(da, db, m, THR, THR, 8, 0.5, seeds=seeds)
            assert list(result) == [0, 0, 0, 0, -1, 0, -1, 0] and not best.any() and (seeds.to_host() == -1).all()
        seeds.from_host(np.full(8, 7, dtype=np.int32))
        result, best = eng.sc2_registration_device(da, db, 0, THR, THR, 8, 0.5, seeds=seeds)  # m = 0: nothing is written
        assert list(result) == [0, 0, 0, 0, -1, 0, -1, 0] and (seeds.to_host() == 7).all()


# ---- the public call --------------------------------------------------------------------------------------------------------------------
def test_public_call_recovers_the_set_the_single_seed_loses(eng):
    """(5000, 0.004, 1): 15 true matches in 5000.  The filter's seed is a false match and it keeps no true one; the best of 64
    seeds by inliers is the true clique -- the case the estimator exists for."""
    m, share, seed = 5000, 0.004, 1
    sk, rk, si, ri, r0, t0 = N.synthetic_matches(m, share, seed=seed)
    true = C.synthetic_truth(m, share, seed)[0]
    a, b = N.matched_points(si, ri, sk, rk)
    kept_s, _, frec = second_order_consistency_filter(si, ri, sk, rk, distance_threshold=THR, engine=eng)
    assert frec.seed not in true and np.intersect1d(frec.keep, true).size == 0 and frec.keep.size > 0
    want_ratio, want_r, want_t, want = R.sc2_registration(si, ri, sk, rk, THR, n_seeds=64)
    ratio, tf, rec = sc2_registration(si, ri, sk, rk, distance_threshold=THR, n_seeds=64, engine=eng)
    assert ratio == want_ratio == true.size / m
    inliers = np.flatnonzero(N.inlier_mask(a, b, np.concatenate([tf.rotation.reshape(9), tf.translation]), THR))
    want_inliers = np.flatnonzero(N.inlier_mask(a, b, np.concatenate([want_r.reshape(9), want_t]), THR))
    assert np.array_equal(inliers, want_inliers) and np.array_equal(inliers, true)
    assert (rec.status, rec.winner_seed, rec.winner_rank, rec.winner_size, rec.winner_inliers, rec.refit_inliers) == (
        "done", want["winner_seed"], want["winner_rank"], want["winner_size"], want["winner_inliers"], want["refit_inliers"])
    assert rec.winner_rank > 0 and rec.winner_seed in true  # not the first maximum of s2
    assert np.array_equal(rec.seeds, want["seeds"]) and np.array_equal(rec.seed_status, want["seed_status"])
    assert np.array_equal(rec.seed_size, want["size"]) and np.array_equal(rec.second_degree, want["second_degree"])
    assert np.array_equal(rec.seed_inliers[want["slot_seed"]], want["counts"]) and (np.delete(rec.seed_inliers, want["slot_seed"]) == -1).all()
    print(f"{(m, share, seed)}: seed rank {rec.winner_rank}, consensus {rec.winner_size}, inliers {rec.winner_inliers} -> "
          f"{rec.refit_inliers}, |R - R0| = {np.linalg.norm(tf.rotation - r0):.2e}")
    assert np.linalg.norm(tf.rotation - r0) <= 2e-3 and np.linalg.norm(tf.translation - t0) <= 2e-3


def test_public_call_one_seed_and_many_agree_where_the_seed_is_true(eng):
    sk, rk, si, ri = N.synthetic_matches(2000, 0.05, seed=2)[:4]
    a, b = N.matched_points(si, ri, sk, rk)
    sets = []
    for n_seeds in (1, 256):
        ratio, tf, rec = sc2_registration(si, ri, sk, rk, distance_threshold=THR, n_seeds=n_seeds, engine=eng)
        sets.append(np.flatnonzero(N.inlier_mask(a, b, np.concatenate([tf.rotation.reshape(9), tf.translation]), THR)))
        assert ratio == sets[-1].size / 2000 and 1 <= rec.seeds.size <= n_seeds
    assert np.array_equal(sets[0], sets[1]) and np.array_equal(sets[0], C.synthetic_truth(2000, 0.05, 2)[0])


def test_errors_are_raised_before_any_allocation(eng):
    a, b = (x[:300] for x in _set((2000, 0.05, 2))[:2])
    nan, inf = float("nan"), float("inf")
    with _Held(eng) as dev:
        da, db = dev.new((300, 3), values=a), dev.new((300, 3), values=b)
        result, best = np.zeros(8, dtype=np.int64), np.zeros(12)
        rp, bp = result.ctypes.data, best.ctypes.data
        opt = [None] * 7

        def chain(m=300, thr=THR, edge=THR, n_seeds=8, share=0.5, pa=da.ptr, pb=db.ptr, r=rp, bst=bp):
            return eng.lib.sf_sc2_registration(eng.h, pa, pb, m, thr, edge, n_seeds, share, *opt, r, bst)

        assert chain() == 0
        for kw in (dict(m=-1), dict(m=32769), dict(m=2 ** 31), dict(thr=-1e-3), dict(thr=nan), dict(thr=inf), dict(edge=-1e-3),
                   dict(edge=nan), dict(n_seeds=0), dict(n_seeds=R.MAX_SEEDS + 1), dict(n_seeds=-3), dict(share=0.0), dict(share=1.5),
                   dict(share=nan), dict(pa=None), dict(pb=None), dict(r=None), dict(bst=None)):
            assert chain(**kw) == -1, kw
            assert "sf_sc2_registration" in _ffi.last_error()
        ds2, dseeds = dev.new((300,), np.uint32), dev.new((8,), np.int32)
        pad = eng.sc2_padded(300)
        dmat, drows = dev.new((pad, pad), np.uint8), dev.new((8, pad), np.uint32)
        st, sz, rt = dev.new((8,), np.uint8), dev.new((8,), np.int32), dev.new((8, 12))
        for m, n_seeds in ((-1, 8), (32769, 8), (300, 0), (300, R.MAX_SEEDS + 1)):
            assert eng.lib.sf_sc2_seeds(eng.h, ds2.ptr, m, n_seeds, dseeds.ptr) == -1 and "sf_sc2_seeds" in _ffi.last_error()
            assert eng.lib.sf_sc2_seed_rows(eng.h, dmat.ptr, m, dseeds.ptr, n_seeds, drows.ptr) == -1 and "sf_sc2_seed_rows" in _ffi.last_error()
            assert eng.lib.sf_sc2_seed_fits(eng.h, da.ptr, db.ptr, m, dseeds.ptr, drows.ptr, n_seeds, 0.5, st.ptr, sz.ptr, rt.ptr, None,
                                            None) == -1 and "sf_sc2_seed_fits" in _ffi.last_error()
        for share in (0.0, 1.0001, nan):
            with pytest.raises(ShotFpfhError, match="group_share"):
                eng.sc2_seed_fits_device(da, db, 300, dseeds, drows, 8, share, st, sz, rt)
        for args in ((None, 300, 8, dseeds.ptr), (ds2.ptr, 300, 8, None)):
            assert eng.lib.sf_sc2_seeds(eng.h, *args) == -1
        for hole in (0, 2, 4):
            args = [dmat.ptr, 300, dseeds.ptr, 8, drows.ptr]
            args[hole] = None
            assert eng.lib.sf_sc2_seed_rows(eng.h, *args) == -1
        # the engine checks the buffers it is handed
        with pytest.raises(ValueError):
            eng.sc2_seeds_device(ds2, 300, 9, dseeds)
        with pytest.raises(ValueError):
            eng.sc2_seed_rows_device(dmat, 300, dseeds, 9, drows)
        with pytest.raises(ValueError):
            eng.sc2_seed_rows_device(dmat, 300 + T, dseeds, 8, drows)
        with pytest.raises(ValueError):
            eng.sc2_seed_fits_device(da, db, 300, dseeds, drows, 8, 0.5, sz, sz, rt)
        with pytest.raises(ValueError):
            eng.sc2_registration_device(da, db, 300, THR, THR, 8, 0.5, counts=dseeds)
    idx = np.zeros(S.MAX_MATCHES + 1, dtype=np.int64)  # index vectors only: refused before any upload
    with pytest.raises(ValueError, match="ratio_test_matching"):
        sc2_registration(idx, idx, a, b, distance_threshold=THR, engine=eng)
    for n_seeds in (0, R.MAX_SEEDS + 1):
        with pytest.raises(ValueError, match="n_seeds"):
            sc2_registration(idx[:300], idx[:300], a, b, distance_threshold=THR, n_seeds=n_seeds, engine=eng)
    with pytest.raises(ValueError, match="nothing to fit"):  # all matches the same pair: no triple
        sc2_registration(idx[:300], idx[:300], a, b, distance_threshold=THR, engine=eng)
