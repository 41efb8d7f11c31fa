"""K8 top-2 (sf_match_top2, csrc/match_top2.hip) and the ratio test on the MI355X.

The yardstick is a NumPy restatement of the contract, kept here: dist(i, j) is the float64 sum of (a[i,t] - b[j,t])^2 taken
left to right over t (NumPy's elementwise operations do not fuse), then sqrt; reference rows rank by (dist, column).  Every
comparison is bit for bit."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import shot_fpfh_amd as s

    return s.default_engine()


def top2_reference(a, b, rows=128):
    """(idx (m1, 2), dist (m1, 2)): the first two reference rows by (dist, column); j2 = -1, d2 = +inf when b has one row."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    m1, m2 = a.shape[0], b.shape[0]
    bt = np.ascontiguousarray(b.T)
    idx, dist = np.full((m1, 2), -1, dtype=np.int64), np.full((m1, 2), np.inf)
    for r0 in range(0, m1, rows):
        ac = a[r0:r0 + rows]
        acc, tmp = np.zeros((ac.shape[0], m2)), np.empty((ac.shape[0], m2))
        for t in range(a.shape[1]):
            np.subtract(ac[:, t:t + 1], bt[t], out=tmp)
            np.multiply(tmp, tmp, out=tmp)
            acc += tmp
        dm = np.sqrt(acc)
        r = np.arange(ac.shape[0])
        j1 = np.argmin(dm, axis=1)  # first minimum: the smaller column on ties
        idx[r0:r0 + rows, 0], dist[r0:r0 + rows, 0] = j1, dm[r, j1]
        if m2 > 1:
            dm[r, j1] = np.inf
            j2 = np.argmin(dm, axis=1)
            idx[r0:r0 + rows, 1], dist[r0:r0 + rows, 1] = j2, dm[r, j2]
    return idx, dist


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.int64), exp[1].view(np.int64))


def shot_like(rng, m, d=352, density=0.3):
    """Sparse non-negative unit rows, as SHOT's."""
    x = rng.random((m, d)) * (rng.random((m, d)) < density)
    x[:, 0] += 1e-3
    return x / np.linalg.norm(x, axis=1)[:, None]


def test_exact_path_match_300(eng):
    g = load_golden("match_300.npz")
    idx, dist, n_exact = eng.match_top2(g["scan"], g["ref"])
    assert same((idx, dist), top2_reference(g["scan"], g["ref"])) and n_exact == 300
    assert np.array_equal(idx[:, 0], eng.match_argmin(g["scan"], g["ref"])[0])


@pytest.mark.parametrize("d", [1, 3, 37, 125, 352])
def test_exact_path_random(eng, d):
    rng = np.random.default_rng(d)
    a, b = rng.standard_normal((333, d)), rng.standard_normal((517, d))
    idx, dist, n_exact = eng.match_top2(a, b)
    assert same((idx, dist), top2_reference(a, b)) and n_exact == 333
    ai, bi = rng.integers(-3, 4, (300, d)).astype(np.float64), rng.integers(-3, 4, (200, d)).astype(np.float64)  # many ties
    assert same(eng.match_top2(ai, bi)[:2], top2_reference(ai, bi))


def tie_sets(rng, m1, m2, d):
    """Reference rows duplicated twice and three times, scan rows equal to a reference row, and scan rows equidistant from
    several reference rows (centre +- unit steps: every distance exactly 1)."""
    b = rng.standard_normal((m2, d))
    b[10], b[11] = b[3], b[3]
    b[m2 - 1] = b[20]
    b[40], b[90], b[m2 - 2] = b[7], b[7], b[7]
    a = rng.standard_normal((m1, d))
    a[0], a[1], a[2], a[3] = b[3], b[7], b[20], b[m2 // 2]
    c = np.round(rng.standard_normal(d) * 4) + 100.0
    for q, j in enumerate(range(100, 106)):
        b[j] = c
        b[j, q] += 1.0 if q % 2 else -1.0
    a[4] = c
    a[5:9] = b[3] + 1e-3 * rng.standard_normal((4, d))
    return a, b


def test_ties_exact_path(eng):
    rng = np.random.default_rng(11)
    a, b = tie_sets(rng, 120, 300, 24)
    idx, dist, _ = eng.match_top2(a, b)
    assert same((idx, dist), top2_reference(a, b))
    assert list(idx[0]) == [3, 10] and dist[0, 0] == 0.0 and dist[0, 1] == 0.0
    assert list(idx[1]) == [7, 40] and list(idx[2]) == [20, 299] and list(idx[4]) == [100, 101] and dist[4, 0] == dist[4, 1] == 1.0


def test_ties_matrix_core_path(eng):
    rng = np.random.default_rng(12)
    a, b = tie_sets(rng, 1024, 2048, 352)
    idx, dist, n_exact = eng.match_top2(a, b)
    assert same((idx, dist), top2_reference(a, b))
    assert list(idx[0]) == [3, 10] and list(idx[1]) == [7, 40] and list(idx[2]) == [20, 2047] and list(idx[4]) == [100, 101]
    assert 0 < n_exact < 1024  # the triplicated row (and the equidistant centre) are rescued, the rest decided by the GEMM


@pytest.mark.parametrize("kind", ["random", "shot"])
def test_matrix_core_path(eng, kind):
    rng = np.random.default_rng(21 if kind == "random" else 22)
    if kind == "random":
        a, b = rng.standard_normal((1024, 352)), rng.standard_normal((2048, 352))
    else:
        a, b = shot_like(rng, 1024), shot_like(rng, 2048)
    idx, dist, n_exact = eng.match_top2(a, b)
    assert same((idx, dist), top2_reference(a, b))
    assert n_exact < 1024 // 4  # the FP64 path decided most rows


def test_near_ties_between_ranks_two_and_three_are_rescued(eng):
    rng = np.random.default_rng(31)
    a, b = shot_like(rng, 1024), shot_like(rng, 2048)
    for q in range(64):  # scan row q: nearest at 0.5 delta, then two rows at delta along different axes
        delta = 1e-3
        b[3 * q] = a[q] + 0.5 * delta * np.eye(352)[q % 352]
        b[3 * q + 1] = a[q] + delta * np.eye(352)[(q + 1) % 352]
        b[3 * q + 2] = a[q] + delta * np.eye(352)[(q + 2) % 352] * (1.0 + 1e-15 * (q % 3))
    idx, dist, n_exact = eng.match_top2(a, b)
    assert same((idx, dist), top2_reference(a, b))
    assert n_exact >= 32


def test_column_zero_is_the_arg_min_on_the_fp16_path(eng):
    """4096 x 16384 x 352 is above the FP16 pre-filter's size rule of sf_match_argmin (work >= 2e10, m1 >= 2048)."""
    rng = np.random.default_rng(41)
    a, b = shot_like(rng, 4096), shot_like(rng, 16384)
    a[:8] = b[100:108]
    idx, dist, _ = eng.match_top2(a, b)
    ai, ad, _ = eng.match_argmin(a, b)
    assert np.array_equal(idx[:, 0], ai) and np.array_equal(dist[:, 0].view(np.int64), ad.view(np.int64))
    rows = np.r_[0:8, rng.choice(4096, 56, replace=False)]
    exp = top2_reference(a[rows], b)
    assert same((idx[rows], dist[rows]), exp)


def test_edge_cases(eng):
    from shot_fpfh_amd import ShotFpfhError

    rng = np.random.default_rng(51)
    a = rng.standard_normal((7, 5))
    idx, dist, _ = eng.match_top2(a, a[2:3])
    assert np.array_equal(idx, np.c_[np.full(7, 0), np.full(7, -1)]) and np.isinf(dist[:, 1]).all()
    assert same((idx, dist), top2_reference(a, a[2:3]))
    assert same(eng.match_top2(a, a[1:3])[:2], top2_reference(a, a[1:3]))
    idx, dist, n = eng.match_top2(np.zeros((0, 5)), a)
    assert idx.shape == (0, 2) and dist.shape == (0, 2) and n == 0
    with pytest.raises(ValueError):
        eng.match_top2(a, np.zeros((0, 5)))
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy()
        x[3, 1] = bad
        with pytest.raises(ValueError):
            eng.match_top2(x, a)
        with pytest.raises(ValueError):
            eng.match_top2(a, x)
        dx, da = eng.empty(x.shape).from_host(x), eng.empty(a.shape).from_host(a)
        with pytest.raises(ShotFpfhError):
            eng.match_top2_device(dx, da, eng.empty((7, 2), np.int64))


def test_device_form_equals_host_form_and_repeats(eng):
    rng = np.random.default_rng(61)
    a, b = shot_like(rng, 1500), shot_like(rng, 2100)
    b[5], b[6], b[7] = b[1], b[1], b[1]
    a[0] = b[1]
    host = eng.match_top2(a, b)
    da, db = eng.empty(a.shape).from_host(a), eng.empty(b.shape).from_host(b)
    runs = []
    for _ in range(2):
        idx, dist = eng.empty((1500, 2), np.int64), eng.empty((1500, 2))
        n = eng.match_top2_device(da, db, idx, dist)
        runs.append((idx.to_host(), dist.to_host(), n))
    for got in runs:
        assert same(got[:2], host[:2]) and got[2] == host[2] and got[2] > 0
    small = eng.empty((1500, 2), np.int64)
    eng.match_top2_device(da, eng.empty((10, 352)).from_host(b[:10]), small)  # exact path, no distances
    assert np.array_equal(small.to_host(), top2_reference(a, b[:10])[0])


def duplicated_ref_300():
    g = load_golden("match_300.npz")
    ref = np.vstack([g["ref"], g["ref"][[4, 50, 51, 200]]])
    return g["scan"], ref


@pytest.mark.parametrize("ratio", [0.5, 0.8, 0.95, 1.0])
def test_ratio_test_on_match_300(eng, ratio):
    from shot_fpfh_amd.matching import ratio_test_matching

    for scan, ref in (tuple(load_golden("match_300.npz")[k] for k in ("scan", "ref")), duplicated_ref_300()):
        s, r = ratio_test_matching(scan, ref, ratio, verbose=False, engine=eng)
        sr, rr = np.flatnonzero(scan.any(axis=1)), np.flatnonzero(ref.any(axis=1))
        idx, dist = top2_reference(scan[sr], ref[rr])
        keep = dist[:, 0] < np.float64(ratio) * dist[:, 1]
        assert np.array_equal(s, sr[keep]) and np.array_equal(r, rr[idx[keep, 0]])


def test_ratio_one_drops_exactly_the_ties(eng):
    from shot_fpfh_amd.matching import match_two_nearest, ratio_test_matching

    scan, ref = duplicated_ref_300()
    rows, ridx, dist = match_two_nearest(scan, ref, engine=eng)
    tied = dist[:, 0] == dist[:, 1]
    assert tied.sum() > 0
    s, _ = ratio_test_matching(scan, ref, 1.0, verbose=False, engine=eng)
    assert np.array_equal(s, rows[~tied])
    for bad in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ratio_test_matching(scan, ref, bad, verbose=False, engine=eng)


def test_pipeline_ratio_matching_end_to_end(eng):
    from conftest import config1_cloud
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    p, n = config1_cloud(6000, 5)
    rot = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    pipe = RegistrationPipeline(scan=p @ rot.T, scan_normals=n @ rot.T, ref=p, ref_normals=n)
    pipe.select_keypoints("subsampling", neighborhood_size=0.08)
    pipe.compute_descriptors(0.2, descriptor_choice="shot_single_scale", disable_progress_bars=True, verbose=False)
    pipe.find_descriptors_matches("ratio", reject_threshold=0.9, threshold_multiplier=10)
    sd, rd = pipe.scan_descriptors, pipe.ref_descriptors
    sr, rr = np.flatnonzero(sd.any(axis=1)), np.flatnonzero(rd.any(axis=1))
    idx, dist = top2_reference(sd[sr], rd[rr])
    keep = dist[:, 0] < 0.9 * dist[:, 1]
    assert np.array_equal(pipe.matches[0], sr[keep]) and np.array_equal(pipe.matches[1], rr[idx[keep, 0]])
    assert 0 < pipe.matches[0].shape[0] <= sr.shape[0]
