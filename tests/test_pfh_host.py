"""Point Feature Histograms (K22) without a GPU: the library's tables, the NumPy statement (tests/pfh_numpy.py) against the
direct PCL formulas and against closed forms, its invariance under the order of a list and of the cloud, every branch of the
source rule, pairs exactly on bin edges, and the argument errors of compute_pfh_descriptor that need no device."""

import numpy as np
import pytest

import pfh_numpy as P

ALL_S = [1, 2, 3, 4, 5, 6, 7, 8, 11, 16]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def neighbourhood(rng, n, parallel):
    """n points in a ball with random unit normals; parallel: the normals within 1e-3 of one direction."""
    p = rng.standard_normal((n, 3)) * 0.05
    nr = _unit(rng.standard_normal((n, 3)))
    if parallel:
        nr = _unit(nr[:1] + 1e-3 * rng.standard_normal((n, 3)))
    return p, nr


# ---- the tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ALL_S)
def test_tables_against_numpy(S):
    q, ca, sa, g = P.tables(S)
    qn, can, san, gn = P.tables_numpy(S)
    assert np.array_equal(bits(q), bits(qn)) and np.array_equal(g, gn)
    it = slice(1, S)  # (the interior edges: the only ones used)
    ulp = np.spacing(1.0)
    assert (np.abs(ca[it] - can[it]) <= 2 * ulp).all() and (np.abs(sa[it] - san[it]) <= 2 * ulp).all()
    assert q[0] == -1.0 and q[S] == 1.0 and (np.diff(q) > 0).all()
    if S % 2 == 0:
        assert q[S // 2] == 0.0 and g[S // 2] == 0 and ca[S // 2] == 1.0 and sa[S // 2] == 0.0
        assert not np.signbit(q[S // 2]) and not np.signbit(sa[S // 2])
    assert (g[: (S + 1) // 2] == -1).all() and (g[S // 2 + 1:] == 1).all()
    assert (sa[it][g[it] < 0] < 0).all() and (sa[it][g[it] > 0] > 0).all()


def test_tables_refuse_bad_bin_counts():
    from shot_fpfh_amd import _ffi

    lib = _ffi.load()
    buf = np.zeros(64)
    sign = np.zeros(64, dtype=np.int32)
    for S in (0, 17, -3):
        assert lib.sf_pfh_tables(S, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, sign.ctypes.data) == -1
        assert "sf_pfh_tables" in _ffi.last_error()
    assert lib.sf_pfh_tables(5, None, buf.ctypes.data, buf.ctypes.data, sign.ctypes.data) == -1
    assert _ffi.PFH_MAX_BINS == P.MAX_BINS == 16


# ---- the statement against the direct formulas ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ALL_S)
def test_rules_equal_the_direct_formulas_off_the_edges(S):
    rng = np.random.default_rng(0)
    tab = P.tables(S)
    total = left_out = wrong = 0
    branches = np.zeros(3, dtype=np.int64)
    for i in range(40):
        p, nr = neighbourhood(rng, int(rng.integers(2, 61)), i % 4 == 3)
        f = P.list_pairs(p, nr, np.arange(p.shape[0]))
        keep = f["keep"]
        assert keep.all()
        b1, b2, b3 = P.rule_bins(f, tab, S)
        w1, w2, w3, margin = P.formula_bins(f, S)
        clear = margin > 1e-9
        total += keep.size
        left_out += int((~clear).sum())
        wrong += int((((b1 != w1) | (b2 != w2) | (b3 != w3)) & clear).sum())
        branches += np.bincount(f["branch"], minlength=3)
        assert b1.max() < S and b2.max() < S and b3.max() < S and min(b1.min(), b2.min(), b3.min()) >= 0
    print(f"S = {S}: {total} pairs, {left_out} within 1e-9 bin widths of an edge, {wrong} disagreements")
    assert wrong == 0
    assert left_out * 10 ** 4 <= total
    assert branches[0] == total  # (random normals: the magnitudes decide every source)


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def test_two_points_land_in_the_predicted_bin():
    """s = 0, t = (1, 0, 0), n_s = (0, 0, 1), n_t = (0, 0.28, 0.96): a_s = +0 and a_t = -0 tie, s comes first; phi = 0,
    v = (0, -1, 0), alpha = -0.28, w = (1, 0, 0), a = 0, B = 0.96: theta = 0.  S = 5: bins (2, 1, 2)."""
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    nr = np.array([[0.0, 0.0, 1.0], [0.0, 0.28, 0.96]])
    f = P.list_pairs(pts, nr, [0, 1])
    assert f["branch"][0] == 2 and not f["tsrc"][0] and f["num2"][0] == -0.28 and f["a"][0] == 0 and f["B"][0] == 0.96
    want = np.zeros(125)
    want[2 + 5 * 1 + 25 * 2] = 100.0
    for order in ([0, 1], [1, 0]):
        assert np.array_equal(bits(P.rows(pts, nr, [order], 5)[0]), bits(want))
    assert np.array_equal(P.rows(pts, nr, [[0, 1]], 1), [[100.0]])


def test_short_lists_duplicates_and_the_row_sum():
    rng = np.random.default_rng(2)
    p, nr = neighbourhood(rng, 30, False)
    assert not P.rows(p, nr, [[], [7]], 5).any()
    nb = np.r_[np.arange(30), [3, 3, 11]]  # entry 3 three times, 11 twice: 3 + 1 pairs at distance zero
    cnt, skipped = P.counts(p, nr, nb, 5)
    assert skipped == 4
    pairs = 33 * 32 // 2
    assert cnt.sum() == pairs - 4
    row = P.rows(p, nr, [nb], 5)[0]
    assert np.array_equal(bits(row), bits(100.0 * cnt / pairs))
    assert abs(row.sum() - 100.0 * (pairs - 4) / pairs) < 1e-11
    with pytest.raises(ValueError):
        P.rows(p, nr, [np.zeros(P.MAX_LIST, dtype=np.int64)], 2)


@pytest.mark.parametrize("S", [2, 5, 8])
def test_a_permuted_list_and_a_permuted_cloud_give_identical_rows(S):
    rng = np.random.default_rng(3)
    p, nr = neighbourhood(rng, 50, False)
    nr[10:20] = nr[10]  # ties of the magnitudes among equal normals on a plane are still possible: keep some structure
    lists = [np.arange(50), np.arange(0, 50, 3), np.arange(5, 40)]
    first = P.rows(p, nr, lists, S)
    assert first.any(axis=1).all()
    shuffled = [rng.permutation(a) for a in lists]
    assert np.array_equal(bits(P.rows(p, nr, shuffled, S)), bits(first))
    order = rng.permutation(50)
    inv = np.argsort(order)
    assert np.array_equal(bits(P.rows(p[order], nr[order], [inv[a] for a in lists], S)), bits(first))


@pytest.mark.parametrize("normal", [(0.0, 0.0, 1.0), (1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0)])
def test_the_lattice_with_a_common_normal_meets_the_tie_branches(normal):
    g = np.arange(4) / 16.0
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    nr = np.tile(np.array(normal), (64, 1))
    f = P.list_pairs(p, nr, np.arange(64))
    assert f["keep"].size == 2016
    by_branch = np.bincount(f["branch"], minlength=3)
    print("pairs decided by |.|, by the signed value, by the coordinates:", by_branch, "skipped:", int((~f["keep"]).sum()))
    assert by_branch[1] > 0 and by_branch[2] > 0  # larger signed value; equal values: the coordinates
    if normal[2] == 1.0:
        assert by_branch[0] == 0 and int((~f["keep"]).sum()) == 96  # every pair ties; the 96 pairs along the normal are skipped
    rng = np.random.default_rng(4)
    mixed = P.list_pairs(p, nr, rng.permutation(64))  # (in the lattice's own order s always comes first)
    assert mixed["tsrc"][mixed["branch"] == 2].any() and (~mixed["tsrc"][mixed["branch"] == 2]).any()
    for S in (4, 5):
        first = P.rows(p, nr, [np.arange(64)], S)
        assert np.array_equal(bits(P.rows(p, nr, [rng.permutation(64)], S)), bits(first))
        order = rng.permutation(64)
        assert np.array_equal(bits(P.rows(p[order], nr[order], [np.arange(64)], S)), bits(first))


# ---- pairs exactly on edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3, 4, 5, 8, 11, 16])
def test_pairs_exactly_on_edges(S):
    pts, nr, lists, want = P.near_edge_fixture(S)
    tab = P.tables(S)
    rows = P.rows(pts, nr, lists, S, tab)
    assert np.array_equal(np.count_nonzero(rows, axis=1), np.ones(len(lists))) and (rows.max(axis=1) == 100.0).all()
    got = np.argmax(rows, axis=1)
    checked = 0
    for i, w in enumerate(want):
        f = P.list_pairs(pts, nr, lists[i])
        assert f["keep"][0] and not f["tsrc"][0] and f["d2"][0] == 1.0 and f["v2"][0] == 1.0
        b = (got[i] % S, got[i] // S % S, got[i] // (S * S))
        for have, expect in zip(b, w):
            if expect is not None:
                checked += 1
                assert have == expect, (S, i, b, w)
    assert checked >= 9
    # the special angles really are what the fixture says
    for i, (a_sign, b_sign) in enumerate([(0, 1), (0, -1), (0, 1), (1, 0), (-1, 0)]):
        fi = P.list_pairs(pts, nr, lists[i])
        assert np.sign(fi["a"][0]) == a_sign and np.sign(fi["B"][0]) == b_sign
    assert P.list_pairs(pts, nr, lists[5])["branch"][0] == 2 and P.list_pairs(pts, nr, lists[5])["num3"][0] == 0.0


# ---- the public function's argument errors -------------------------------------------------------------------------------------
def test_compute_pfh_descriptor_argument_errors_need_no_device():
    from shot_fpfh_amd.descriptors import compute_pfh_descriptor

    pts = np.random.default_rng(5).random((20, 3))
    nr = _unit(np.random.default_rng(6).standard_normal((20, 3)))
    kp = np.arange(5)
    for S in (0, 17, -1):
        with pytest.raises(ValueError):
            compute_pfh_descriptor(kp, pts, nr, 0.1, S)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            compute_pfh_descriptor(kp, pts, nr, radius)
    with pytest.raises(ValueError):
        compute_pfh_descriptor(kp, pts, nr[:-1], 0.1)
    with pytest.raises(ValueError):
        compute_pfh_descriptor(kp, pts[:, :2], nr[:, :2], 0.1)
    with pytest.raises(ValueError):
        compute_pfh_descriptor(np.array([0, 20]), pts, nr, 0.1)
    with pytest.raises(ValueError):
        compute_pfh_descriptor(np.ones(19, dtype=bool), pts, nr, 0.1)
    # nothing to compute: zeros of the right shape, still without a device
    assert compute_pfh_descriptor(np.zeros(0, dtype=np.int64), pts, nr, 0.1).shape == (0, 125)
    assert compute_pfh_descriptor(np.zeros(20, dtype=bool), pts, nr, 0.1, 3).shape == (0, 27)
    assert compute_pfh_descriptor(np.zeros(0, dtype=np.int64), np.zeros((0, 3)), np.zeros((0, 3)), 0.1, n_bins=2).shape == (0, 8)


# ---- the kernels' registers ---------------------------------------------------------------------------------------------------
def test_pfh_kernels_do_not_spill():
    """From the compiler's resource remarks of csrc/pfh.hip (written by every build): both instantiations of k_pfh keep every
    register -- a spill would sit inside the pair loop -- and use no scratch."""
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "shot_fpfh_amd", "csrc", "build", "pfh.remarks")
    if not os.path.exists(path):
        pytest.skip("no build/pfh.remarks (the library was not built by its Makefile here)")
    res, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in res.items() if "k_pfh" in k}
    assert len(kernels) == 2, list(res)
    for name, r in kernels.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)  # eight waves per SIMD by registers
