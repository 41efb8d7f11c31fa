"""Unique Shape Context (K21) without a GPU: the library's host-side tables, the NumPy statement (tests/usc_numpy.py) against
closed forms, and the exact sums of csrc/usc_acc.h built for the host (tests/usc_acc_host_shim.hip) against fractions.Fraction."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import usc_numpy as U
from conftest import ROOT

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
SHAPES = [(14, 14, 10), (12, 11, 15), (2, 1, 1), (4, 2, 1), (16, 16, 16)]


def ulps(a, b):
    """|a - b| in units of the spacing of b (0 where both are 0)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(b), np.finfo(np.float64).tiny))


# ---- the tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("radius, min_radius", [(0.03, 0.003), (1.0, 0.25), (37.5, 0.01)])
def test_library_tables_match_numpy_formulas(shape, radius, min_radius):
    """Every table within 2 ulp of its NumPy formula.  e2, ca, sa and q: the whole chain from the parameters.  vol: its formula
    on the library's OWN edges, which the tables give back exactly (sqrt(x x) = |x| in binary floating point) -- the shell volume
    e[j + 1]^3 - e[j]^3 cancels, so an ulp of e that two correct exp()s disagree by is several ulp of vol (usc_numpy.vol_numpy:
    NumPy's exp is 0.51 - 0.57 ulp off at four of these edges where the library's is the correctly rounded value, e2 then
    differs by 2 ulp and a vol taken through NumPy's own e by 5, at (16, 16, 16); that figure is printed, the formula is
    checked where it is well conditioned)."""
    L, K, J = shape
    lib_tab, np_tab = U.tables(radius, min_radius, L, K, J), U.tables_numpy(radius, min_radius, L, K, J)
    e2, ca, sa, q, vol = lib_tab
    e, ct = np.sqrt(e2), np.copysign(np.sqrt(np.abs(q)), q)
    assert np.array_equal(e * e, e2) and np.array_equal(ct * np.abs(ct), q)  # (the library's edges, exactly)
    print(f"vol through NumPy's own edges: {ulps(vol, np_tab[4]).max():.2f} ulp")
    for name, a, b in zip(("e2", "ca", "sa", "q", "vol"), lib_tab, np_tab[:4] + (U.vol_numpy(e, ct, L),)):
        assert a.shape == b.shape, name
        worst = ulps(a, b).max()
        print(f"{name}: {worst:.2f} ulp")
        # cos(pi / 2) and its like: a value that cancelled to ~1e-17 has no meaningful ulp; those are held to 2 ulp of 1
        small = np.abs(b) < 1e-15
        assert (ulps(a, b)[~small] <= 2).all(), (name, worst)
        assert (np.abs(a - b)[small] <= 2 * np.finfo(np.float64).eps).all(), name
    assert e2[0] == min_radius * min_radius and e2[J] == radius * radius  # e[0] = r0, e[J] = R
    assert q[0] == 1.0 and q[K] == -1.0  # ct[0] = 1, ct[K] = -1
    if K % 2 == 0:
        assert q[K // 2] == 0.0 and not np.signbit(q[K // 2])  # ct[K / 2] = 0
    assert ca[0] == 1.0 and sa[0] == 0.0
    assert (np.diff(e2) > 0).all() and (np.diff(q) < 0).all() and (vol > 0).all() and np.isfinite(vol).all()
    assert vol.shape == (L * K * J,)
    assert np.array_equal(vol.reshape(L, K, J), np.broadcast_to(vol.reshape(L, K, J)[0], (L, K, J)))  # no azimuth dependence


def test_argument_refusals():
    """Odd L, D > 4096, r0 >= R (and their neighbours): by the statement, by sf_usc_tables, and by compute_usc_descriptor before
    it touches the GPU (ValueError, where creating an engine without a GPU would raise ShotFpfhError)."""
    from shot_fpfh_amd import _ffi
    from shot_fpfh_amd.descriptors import compute_usc_descriptor

    lib = _ffi.load()
    buf = np.zeros(8192)
    p = buf.ctypes.data_as(C.c_void_p)
    bad = [(1.0, 0.1, 13, 14, 10), (1.0, 0.1, 0, 14, 10), (1.0, 0.1, 14, 0, 10), (1.0, 0.1, 14, 14, 0), (1.0, 0.1, 16, 16, 17),
           (1.0, 0.1, 4098, 1, 1), (1.0, 1.0, 14, 14, 10), (1.0, 2.0, 14, 14, 10), (1.0, 0.0, 14, 14, 10), (1.0, -0.1, 14, 14, 10),
           (0.0, 0.1, 14, 14, 10), (1.0, float("nan"), 14, 14, 10), (float("inf"), 0.1, 14, 14, 10)]
    cloud, kp = np.random.default_rng(0).random((10, 3)), np.zeros((2, 3))
    for R, r0, L, K, J in bad:
        with pytest.raises(ValueError):
            U.check_shape(R, r0, L, K, J)
        assert lib.sf_usc_tables(R, r0, L, K, J, p, p, p, p, p) == -1, (R, r0, L, K, J)
        assert _ffi.last_error().startswith("sf_usc_tables:")
        with pytest.raises(ValueError):
            compute_usc_descriptor(cloud, kp, R, min_radius=r0, azimuth_bins=L, elevation_bins=K, radius_bins=J)
    assert lib.sf_usc_tables(1.0, 0.1, 16, 16, 16, p, p, p, p, p) == 0  # 4096 bins: the cap itself
    assert lib.sf_usc_tables(1.0, 0.1, 14, 14, 10, None, p, p, p, p) == -1
    for kw in (dict(density_radius=0.0), dict(local_rf_radius=-1.0), dict(azimuth_bins=14.5)):
        with pytest.raises((ValueError, TypeError)):
            compute_usc_descriptor(cloud, kp, 1.0, **kw)
    with pytest.raises(ValueError):
        compute_usc_descriptor(cloud[:, :2], kp, 1.0)


# ---- the statement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(14, 14, 10), (12, 11, 15), (4, 2, 1), (2, 1, 1)])
def test_statement_bins_match_atan2_acos_searchsorted(shape):
    L, K, J = shape
    R, r0 = 0.5, 0.05
    rng = np.random.default_rng(11)
    n = 20000
    d = rng.standard_normal((n, 3))
    d *= (rng.random(n) ** (1 / 3) * R * 1.05 / np.linalg.norm(d, axis=1))[:, None]  # (some beyond R, some below r0)
    rot = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    tab = U.tables(R, r0, L, K, J)
    r2, lx, ly, lz = U.local_coordinates(d, rot)
    j, l, k = U.bins(r2, lx, ly, lz, tab, L, K, J)
    r = np.sqrt(r2)
    e = np.sqrt(tab[0])
    phi = np.mod(np.arctan2(ly, lx), 2 * np.pi)
    theta = np.arccos(np.clip(lz / r, -1, 1))
    # away from the edges: 1e-9 of the bin's own unit
    ok = np.abs(r[:, None] / e[None, :] - 1).min(axis=1) > 1e-9
    fa, ft = phi / (2 * np.pi / L), theta / (np.pi / K)
    ok &= (np.abs(fa - np.rint(fa)) > 1e-9) & (np.abs(ft - np.rint(ft)) > 1e-9)
    assert ok.sum() > 0.99 * n
    j_ref = np.searchsorted(e[1:J], r, side="right")
    l_ref = np.minimum(np.floor(fa).astype(int), L - 1)
    k_ref = np.minimum(np.floor(ft).astype(int), K - 1)
    assert np.array_equal(j[ok], j_ref[ok]) and np.array_equal(l[ok], l_ref[ok]) and np.array_equal(k[ok], k_ref[ok])
    assert j.min() == 0 and j.max() == J - 1 and l.max() == L - 1 and k.max() == K - 1 and (r < r0).any() and (r > R).any()


def test_statement_edge_rules():
    """What the comparison rules say ON an edge: r = e[i] belongs to bin i, r = R to the last; the azimuth edge at angle 0
    (ly = 0, lx > 0) to bin 0 and the one at pi (ly = 0, lx < 0) to bin L / 2; the equator lz = 0 with K even to bin K / 2
    (theta = pi / 2 is that bin's lower edge); the poles to bins 0 and K - 1, and their lx = ly = 0 passes every azimuth
    comparison: bin L / 2 - 1."""
    L, K, J = 14, 14, 10
    R, r0 = 1.0, 0.125
    tab = U.tables(R, r0, L, K, J)
    e = np.sqrt(tab[0])
    eye = np.eye(3)
    assert e[0] == r0 and e[J] == R
    on = [i for i in range(J + 1) if e[i] * e[i] == tab[0][i]]  # edges whose square is the tabulated one exactly
    assert 0 in on and J in on
    d = np.array([[e[i], 0.0, 0.0] for i in on])
    r2, lx, ly, lz = U.local_coordinates(d, eye)
    j, l, k = U.bins(r2, lx, ly, lz, tab, L, K, J)
    assert np.array_equal(j, [min(i, J - 1) for i in on]) and (l == 0).all() and (k == K // 2).all()
    d = np.array([[-0.5, 0.0, 0.0], [0.0, 0.0, 0.5], [0.0, 0.0, -0.5], [0.0, 0.5, 0.0], [0.0, -0.5, 0.0], [0.5, 0.0, -0.0]])
    j, l, k = U.bins(*U.local_coordinates(d, eye), tab, L, K, J)
    assert l.tolist() == [L // 2, L // 2 - 1, L // 2 - 1, L // 4, L // 2 + L // 4, 0]  # (14 // 4 = 3: pi / 2 lies inside bin 3)
    assert k.tolist() == [K // 2, 0, K - 1, K // 2, K // 2, K // 2]


def test_statement_conserves_mass():
    """sum_b row[b] / vol[b] = fsum of the weights of the neighbours at non-zero distance: every term carries the rounding of
    one product and one quotient (2 x 2^-53 relative), the fsum over the bins one more."""
    rng = np.random.default_rng(5)
    pts = rng.random((3000, 3))
    w = 1.0 / rng.integers(1, 400, pts.shape[0]).astype(np.float64)
    kp = pts[:40]
    R = 0.2
    lists = [np.flatnonzero(((pts - q) ** 2).sum(axis=1) <= R * R) for q in kp]
    frames = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in kp])
    tab = U.tables(R, R / 10, 14, 14, 10)
    rows = U.rows(pts, kp, lists, frames, w, R, tab=tab)
    assert rows.shape == (40, 1960) and (rows >= 0).all()
    for i, nb in enumerate(lists):
        others = nb[((pts[nb] - kp[i]) ** 2).sum(axis=1) != 0]
        total = math.fsum(w[others])
        assert len(others) == len(nb) - 1 and total > 0
        got = math.fsum(rows[i] / tab[4])
        assert abs(got - total) <= 4 * 2.0 ** -53 * total, (i, got, total)
    # the gate and the norm
    gated = U.rows(pts, kp, lists, frames, w, R, tab=tab, min_neighborhood_size=max(len(a) for a in lists))
    assert not gated.any()
    unit = U.rows(pts, kp, lists, frames, w, R, tab=tab, normalize=True)
    assert np.allclose(np.linalg.norm(unit, axis=1), 1.0, rtol=1e-14, atol=0)


# ---- the exact sums -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def acc(tmp_path_factory):
    """usc_acc.h built for the host with the flags of csrc/Makefile."""
    if HIPCC is None:
        pytest.skip("no hipcc")
    so = str(tmp_path_factory.mktemp("usc_acc_host") / "libusc_acc_host.so")
    r = subprocess.run([HIPCC, "--offload-host-only", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                        "-I", os.path.join(ROOT, "shot_fpfh_amd", "csrc"), os.path.join(ROOT, "tests", "usc_acc_host_shim.hip"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(so)
    lib.usc_acc_split_host.restype, lib.usc_acc_split_host.argtypes = C.c_int, [C.c_double, C.c_void_p, C.c_void_p]
    lib.usc_acc_round_host.restype, lib.usc_acc_round_host.argtypes = C.c_double, [C.c_ulonglong, C.c_ulonglong]
    lib.usc_acc_sum_host.restype, lib.usc_acc_sum_host.argtypes = C.c_double, [C.c_void_p, C.c_int64, C.c_void_p]
    return lib


def acc_sum(lib, w):
    w = np.ascontiguousarray(w, dtype=np.float64)
    rejected = C.c_int64(0)
    s = lib.usc_acc_sum_host(w.ctypes.data, w.size, C.byref(rejected))
    return s, rejected.value


def exact(w):
    """The correctly rounded sum: Fraction arithmetic is exact and float(Fraction) rounds to nearest, ties to even."""
    return float(sum((Fraction(float(x)) for x in w), Fraction(0)))


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def test_split_is_the_weight_in_units_of_2_to_minus_75(acc):
    rng = np.random.default_rng(1)
    cs = np.r_[1, 2, 3, 2 ** 22 - 1, 2 ** 21, 2 ** 21 + 1, rng.integers(1, 2 ** 22, 2000)]
    for c in cs:
        w = 1.0 / float(c)
        lo, hi = C.c_ulonglong(0), C.c_ulonglong(0)
        assert acc.usc_acc_split_host(w, C.byref(lo), C.byref(hi)) == 1
        assert lo.value < 2 ** 40 and hi.value < 2 ** 36
        assert Fraction(hi.value * 2 ** 40 + lo.value, 2 ** 75) == Fraction(w)
    for w in (2.0 ** -22, 1.0, np.nextafter(2.0 ** -22, 1.0), np.nextafter(1.0, 0.0)):  # the closed range's ends: accepted
        lo, hi = C.c_ulonglong(0), C.c_ulonglong(0)
        assert acc.usc_acc_split_host(w, C.byref(lo), C.byref(hi)) == 1
        assert Fraction(hi.value * 2 ** 40 + lo.value, 2 ** 75) == Fraction(float(w))
    for w in (0.0, -0.5, np.nextafter(2.0 ** -22, 0.0), np.nextafter(1.0, 2.0), 2.0, float("inf"), float("nan"), 5e-324):
        lo, hi = C.c_ulonglong(7), C.c_ulonglong(9)
        assert acc.usc_acc_split_host(w, C.byref(lo), C.byref(hi)) == 0
        assert (lo.value, hi.value) == (7, 9)


def test_limb_sums_of_random_counts_are_the_exact_sum(acc):
    rng = np.random.default_rng(2)
    for trial in range(300):
        n = int(rng.integers(1, 3000))
        top = int(rng.choice([4, 60, 1000, 2 ** 22]))
        w = 1.0 / rng.integers(1, top, n).astype(np.float64)
        got, rejected = acc_sum(acc, w)
        assert rejected == 0
        want = exact(w)
        assert same_bits(got, want) and same_bits(got, math.fsum(w)), (trial, got, want)
    assert acc_sum(acc, np.zeros(0)) == (0.0, 0)


def test_limb_sums_without_rounding(acc):
    """All ones, and powers of two: every partial sum is representable, the result is the plain sum."""
    for n in (1, 2, 63, 64, 65, 1000, 2 ** 16 + 1):
        got, _ = acc_sum(acc, np.ones(n))
        assert same_bits(got, float(n))
    rng = np.random.default_rng(3)
    for trial in range(100):
        w = 2.0 ** -rng.integers(0, 23, int(rng.integers(1, 500))).astype(np.float64)
        got, rejected = acc_sum(acc, w)
        assert rejected == 0 and same_bits(got, exact(w)) and same_bits(got, float(np.sum(w)))
    got, rejected = acc_sum(acc, [0.5, 3.0, 0.25, float("nan"), 1e-9])
    assert rejected == 3 and got == 0.75


def test_limb_sums_at_constructed_ties(acc):
    """Sums exactly halfway between two doubles go to the even one, and one unit of 2^-75 either side of the tie decides."""
    eps = 2.0 ** -52
    for odd in range(1, 40):
        w = [2.0 ** -22 * (1 + odd * eps), 2.0 ** -22]  # sum = 2^-21 (1 + odd 2^-53): a tie when odd is odd
        got, _ = acc_sum(acc, w)
        want = exact(w)
        assert same_bits(got, want)
        if odd % 2:
            assert int(np.float64(got).view(np.uint64)) & 1 == 0, "a tie goes to the even mantissa"
    # on the limbs themselves: S = (M << (k + 1)) + half + delta for 53-bit M, delta in {-1, 0, +1}, split every which way
    rng = np.random.default_rng(4)
    for trial in range(2000):
        M = (1 << 52) | int(rng.integers(0, 1 << 52))
        k = int(rng.integers(0, 45))  # S < 2^99
        for delta in (-1, 0, 1):
            S = (M << (k + 1)) + (1 << k) + delta
            hi = S >> 40
            move = int(rng.integers(0, min(hi, (1 << 23)) + 1))  # lo may hold up to 2^64 - 1: carry some of hi there
            lo = (S & ((1 << 40) - 1)) + (move << 40)
            hi -= move
            assert lo < 2 ** 64 and hi < 2 ** 64 and hi * 2 ** 40 + lo == S
            got = acc.usc_acc_round_host(lo, hi)
            want = float(Fraction(S, 2 ** 75))
            assert same_bits(got, want), (hex(S), got, want)
            if delta == 0 and k > 0:
                assert int(np.float64(got).view(np.uint64)) & 1 == 0
    # short sums: 53 bits or fewer are exact; the first that is not
    for S in (0, 1, 2 ** 40 - 1, 2 ** 40, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 54 + 2, 2 ** 54 + 3, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 2 ** 11,
              2 ** 64 + 3 * 2 ** 11, 2 ** 99 + 2 ** 46, 2 ** 99 + 3 * 2 ** 46):
        got = acc.usc_acc_round_host(S & ((1 << 40) - 1), S >> 40)
        assert same_bits(got, float(Fraction(S, 2 ** 75))), hex(S)


# ---- the build ----------------------------------------------------------------------------------------------------------------
def test_usc_kernels_do_not_spill():
    path = os.path.join(ROOT, "shot_fpfh_amd", "csrc", "build", "usc.remarks")
    if not os.path.exists(path):
        pytest.skip("no build/usc.remarks (the library was not built by its Makefile here)")
    res, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", ln)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    # (k_usc, and search_util.h's two maps between the caller's and the cell-sorted order, which took over from k_usc_weights and
    # k_usc_sort_weights)
    patterns = ("k_usc", "k_perm_scatter", "k_perm_gather")
    kernels = {name: r for name, r in res.items() if any(p in name for p in patterns)}
    assert len(kernels) >= 3 and all(any(p in name for name in kernels) for p in patterns), sorted(res)
    for name, r in kernels.items():
        assert r.get("VGPRs Spill", 0) <= 4 and r.get("ScratchSize", 0) == 0, (name, r)
