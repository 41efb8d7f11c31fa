"""The NumPy statement of Point Feature Histograms (K22): what tests/test_pfh_host.py checks against closed forms and the direct
formulas, and tests/test_hip_pfh.py holds the device to, bit for bit.  Modelled on pcl::computePairFeatures and
pcl::PFHEstimation::computePointPFHSignature, decided here so that a row is a pure function of the cloud: it never depends on
the order of a list or of the cloud, and no bin depends on atan2, acos or a division.

All arithmetic is unfused float64, elementwise, in the order written; dot products are (x0 y0 + x1 y1) + x2 y2, cross products
the usual component formulas.

Parameters: radius R; n_bins S, 1 <= S <= 16; rows of S^3.
Tables (sf_pfh_tables -- `tables`; their NumPy formulas are `tables_numpy`), S + 1 entries each, the interior ones 1 .. S - 1 used:
         c[i] = -1 + 2 i / S, c[0] = -1, c[S] = 1, c[S / 2] = 0 (S even) exactly;  q = c |c|
         e[i] = -pi + 2 pi i / S;  ca[i], sa[i] = cos, sin(e[i]), (1, 0) exactly where e[i] = 0;  g[i] = sign(2 i - S)
A keypoint's list has k entries; every unordered pair {s, t} of them is visited once:
      1. d = p_t - p_s;  d2 = d.d;  skipped when d2 == 0
      2. a_s = n_s.d;  a_t = -(n_t.d)
      3. the source: t when |a_t| > |a_s|, s when |a_s| > |a_t|; on equality the one with the larger signed value; if those are
         equal too, the one whose coordinates come first in (x, y, z) lexicographic order.  t the source: d := -d.
         n1 = the source's normal, n2 = the other's, num3 = the source's value
      4. v = d x n1;  v2 = v.v;  skipped when v2 == 0
      5. num2 = v.n2;  w = n1 x v;  a = w.n2;  B = (n1.n2) sqrt(v2);  a == 0 and B == 0: B := 1
      6. b3 = #{1 <= i < S : num3 |num3| >= q[i] d2}                       (phi = n1.d / |d|)
         b2 = #{1 <= i < S : num2 |num2| >= q[i] v2}                       (alpha = v.n2 / |v|)
         b1 = #{1 <= i < S : ge_i}                                         (theta = atan2(a, B) over (-pi, pi])
              X_i = (ca[i] a - sa[i] B >= 0), up = (a >= 0);  ge_i = up or X_i where g[i] < 0, up and X_i where g[i] > 0,
              up where g[i] = 0
      7. count[b1 + S b2 + S^2 b3] += 1
Row:     row[b] = (100.0 count[b]) / P, P = k (k - 1) / 2 (every pair of the list, the skipped ones included); zeros for k < 2.
p_s - p_t is the exact negation of p_t - p_s and the source rule is symmetric: any enumeration of the pairs gives the same counts.
"""
import ctypes as C

import numpy as np

MAX_BINS = 16
MAX_LIST = 65536  # a list this long or longer is refused (P must stay below 2^32)


def check_bins(S):
    if not 1 <= S <= MAX_BINS:
        raise ValueError("1 <= n_bins <= 16")


def tables(S):
    """(q, ca, sa, g) as the library computes them (sf_pfh_tables: host only, no GPU)."""
    from shot_fpfh_amd import _ffi

    check_bins(S)
    q, ca, sa, g = np.zeros(S + 1), np.zeros(S + 1), np.zeros(S + 1), np.zeros(S + 1, dtype=np.int32)
    rc = _ffi.load().sf_pfh_tables(S, *(a.ctypes.data_as(C.c_void_p) for a in (q, ca, sa, g)))
    assert rc == 0, _ffi.last_error()
    return q, ca, sa, g


def tables_numpy(S):
    """The same four tables from NumPy's own cos / sin (ca and sa equal to the library's within an ulp or two, q and g bit-equal)."""
    check_bins(S)
    i = np.arange(S + 1)
    c = -1.0 + 2.0 * i / S
    c[0], c[S] = -1.0, 1.0
    if S % 2 == 0:
        c[S // 2] = 0.0
    e = -np.pi + 2.0 * np.pi * i / S
    g = np.sign(2 * i - S).astype(np.int32)
    return c * np.abs(c), np.where(g == 0, 1.0, np.cos(e)), np.where(g == 0, 0.0, np.sin(e)), g


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def pair_features(ps, ns, pt, nt):
    """Steps 1-5 for arrays of pairs (each argument p x 3): a dict of keep, d2, v2, num3, num2, a, B, and `branch`, which rule
    of step 3 decided the source (0: |.|, 1: the signed value, 2: the coordinates) -- and `tsrc`, whether t is the source."""
    d = pt - ps
    d2 = _dot(d, d)
    a_s = _dot(ns, d)
    a_t = -_dot(nt, d)
    fs, ft = np.abs(a_s), np.abs(a_t)
    t_first = (d[:, 0] < 0) | ((d[:, 0] == 0) & ((d[:, 1] < 0) | ((d[:, 1] == 0) & (d[:, 2] < 0))))  # p_t before p_s
    tsrc = (ft > fs) | ((ft == fs) & ((a_t > a_s) | ((a_t == a_s) & t_first)))
    branch = np.where(ft != fs, 0, np.where(a_t != a_s, 1, 2))
    d = np.where(tsrc[:, None], -d, d)
    n1 = np.where(tsrc[:, None], nt, ns)
    n2 = np.where(tsrc[:, None], ns, nt)
    num3 = np.where(tsrc, a_t, a_s)
    v = _cross(d, n1)
    v2 = _dot(v, v)
    num2 = _dot(v, n2)
    w = _cross(n1, v)
    a = _dot(w, n2)
    B = _dot(n1, n2) * np.sqrt(v2)
    B = np.where((a == 0) & (B == 0), 1.0, B)
    return dict(keep=(d2 != 0) & (v2 != 0), d2=d2, v2=v2, num3=num3, num2=num2, a=a, B=B, branch=branch, tsrc=tsrc)


def rule_bins(f, tab, S):
    """(b1, b2, b3) of pairs given by their features, by the comparison rules of step 6."""
    q, ca, sa, g = tab
    it = slice(1, S)
    b3 = ((f["num3"] * np.abs(f["num3"]))[:, None] >= q[None, it] * f["d2"][:, None]).sum(axis=1)
    b2 = ((f["num2"] * np.abs(f["num2"]))[:, None] >= q[None, it] * f["v2"][:, None]).sum(axis=1)
    X = ca[None, it] * f["a"][:, None] - sa[None, it] * f["B"][:, None] >= 0
    up = (f["a"] >= 0)[:, None]
    gi = g[None, it]
    ge = np.where(gi < 0, up | X, np.where(gi > 0, up & X, up))
    return ge.sum(axis=1), b2, b3


def formula_bins(f, S):
    """(b1, b2, b3) by the direct formulas of PCL: phi and alpha by division, theta by arctan2, and
    bin = clip(floor(S (f - lo) / (hi - lo)), 0, S - 1); with them `margin`, each pair's distance from the nearest bin edge in bin
    widths (the smallest over the three features)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        f3 = f["num3"] / np.sqrt(f["d2"])
        f2 = f["num2"] / np.sqrt(f["v2"])
    f1 = np.arctan2(f["a"], f["B"])
    bins, margin = [], np.full(f1.shape, np.inf)
    for val, lo, hi in ((f1, -np.pi, np.pi), (f2, -1.0, 1.0), (f3, -1.0, 1.0)):
        pos = S * (val - lo) / (hi - lo)
        bins.append(np.clip(np.floor(pos), 0, S - 1).astype(np.int64))
        inner = (pos > 0.5) & (pos < S - 0.5)  # (the outer edges are clipped: no decision hangs on them)
        margin = np.minimum(margin, np.where(inner, np.abs(pos - np.rint(pos)), np.inf))
    return bins[0], bins[1], bins[2], margin


def list_pairs(points, normals, nb):
    """The features of every unordered pair of the list `nb` (indices into points), s < t by list position."""
    nb = np.asarray(nb, dtype=np.int64)
    s, t = np.triu_indices(nb.size, 1)
    return pair_features(points[nb[s]], normals[nb[s]], points[nb[t]], normals[nb[t]])


def counts(points, normals, nb, S, tab=None):
    """The S^3 integer counts of one list, and how many of its pairs were skipped."""
    tab = tables(S) if tab is None else tab
    f = list_pairs(points, normals, nb)
    keep = f["keep"]
    b1, b2, b3 = rule_bins({k: v[keep] for k, v in f.items()}, tab, S)
    return np.bincount(b1 + S * b2 + S * S * b3, minlength=S ** 3).astype(np.int64), int((~keep).sum())


def rows(points, normals, lists, S=5, tab=None):
    """The m x S^3 rows of the neighbourhoods `lists` (index arrays into points)."""
    tab = tables(S) if tab is None else tab
    out = np.zeros((len(lists), S ** 3))
    for i, nb in enumerate(lists):
        k = len(nb)
        if k < 2:
            continue
        if k >= MAX_LIST:
            raise ValueError("a list of 65 536 entries or more")
        cnt, _ = counts(points, normals, nb, S, tab)
        out[i] = (100.0 * cnt.astype(np.float64)) / float(k * (k - 1) // 2)
    return out


def near_edge_fixture(S):
    """Pairs whose numerators sit exactly on bin edges, one two-entry list each: (points, normals, lists, want), want[i] the
    (b1, b2, b3) a closed form predicts for pair i, or None where only the statement speaks.
    Pair i is s = (4 i, 0, 0), t = s + (1, 0, 0), n_s = (h, 1, 0), n_t = (x, y, z) with |x| < |h| (or a tie that the coordinates
    give to s), every number dyadic or a table entry, so that exactly: d2 = 1, num3 = h, v = (0, 0, 1), v2 = 1, num2 = z,
    a = x - h y, B = h x + y."""
    c = -1.0 + 2.0 * np.arange(S + 1) / S
    c[0], c[S] = -1.0, 1.0
    if S % 2 == 0:
        c[S // 2] = 0.0
    mid = S // 2  # the bin of a feature at the centre of its range: floor(S / 2)
    cases = [  # (h, (x, y, z), want)
        (0.5, (0.25, 0.5, 0.0), (mid, mid, None)),       # theta = 0: a = 0, B > 0
        (0.5, (-0.25, -0.5, 0.0), (S - 1, mid, None)),   # theta = pi: a = 0, B < 0
        (0.5, (0.0, 0.0, 0.0), (mid, mid, None)),        # a = B = 0: B := 1, theta = 0
        (0.5, (0.25, -0.125, 0.0), ((3 * S) // 4 if S % 4 == 0 else None, mid, None)),  # theta = pi / 2: B = 0, a > 0
        # theta = -pi / 2 (B = 0, a < 0): the rounded edge e[S / 4] lies above -pi / 2 (cos of it is +6e-17), so the bin below
        (0.5, (-0.25, 0.125, 0.0), (S // 4 - 1 if S % 4 == 0 else None, mid, None)),
        (0.0, (0.0, 1.0, 0.25), (None, None, mid)),      # phi = 0 by a tie of +0 and -0 that the coordinates give to s
    ]
    for i in range(1, S):
        if c[i] != 0.0:
            cases.append((0.5, (0.25, 0.5, c[i]), (mid, i, None)))                        # alpha on edge i: bin i
            cases.append((0.5, (0.25, 0.5, np.nextafter(c[i], -2.0)), (mid, i - 1, None)))  # one ulp below: bin i - 1
            cases.append((c[i], (0.0, 1.0, 0.25), (None, None, i)))                       # phi on edge i
            cases.append((np.nextafter(c[i], -2.0), (0.0, 1.0, 0.25), (None, None, i - 1)))
    n = len(cases)
    points = np.zeros((2 * n, 3))
    normals = np.zeros((2 * n, 3))
    points[0::2, 0] = 4.0 * np.arange(n)
    points[1::2, 0] = 4.0 * np.arange(n) + 1.0
    for i, (h, nt, _) in enumerate(cases):
        normals[2 * i] = (h, 1.0, 0.0)
        normals[2 * i + 1] = nt
    return points, normals, [np.array([2 * i, 2 * i + 1]) for i in range(n)], [w for _, _, w in cases]
