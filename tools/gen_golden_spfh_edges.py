#!/usr/bin/env python3
"""Generate tests/golden/spfh_edges.npz by IMPORTING the reference (aubin-tchoi/shot-fpfh): compute_fpfh_descriptor
(fpfh.py:16-117) on clouds built so that the SPFH pair features (alpha, phi, theta) land on or next to histogram edges.

Runs only in the build container, where /root/reference exists:

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_spfh_edges.py

Stores only data.  A case is one cloud (float64 points and normals, stored exactly) with one or more runs (radius, n_bins);
keypoints are `<case>_kp` and the SPFH rows kept are those of `<case>_spfh_sel` (both stored for the planes only; every point
otherwise).  `<case>_runs` holds one (radius, n_bins, ndiff) row per run j; rows are sparse (_i flat int32 indices into the
dense (rows, n_bins^3) array, _v values):
  <case>_r<j>_con_*   the CONTRACT FPFH rows: the reference's expressions with `.dot(u)` (phi's numerator, theta's denominator)
                      replaced by the index-order sum plus +0.0, and np.arctan2 by the C library's atan2 -- what the C
                      oracle and K6 compute
  <case>_r<j>_ref_*   the reference's FPFH rows, stored only when ndiff > 0 (else they ARE the contract rows)
  <case>_r<j>_spfh_*  the contract SPFH rows
ndiff counts the rows where contract and reference differ; the generator asserts that each one has a pair in its
neighbourhood whose phi or theta bin flips between the two evaluations.
The contract's alpha and theta numerator are the reference's own (np.einsum, whose order this script checks), so the gaps
are OpenBLAS gemv's rounding of the two dot products, which depends on the CPU and on the matrix's shape, and numpy's
SIMD arctan2, which can round an ulp away from the correctly rounded value (it decides a few of the exact theta edges).

Cases: signed_zero (axis-aligned normals with +-0 components), plane_t0..2 (exact tilted planes), edge_pt_<n> (phi and theta
on and around every interior edge, theta around +-pi/2), edge_a_<n> (alpha on and around every interior edge), theta_cancel
(theta near edges where the triple-product form cancels), reach_<n>_<s> (radius * max|n|^2 on and around the nearest alpha
edge that K6's alpha shortcut / pair form / windowed table depends on).
"""
from __future__ import annotations

import math
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import sklearn  # noqa: E402
from shot_fpfh.descriptors.fpfh import compute_fpfh_descriptor  # noqa: E402
from sklearn.neighbors import KDTree  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
VERSIONS = np.array([f"numpy {np.__version__}", f"scipy {scipy.__version__}", f"sklearn {sklearn.__version__}"])
NS_EDGE = [2, 3, 4, 5, 6, 7, 8, 9, 11, 16]
PI = np.pi


def edges(n):
    return np.linspace(-1, 1, n + 1), np.linspace(-PI / 2, PI / 2, n + 1)


def hbin(e, x):
    """np.histogramdd's rule: searchsorted(e, x, 'right') - 1, x == last edge -> last bin, outside / NaN -> -1."""
    x = np.asarray(x, dtype=np.float64)
    b = np.searchsorted(e, x, side="right") - 1
    b = np.where(x == e[-1], len(e) - 2, b)
    return np.where((x >= e[0]) & (x <= e[-1]), b, -1)


# ---- the pair features, vectorised over rows (u fixed): the reference's expressions (fpfh.py:47-57) ----------------------
def seq_dot(m, u):
    """The contract's dot product: index order, a zero result is +0.0 (a BLAS accumulator starts from +0)."""
    return ((m[:, 0] * u[0] + m[:, 1] * u[1]) + m[:, 2] * u[2]) + 0.0


def libm_atan2(a, b):
    """The C library's atan2 (correctly rounded in glibc); numpy's own SIMD arctan2 can be an ulp away from it."""
    return np.array([math.atan2(x, y) for x, y in zip(a, b)], dtype=np.float64)


def features(c, u, nj, blas=True):
    """blas: the reference's expressions; else the contract's (index-order dot products + 0.0, the C library's atan2)."""
    dot = (lambda m, x: m.dot(x)) if blas else seq_dot
    atan2 = np.arctan2 if blas else libm_atan2
    dist = np.linalg.norm(c, axis=1)
    v = np.cross(c, u)
    w = np.cross(u, v)
    alpha = np.einsum("ij,ij->i", v, nj)
    phi = dot(c, u) / dist
    theta = atan2(np.einsum("ij,ij->i", nj, w), dot(nj, u))
    return alpha, phi, theta


def check_numpy_orders():
    """What the oracle and K6 assume of numpy: einsum sums (x0 y0 + x2 y2) + x1 y1 and starts from +0; np.cross is the textbook
    difference of products; np.linalg.norm(axis=1) is sqrt((x0^2 + x1^2) + x2^2).  A numpy that changes any of these fails here."""
    rng = np.random.default_rng(77)
    for n in (1, 2, 3, 7, 8, 9, 16, 17, 100, 3000):
        x, y = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
        e = np.einsum("ij,ij->i", x, y)
        assert np.array_equal(e, ((x[:, 0] * y[:, 0] + x[:, 2] * y[:, 2]) + x[:, 1] * y[:, 1]) + 0.0), n
        u = y[0]
        cr = np.stack([x[:, 1] * u[2] - x[:, 2] * u[1], x[:, 2] * u[0] - x[:, 0] * u[2], x[:, 0] * u[1] - x[:, 1] * u[0]], 1)
        assert np.array_equal(np.cross(x, u), cr), n
        cr = np.stack([u[1] * x[:, 2] - u[2] * x[:, 1], u[2] * x[:, 0] - u[0] * x[:, 2], u[0] * x[:, 1] - u[1] * x[:, 0]], 1)
        assert np.array_equal(np.cross(u, x), cr), n
        assert np.array_equal(np.linalg.norm(x, axis=1), np.sqrt((x[:, 0] ** 2 + x[:, 1] ** 2) + x[:, 2] ** 2)), n
    z = np.array([[-0.0, -0.0, -1.0]])
    assert not np.signbit(np.einsum("ij,ij->i", z, np.array([[1.0, 0.0, 0.0]]))[0])


# ---- reference-shaped SPFH / FPFH with either dot product, per pair bins for the flip check -----------------------------
def shaped(p, nr, radius, n, kp, blas):
    lists, dists = KDTree(p).query_radius(p, radius, return_distance=True)
    ea, et = edges(n)
    spfh = np.zeros((p.shape[0], n**3))
    pair_bins = []
    for i in range(p.shape[0]):
        nbr = lists[i]
        c = p[nbr] - p[i]
        far = np.linalg.norm(c, axis=1) > 0
        a, ph, th = features(c[far], nr[i], nr[nbr][far], blas)
        ba, bp, bt = hbin(ea, a), hbin(ea, ph), hbin(et, th)
        pair_bins.append(np.stack([ba, bp, bt], 1))
        ok = (ba >= 0) & (bp >= 0) & (bt >= 0)
        np.add.at(spfh[i], ((ba * n + bp) * n + bt)[ok], 1.0)
        spfh[i] /= nbr.shape[0]
    out = np.zeros((len(kp), n**3))
    for row, q in enumerate(kp):
        nbr, d = lists[q], dists[q]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[row] = spfh[q] + (spfh[nbr] / d[:, None])[d > 0].sum(axis=0) / nbr.shape[0]
    return out, spfh, pair_bins, lists


def put_sparse(arrs, key, m):
    flat = m.ravel()
    nz = np.flatnonzero(flat)
    assert flat.size < 2**31
    arrs[key + "_i"], arrs[key + "_v"] = nz.astype(np.int32), flat[nz]


def run_case(arrs, case, p, nr, runs, kp=None, spfh_sel=None, counts=None):
    """runs: list of (radius, n_bins).  Reference rows, contract rows, and the check that they differ only where a bin flips."""
    kp = np.arange(p.shape[0]) if kp is None else np.asarray(kp)
    spfh_sel = np.arange(p.shape[0]) if spfh_sel is None else np.asarray(spfh_sel)
    arrs[f"{case}_points"], arrs[f"{case}_normals"] = p, nr
    if len(kp) != p.shape[0] or len(spfh_sel) != p.shape[0]:
        arrs[f"{case}_kp"], arrs[f"{case}_spfh_sel"] = kp.astype(np.int32), spfh_sel.astype(np.int32)
    table = []
    for j, (radius, n) in enumerate(runs):
        ref = compute_fpfh_descriptor(kp, p, nr, radius, n, verbose=False)
        blas, _, bins_b, lists = shaped(p, nr, radius, n, kp, True)
        assert np.array_equal(blas, ref), f"{case} run {j}: the reference-shaped rows are not the reference's"
        con, spfh_c, bins_c, _ = shaped(p, nr, radius, n, kp, False)
        flipped = np.array([not np.array_equal(a, b) for a, b in zip(bins_b, bins_c)])
        for i in np.flatnonzero(flipped):  # alpha is the same expression on both sides: only phi or theta can move
            assert np.array_equal(bins_b[i][:, 0], bins_c[i][:, 0])
        near = np.array([flipped[lists[q]].any() for q in kp])
        diff = np.any(con != ref, axis=1)
        assert not (diff & ~near).any(), f"{case} run {j}: contract rows differ where no bin flipped"
        ndiff = int(diff.sum())
        k = f"{case}_r{j}"
        table.append((radius, n, ndiff))
        if ndiff:
            put_sparse(arrs, k + "_ref", ref)
        put_sparse(arrs, k + "_con", con)
        put_sparse(arrs, k + "_spfh", spfh_c[spfh_sel])
        if counts is not None:
            counts.append((case, radius, n, len(kp), ndiff, int(flipped.sum())))
        print(f"  {case} r={radius!r} n={n}: {len(kp)} rows, contract != reference on {ndiff}, {int(flipped.sum())} points flip a bin")
    arrs[f"{case}_runs"] = np.array(table, dtype=np.float64)  # radius, n_bins, rows where contract != reference


# ---- isolated pairs ------------------------------------------------------------------------------------------------
class Pairs:
    """Point pairs on a grid of the z = 0 plane, `spacing` apart (more than twice the radius: every list is the point itself
    plus its partner).  A base point has z = 0 exactly, so the partner's z offset keeps every bit."""

    def __init__(self, spacing, offset=(0.0, 0.0, 0.0)):
        self.spacing, self.offset, self.rows = spacing, np.asarray(offset, dtype=np.float64), []

    def base(self):
        k = len(self.rows)
        return self.offset + np.array([self.spacing * (k % 32), self.spacing * (k // 32), 0.0])

    def add(self, pi, ui, pj, nj):
        self.rows.append((pi, ui, pj, nj))

    def arrays(self):
        p = np.array([x for r in self.rows for x in (r[0], r[2])], dtype=np.float64)
        nr = np.array([x for r in self.rows for x in (r[1], r[3])], dtype=np.float64)
        return p, nr


def ulps(x, k):
    """x moved by k ulps (vectorised over k)."""
    x = np.float64(x)
    out = np.empty(len(k))
    for t, kk in enumerate(k):
        y = x
        for _ in range(abs(int(kk))):
            y = np.nextafter(y, np.inf if kk > 0 else -np.inf)
        out[t] = y
    return out


def ulp_grid(x, half):
    """x and its neighbours up to `half` ulps away, by x + m * spacing (exact while x stays within its binade)."""
    sp = np.spacing(np.float64(x)) if x != 0 else np.float64(5e-324)
    return np.float64(x) + np.arange(-half, half + 1) * sp


def targets(e, n):
    """The values a feature is steered to around edge e: on it, +-1 and +-2 ulps, +-1e-13 and +-1e-9 relative (1 for e = 0)."""
    s = abs(e) if e != 0 else 1.0
    exact = list(ulps(e, [0, 1, -1, 2, -2]))
    return [(t, True) for t in exact] + [(e + d * s, False) for d in (1e-13, -1e-13, 1e-9, -1e-9)]


def pick(vals, t, exact, e):
    """Index of the candidate that hits t exactly (exact targets), else the closest one on t's side of the edge e."""
    if exact:
        hit = np.flatnonzero(vals == t)
        if hit.size:
            return hit[hit.size // 2], True
    side = (vals > e) if t > e else (vals < e) if t < e else (vals == e)
    cand = np.flatnonzero(side)
    if not cand.size:
        return None, False
    return cand[np.argmin(np.abs(vals[cand] - t))], False


def search(pr, u, pj0, nj0, a_comp, b_comp, feat, t, exact, e, half=200):
    """Scan partner position component a_comp ('p', k) / normal component ('n', k) over ulp grids; keep the pair that puts
    feature `feat` (0 alpha, 1 phi, 2 theta: the reference's expressions) on target t."""
    pi = pr.base()
    pj0 = pi + np.asarray(pj0, dtype=np.float64)
    ga = ulp_grid((pj0 if a_comp[0] == "p" else nj0)[a_comp[1]], half)
    gb = ulp_grid((pj0 if b_comp[0] == "p" else nj0)[b_comp[1]], half)
    A, B = np.meshgrid(ga, gb, indexing="ij")
    m = A.size
    pj = np.tile(pj0, (m, 1))
    nj = np.tile(np.asarray(nj0, dtype=np.float64), (m, 1))
    for comp, vals in ((a_comp, A.ravel()), (b_comp, B.ravel())):
        (pj if comp[0] == "p" else nj)[:, comp[1]] = vals
    with np.errstate(invalid="ignore", divide="ignore"):
        f = features(pj - pi, u, nj)[feat]
    k, hit = pick(f, t, exact, e)
    if k is None:
        return exact
    pr.add(pi, np.asarray(u, dtype=np.float64), pj[k], nj[k])
    return exact and not hit  # (an exact target missed)


def edge_pt_case(n, radius):
    """phi and theta on / around every interior edge (partner 0.04 away, u = +-z: c.u and n_j.u are exact in any order), theta
    around +-pi/2 (b tiny, +-0)."""
    ea, et = edges(n)
    pr = Pairs(3 * radius)
    miss = 0
    for e in ea[1:-1]:  # phi = c_z / |c| with u = +z
        for t, ex in targets(e, n):
            cx = 0.03
            cz = t * cx / np.sqrt(max(1 - t * t, 1e-300))
            miss += search(pr, np.array([0.0, 0.0, 1.0]), [cx, 0.0, cz], np.array([0.6, 0.0, 0.8]), ("p", 2), ("p", 0), 1, t, ex, e)
    for e in et[1:-1]:  # theta = atan2(n0 c_x, n2) with u = +z, c = (c_x, 0, c_z)
        for t, ex in targets(e, n):
            cx = 0.035
            nj = np.array([np.tan(t), 0.0, cx])
            nj /= np.linalg.norm(nj)
            miss += search(pr, np.array([0.0, 0.0, 1.0]), [cx, 0.0, 0.01], nj, ("n", 0), ("n", 2), 2, t, ex, e)
    for sgn in (1.0, -1.0):  # theta around +-pi/2: b = n_j . u tiny, +-0
        for b in (0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, 1e-17, -1e-17, 1e-16, -1e-16, 1e-14, -1e-14, 1e-13, -1e-13,
                  2e-13, -2e-13, 1e-12, -1e-12):
            pi = pr.base()
            pr.add(pi, np.array([0.0, 0.0, 1.0]), pi + np.array([sgn * 0.035, 0.0, 0.01]), np.array([1.0, 0.0, b]))
    return pr, miss


def edge_a_case(n, radius):
    """alpha = (c x u) . n_j on / around every interior alpha edge, u and n_j general unit vectors (all three einsum terms
    non-zero, so its order matters)."""
    ea, _ = edges(n)
    pr = Pairs(3 * radius)
    rng = np.random.default_rng(900 + n)
    miss = 0
    for e in ea[1:-1]:
        for t, ex in targets(e, n):
            u = rng.standard_normal(3)
            u /= np.linalg.norm(u)
            nj = rng.standard_normal(3)
            nj /= np.linalg.norm(nj)
            g = np.cross(u, nj)  # alpha = c . (u x n_j): walk c along g to the target, keeping |c| <= 0.85 radius
            c0 = rng.standard_normal(3)
            c0 -= g * (c0 @ g) / (g @ g)
            c0 *= 0.3 * radius / np.linalg.norm(c0)
            c = c0 + g * (t / (g @ g))
            if np.linalg.norm(c) > 0.85 * radius or abs(g[2]) < 0.2:
                c = g * (t / (g @ g))
            miss += search(pr, u, c, nj, ("p", 2), ("n", 0), 0, t, ex, e, half=150)
    return pr, miss


def theta_cancel_case(radius):
    """theta near its edges where a = n_j . (u x (c x u)) cancels: c nearly parallel to u, |c| near r, normals of norm 1 +- a
    few ulps and 2.0, and a cloud offset by (4096, -2048, 1024) (coarse coordinates, c rounded)."""
    rng = np.random.default_rng(31)
    out = []
    for offset in ((0.0, 0.0, 0.0), (4096.0, -2048.0, 1024.0)):
        pr = Pairs(3 * radius, offset)
        for scale in (1.0, ulps(1.0, [3])[0], ulps(1.0, [-3])[0], 2.0):
            for n in (2, 4, 5, 8):
                _, et = edges(n)
                for e in et[1:-1]:
                    for psi in (1e-3, 1e-6, 1e-8):
                        u = rng.standard_normal(3)
                        u *= scale / np.linalg.norm(u)
                        tdir = np.cross(u, rng.standard_normal(3))
                        tdir /= np.linalg.norm(tdir)
                        uh = u / np.linalg.norm(u)
                        c = 0.97 * radius * (np.cos(psi) * uh + np.sin(psi) * tdir)
                        th = np.arctan(np.tan(e) * np.linalg.norm(u) / np.sin(psi) / (0.97 * radius))  # a / b = tan(e)
                        nj = np.cos(th) * uh + np.sin(th) * tdir
                        nj *= scale / np.linalg.norm(nj)
                        for t, ex in targets(e, n)[:3]:
                            search(pr, u, c, nj, ("n", 0), ("n", 1), 2, t, ex, e, half=40)
        out.append(pr)
    return out


def reach_case(n, s):
    """Isolated pairs with |c| = r exactly, c perpendicular to u and n_j = s e_z: alpha = r s^2 (rounded), right at the reach
    radius * max|n|^2 that K6's alpha shortcut tests, for radii on and around the boundary edge."""
    ea, _ = edges(n)
    bnd = ea[n // 2 + 1]  # odd n: the first positive edge (the shortcut's); even n: the one past the edge at 0 (the pair form's)
    n2 = s * s
    r0 = bnd / n2
    radii = sorted(set(list(ulps(r0, [0, 1, -1, 2, -2])) + [r0 * (1 + 1e-9), r0 * (1 - 1e-9)]))
    pr = Pairs(3.0)
    for r in radii:
        for sx in (1.0, -1.0):
            for sz in (1.0, -1.0):
                pi = pr.base()
                pr.add(pi, np.array([0.0, s, 0.0]), pi + np.array([sx * r, 0.0, 0.0]), np.array([0.0, 0.0, sz * s]))
        pi = pr.base()  # a partner just inside, one with a general direction
        pr.add(pi, np.array([0.0, s, 0.0]), pi + np.array([0.999 * r, 0.0, 0.0]), np.array([0.0, 0.0, s]))
    return pr, radii


def signed_zero_case():
    """Axis-aligned normals with every sign pattern of their zero components, partner along n_j's axis: n_j . u = +-0 while
    n_j . w != 0.  Then clusters of k = 2..9 points, each with one such neighbour at some position of the lists."""
    rng = np.random.default_rng(12)
    normals = []
    for ax in range(3):
        for sg in (1.0, -1.0):
            for z0 in (0.0, -0.0):
                for z1 in (0.0, -0.0):
                    v = np.empty(3)
                    v[ax], v[(ax + 1) % 3], v[(ax + 2) % 3] = sg, z0, z1
                    normals.append(v)
    pr = Pairs(0.5)
    pi = pr.base()  # the case of the issue: normals (-0, -0, -1) and (1, 0, 0), partner 0.1 along x
    pr.add(pi, np.array([-0.0, -0.0, -1.0]), pi + np.array([0.1, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    for u in normals:
        ax = int(np.flatnonzero(u != 0)[0])
        for nj in [m for m in normals if np.flatnonzero(m != 0)[0] != ax][::3]:
            bx = int(np.flatnonzero(nj != 0)[0])
            c = np.zeros(3)
            c[bx] = rng.choice([0.1, -0.1])
            pi = pr.base()
            pr.add(pi, u, pi + c, nj)
    p, nr = pr.arrays()
    # clusters: a centre with normal (-0, -0, -1), one neighbour at +x with normal (1, -0, 0), k - 2 random neighbours
    extra_p, extra_n = [], []
    base0 = np.array([0.0, 40.0, 0.0])
    for k in range(2, 10):
        for rep in range(3):
            b = base0 + np.array([0.5 * (3 * (k - 2) + rep), 0.0, 0.0])
            pts = [b, b + np.array([0.1, 0.0, 0.0])]
            nrm = [np.array([-0.0, -0.0, -1.0]), np.array([1.0, -0.0, 0.0])]
            for _ in range(k - 2):
                d = rng.standard_normal(3)
                pts.append(b + 0.1 * rng.random() * d / np.linalg.norm(d))
                m = rng.standard_normal(3)
                nrm.append(m / np.linalg.norm(m))
            order = rng.permutation(k)  # (the list order is the tree's; shuffling the storage moves the neighbour around)
            extra_p += [pts[o] for o in order]
            extra_n += [nrm[o] for o in order]
    return np.vstack([p, extra_p]), np.vstack([nr, extra_n])


def plane(seed, n, tilt):
    rng = np.random.default_rng(seed)
    uv = rng.random((n, 2))
    a, b = tilt
    p = np.stack([uv[:, 0], uv[:, 1], a * uv[:, 0] + b * uv[:, 1]], 1)
    nrm = np.array([a, b, -1.0])
    nrm /= np.linalg.norm(nrm)
    return p, np.tile(nrm, (n, 1))


def main():
    check_numpy_orders()
    arrs, counts = {}, []
    p, nr = signed_zero_case()
    run_case(arrs, "signed_zero", p, nr, [(0.2, n) for n in (2, 3, 4, 5, 6, 8)], counts=counts)
    # the exact tilted plane of the issue, two more tilts; FPFH rows of 64 keypoints, SPFH rows of 160 points
    for t, (seed, npts, tilt) in enumerate(((5, 1500, (0.3, -0.2)), (6, 900, (-0.7, 0.45)), (7, 900, (0.05, 1.3)))):
        p, nr = plane(seed, npts, tilt)
        sel = np.random.default_rng(100 + t).choice(npts, 160, replace=False)
        run_case(arrs, f"plane_t{t}", p, nr, [(0.08, n) for n in (2, 3, 4, 5, 6, 8, 11)], kp=np.sort(sel[:64]),
                 spfh_sel=np.sort(sel), counts=counts)
    misses = 0
    for n in NS_EDGE:
        pr, miss = edge_pt_case(n, 0.06)
        misses += miss
        p, nr = pr.arrays()
        run_case(arrs, f"edge_pt_{n}", p, nr, [(0.06, n)], counts=counts)
        pr, miss = edge_a_case(n, 1.0)
        misses += miss
        p, nr = pr.arrays()
        run_case(arrs, f"edge_a_{n}", p, nr, [(1.0, n)], counts=counts)
    print(f"  edge pairs: {misses} exact targets not hit (their nearest value on the same side of the edge is kept)")
    for k, pr in enumerate(theta_cancel_case(0.1)):
        p, nr = pr.arrays()
        run_case(arrs, f"theta_cancel_{k}", p, nr, [(0.1, n) for n in (2, 4, 5, 8)], counts=counts)
    for n in (2, 3, 4, 5, 6, 8, 9, 11):
        for si, s in enumerate((1.0, float(np.float32(1.0000001)), ulps(1.0, [-2])[0])):
            pr, radii = reach_case(n, s)
            p, nr = pr.arrays()
            run_case(arrs, f"reach_{n}_{si}", p, nr, [(r, n) for r in radii], counts=counts)
    cases = sorted({k[: -len("_points")] for k in arrs if k.endswith("_points")})
    arrs["cases"] = np.array(cases)
    path = os.path.join(OUT, "spfh_edges.npz")
    np.savez_compressed(path, versions=VERSIONS, **arrs)
    print("contract != reference (rows / points that flip a bin):")
    for case, r, n, rows, nd, nf in counts:
        if nd or case.startswith("plane"):
            print(f"  {case} n={n}: {nd} of {rows} rows, {nf} points")
    print(f"spfh_edges.npz: {os.path.getsize(path) / 1024:.0f} KiB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
