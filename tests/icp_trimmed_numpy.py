"""Trimmed ICP (K18), stated in plain NumPy (float64).  What sf_select_kth (csrc/select.hip), sf_icp_accumulate_trimmed (k_icp_keys,
k_icp_sums, csrc/icp.hip) and shot_fpfh_amd.icp.icp_trimmed are held to -- not a test file, and the product does not import it.

One pass at (R, t) with the share `trim` in (0, 1]:
    n0    the pairs of tests/icp_robust_numpy.py, i.e. those with sqrt(d2) <= d_max (the gate first, and unchanged)
    r2    the mode's squared residual of each, `icp_robust_numpy.residual2`: d2, h h, or the Mahalanobis term clamped at 0
    rank  min(n0, max(1, ceil(trim n0)))
    cut   the rank-th smallest r2 by np.partition, in the order of the bit patterns with the sign cleared (mode 2's clamp can leave
          -0.0, which orders as zero; the cut itself is reported as +0.0)
    used  r2 <= cut: every tie at the cut is used, so the used set does not depend on the order of the pairs and may exceed rank
and the 48 sums of `icp_robust_numpy.terms` over the USED rows only -- weights, weighted centroids and all -- with
    [0] the used pairs   [37] n0   [38] rank   [47] cut
With trim == 1.0 there is no selection: every pair is used, [37] = [38] = [0] and [47] = 0.  Without a pair everything is zero.
"""
import math

import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

import gicp_numpy as G
import icp_numpy as I
import icp_robust_numpy as S

N_SUMS = S.N_SUMS
POINT, PLANE, GICP = S.POINT, S.PLANE, S.GICP
SLOT_N0, SLOT_RANK, SLOT_CUT = 37, 38, 47
UNUSED = {mode: [c for c in S.UNUSED[mode] if c not in (SLOT_N0, SLOT_RANK, SLOT_CUT)] for mode in (POINT, PLANE, GICP)}  # of no pass


# ---- the order statistic ----------------------------------------------------------------------------------------------------------------
def key_order(x):
    """the keys sf_select_kth orders by, as doubles np.partition orders the same way: the sign bit cleared (-0.0 -> 0.0, a negative
    value -> its magnitude, a NaN stays a NaN and sorts last)"""
    return np.abs(np.asarray(x, dtype=np.float64))


def select_kth(x, rank):
    """(value, keys that order below it, keys that order at or below it) of the rank-th smallest (1-based); for a rank inside the
    NaNs the value is a NaN and the counts are those of all the NaNs taken as one value"""
    k = key_order(x)
    v = float(np.partition(k, rank - 1)[rank - 1])
    if math.isnan(v):
        finite = int(np.count_nonzero(~np.isnan(k)))
        return v, finite, k.shape[0]
    return v, int(np.count_nonzero(k < v)), int(np.count_nonzero(k <= v))


def trim_rank(trim, n0):
    """min(n0, max(1, ceil(trim n0))), the product rounded as a double"""
    return min(n0, max(1, math.ceil(float(trim) * float(n0))))


def used_pairs(r2, trim):
    """(n0, rank, cut, used mask) of the squared residuals of the pairs inside d_max"""
    n0 = int(r2.shape[0])
    if n0 == 0:
        return 0, 0, 0.0, np.zeros(0, dtype=bool)
    if trim == 1.0:
        return n0, n0, 0.0, np.ones(n0, dtype=bool)
    rank = trim_rank(trim, n0)
    cut = select_kth(r2, rank)[0]
    return n0, rank, cut, r2 <= cut


# ---- one pass -----------------------------------------------------------------------------------------------------------------------------
def keys(mode, a, na, ref, nref, R, t, d_max, eps=1e-3, tree=None):
    """r2 of the pairs inside d_max, in row order"""
    return S.pass_a(mode, 0, 1.0, a, na, ref, nref, R, t, d_max, eps, tree)[1]


def terms(mode, loss, k, trim, a, na, ref, nref, R, t, d_max, eps=1e-3, means=None, tree=None, how="fsum"):
    """((used, 48) terms, their magnitudes, (n0, rank, cut)).  Mode 0 is centred with `means`; without them, with the weighted
    centroids of the USED pairs."""
    w, r2, _r2m, p, q = S.pass_a(mode, loss, k, a, na, ref, nref, R, t, d_max, eps, tree)
    n0, rank, cut, used = used_pairs(r2, trim)
    if mode == POINT and means is None:
        means = S.weighted_centroids(w[used], p[used], q[used], how)
    tm, mg = S.terms(mode, loss, k, a, na, ref, nref, R, t, d_max, eps, means if mode == POINT else None, tree, how)
    return tm[used], mg[used], (n0, rank, cut)


def sums(mode, loss, k, trim, a, na, ref, nref, R, t, d_max, eps=1e-3, means=None, tree=None, how="fsum"):
    """dict(vec: the 48 numbers with [37], [38], [47] filled in, abs: the sums of the magnitudes (zero in those three), count: the
    used pairs, n0, rank, cut)"""
    tm, mg, (n0, rank, cut) = terms(mode, loss, k, trim, a, na, ref, nref, R, t, d_max, eps, means, tree, how)
    vec, mag = I._sum(tm, how), mg.sum(axis=0)
    vec[[SLOT_N0, SLOT_RANK, SLOT_CUT]] = (n0, rank, cut)
    mag[[SLOT_N0, SLOT_RANK, SLOT_CUT]] = 0.0
    return dict(vec=vec, abs=mag, count=tm.shape[0], n0=n0, rank=rank, cut=cut)


# ---- the run --------------------------------------------------------------------------------------------------------------------------------
def trimmed_overlap(overlap, anneal_iterations, i):
    if anneal_iterations <= 0:
        return overlap
    return max(overlap, 1.0 - (1.0 - overlap) * i / anneal_iterations)


def refine(scan, na, ref, nref, mode, d_max, overlap, anneal_iterations=10, loss=0, scale=None, scale_start=None, division_factor=1.4,
           R=None, t=None, eps=1e-3, max_iter=50, rms_threshold=1e-2, step_tolerance=1e-9, how="fsum"):
    """The loop of `icp_robust_numpy.refine` over the share trimmed_overlap(overlap, anneal_iterations, i) of the pairs of iteration
    i: the rms is the mode's own over the USED pairs, and a small step stops the run only once the share is `overlap` (and the
    scale `scale`).  Without a loss the scale is 1 throughout and no weight looks at it.
    dict(R, t, rms, converged, iterations, rms_trace, steps, shares, scales, selections) with selections[i] = (n0, rank, used)."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    if loss == 0:
        scale = scale_start = 1.0
    scale_start = d_max if scale_start is None else scale_start
    tree = cKDTree(ref)
    trace, steps, shares, scales, selections, rms, converged = [], [], [], [], [], 0.0, False
    for i in range(max_iter):
        k = S.annealed_scale(scale, scale_start, division_factor, i)
        share = trimmed_overlap(overlap, anneal_iterations, i)
        tm, _mg, (n0, rank, _cut) = terms(mode, loss, k, share, scan, na, ref, nref, R, t, d_max, eps, None, tree, how)
        v = I._sum(tm, how)
        count = int(v[0])
        if count == 0:
            raise np.linalg.LinAlgError("no scan point has a reference point within d_max")
        if not v[7] > 0:
            raise np.linalg.LinAlgError(f"every pair has weight zero at the scale {k!r}")
        if mode == POINT:
            dR, dt = I.kabsch(v[8:17].reshape(3, 3), v[40:43] / v[7], v[43:46] / v[7])
            R2, t2 = I.compose(dR, dt, R, t)
            rms = float(np.sqrt(v[17]))
            step = max(float(np.abs(dR - np.eye(3)).max()), float(np.abs(dt).max()))
        elif mode == PLANE:
            _c, _sp, _sq, gtg, gth, abs_h = I.unpack(v[:40], mode)
            sol = np.linalg.solve(gtg, gth)
            R2, t2 = I.compose(Rotation.from_euler("xyz", sol[:3]).as_matrix(), sol[3:6], R, t)
            rms = abs_h / count
            step = float(np.abs(sol).max())
        else:
            _c, H, g, _rmr, rr = G.unpack(v[:40])
            xi = np.linalg.solve(H, g)
            dR = G.rodrigues(xi[:3])
            R2, t2 = dR @ R, dR @ t + xi[3:]
            rms = math.sqrt(rr / count)
            step = float(np.abs(xi).max())
        R, t = R2, t2
        trace.append(rms), steps.append(step), shares.append(share), scales.append(k), selections.append((n0, rank, count))
        small = k == scale and share == overlap and step < step_tolerance
        if rms < rms_threshold or small:
            converged = True
            break
    return dict(R=R, t=t, rms=rms, converged=converged, iterations=len(trace), rms_trace=trace, steps=steps, shares=shares,
                scales=scales, selections=selections)


# ---- the input sets ---------------------------------------------------------------------------------------------------------------------
OVERLAP, ANNEAL, ITERATIONS = 0.8, 10, S.ITERATIONS  # the table's: 375 of 1 875 scan points are clutter; linear over 10; 60 iterations
SELECT_SIZES = [1, 2, 63, 64, 65, 257, 65536, 65537, 200001]
SELECT_FAMILIES = ["random", "all_equal", "two_values", "seven_values", "low_bits", "exponents", "signed_zeros", "nans"]


def select_keys(family, n, seed=0):
    """n keys of a family (float64).  "low_bits": equal in their top 52 bits (sign cleared), random in the low 11 -- only the last
    digit passes tell them apart; "exponents": 0.0, 5e-324, 2^-1022, 1, 2^1023, +inf -- the first pass alone; "signed_zeros": -0.0
    among +0.0 and positives; "nans": one key in five a NaN (at least one key is not)."""
    rng = np.random.default_rng([seed, n, SELECT_FAMILIES.index(family)])
    if family == "random":
        return rng.random(n)
    if family == "all_equal":
        return np.full(n, 0.3125)
    if family == "two_values":
        return np.where(rng.random(n) < 0.4, 0.25, 0.75)
    if family == "seven_values":
        return rng.permutation(np.resize(np.array([0.0, 1e-300, 0.1, 0.1 + 2.0**-56, 1.0, 3.5, 1e300]), n))
    if family == "low_bits":
        base = np.float64(1.2345).view(np.uint64) & ~np.uint64(0x7FF)
        return (base | rng.integers(0, 2048, n, dtype=np.uint64)).view(np.float64)
    if family == "exponents":
        return rng.permutation(np.resize(np.array([0.0, 5e-324, 2.0**-1022, 1.0, 2.0**1023, np.inf]), n))
    if family == "signed_zeros":
        return rng.permutation(np.resize(np.array([-0.0, 0.0, -0.0, 0.5, 0.0, 2.0]), n))
    if family == "nans":
        x = rng.random(n)
        x[1::5] = np.nan
        return x
    raise ValueError(family)


def select_ranks(x):
    """the ranks a family is asked at: 1, 2, ceil(n / 2), n - 1, n and every tie boundary +- 1 (the first and last rank of every
    distinct value, at most 16 values, and their neighbours); with NaNs, ranks up to the count of the others only"""
    k = key_order(x)
    n = int(np.count_nonzero(~np.isnan(k)))
    ranks = {1, 2, (n + 1) // 2, n - 1, n}
    values, counts = np.unique(k[~np.isnan(k)], return_counts=True)
    if values.shape[0] <= 16:
        ends = np.cumsum(counts)
        for e in ends:
            ranks.update((int(e) - 1, int(e), int(e) + 1))
    return sorted(r for r in ranks if 1 <= r <= n)
