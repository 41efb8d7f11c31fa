"""Fast global registration (Zhou, Park, Koltun, ECCV 2016) over given matches, stated in plain NumPy (float64): a scaled
Geman-McClure cost minimised by graduated non-convexity, a fixed number of weighted Gauss-Newton steps on SE(3).  What
shot_fpfh_amd.matching.fast_global_registration and the K12 kernels (csrc/fgr.hip) are held to -- not a test file.

Every per-row expression is written out operation by operation, left to right, in the order the kernel forms it: NumPy rounds each
of them once (no fused multiply-add), as the library's -ffp-contract=off build does, so the rows' terms are the same numbers on
both sides and what is left to differ is the order of the sums, the 6 x 6 solve and sin / cos.
"""
import math

import numpy as np

from ransac_numpy import matched_points, synthetic_matches  # noqa: F401 -- re-exported for the tests
from shot_fpfh_amd.matching.ransac import draw_stream

N_TERMS = 29           # 21 of A's upper triangle (row by row), 6 of g, E, W
PIVOT_TOL = 1e-12      # an LDL^T pivot d_j <= PIVOT_TOL * A_jj is "not positive": rounding leaves ~2^-52 A_jj where the exact pivot is 0
STATUS_OK, STATUS_DEGENERATE, STATUS_NO_EXTENT = 0, 1, 2
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]


def fsum_cols(x):
    return np.array([math.fsum(col.tolist()) for col in np.atleast_2d(x).T])


def _sum(x, how, order=None):
    if how == "fsum":
        return fsum_cols(x)
    return np.sum(x if order is None else x[order], axis=0)  # "np": NumPy's pairwise sum over a permuted row order


def normalise(a, b, how="fsum", order=None):
    """ca, cb, s and the normalised rows x, y."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    k = a.shape[0]
    if k < 3 or b.shape[0] != k:
        raise ValueError(f"{k} rows: at least 3 matched pairs are needed")
    ca, cb = _sum(a, how, order) / k, _sum(b, how, order) / k
    da, db = a - ca, b - cb
    d2a = (da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2]
    d2b = (db[:, 0] * db[:, 0] + db[:, 1] * db[:, 1]) + db[:, 2] * db[:, 2]
    s = math.sqrt(max(float(d2a.max()), float(d2b.max())))
    if not (s > 0.0 and math.isfinite(s)):
        raise ValueError("the matched points have no extent (or are not finite)")
    return ca, cb, s, da / s, db / s


def terms(x, y, R, t, mu):
    """(k, 29) terms of one pass and the (k, 29) sums of the magnitudes of the products each term is made of.

    p = R x + t, r = p - y, l = mu / (mu + r.r), w = l^2, J = [-[p]x | I]:
      A = sum w J^T J = sum w [[(p.p) I - p p^T, [p]x], [-[p]x, I]],  g = sum w J^T r = sum w [p x r; r],
      E = sum (w r.r + mu (l - 1)^2),  W = sum w.
    A cross product's component is TWO products of opposite sign: its magnitude column adds the two magnitudes (what the
    rounding of the difference is relative to)."""
    R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    p0 = ((R[0, 0] * x0 + R[0, 1] * x1) + R[0, 2] * x2) + t[0]
    p1 = ((R[1, 0] * x0 + R[1, 1] * x1) + R[1, 2] * x2) + t[1]
    p2 = ((R[2, 0] * x0 + R[2, 1] * x1) + R[2, 2] * x2) + t[2]
    r0, r1, r2 = p0 - y[:, 0], p1 - y[:, 1], p2 - y[:, 2]
    rr = (r0 * r0 + r1 * r1) + r2 * r2
    l = mu / (mu + rr)
    w = l * l
    wp0, wp1, wp2 = w * p0, w * p1, w * p2
    wr0, wr1, wr2 = w * r0, w * r1, w * r2
    lm = l - 1.0
    z = np.zeros_like(w)
    cols = [
        w * (p1 * p1 + p2 * p2), -(wp0 * p1), -(wp0 * p2), z, -wp2, wp1,  # A row 0
        w * (p0 * p0 + p2 * p2), -(wp1 * p2), wp2, z, -wp0,               # A row 1
        w * (p0 * p0 + p1 * p1), -wp1, wp0, z,                            # A row 2
        w, z, z, w, z, w,                                                 # A rows 3 .. 5
        p1 * wr2 - p2 * wr1, p2 * wr0 - p0 * wr2, p0 * wr1 - p1 * wr0,    # g: p x (w r)
        wr0, wr1, wr2,                                                    # g: w r
        w * rr + mu * (lm * lm),                                          # E
        w,                                                                # W
    ]
    mags = [np.abs(c) for c in cols]
    mags[21] = np.abs(p1 * wr2) + np.abs(p2 * wr1)
    mags[22] = np.abs(p2 * wr0) + np.abs(p0 * wr2)
    mags[23] = np.abs(p0 * wr1) + np.abs(p1 * wr0)
    return np.stack(cols, axis=1), np.stack(mags, axis=1)


def unpack(v):
    """29 sums -> A (6, 6, symmetric), g (6), E, W"""
    A = np.zeros((6, 6))
    for n, (i, j) in enumerate(TRIU):
        A[i, j] = A[j, i] = v[n]
    return A, np.array(v[21:27], dtype=np.float64), float(v[27]), float(v[28])


def sums(x, y, R, t, mu):
    """A, g, E, W by math.fsum, the 29 sums as a vector, and the 29 sums of the magnitudes."""
    tm, mg = terms(x, y, R, t, mu)
    v = fsum_cols(tm)
    A, g, E, W = unpack(v)
    return dict(A=A, g=g, E=E, W=W, vec=v, abs=mg.sum(axis=0))


def solve_ldlt(A, g):
    """xi of A xi = -g by LDL^T without pivoting; None when a pivot is not positive (PIVOT_TOL) or not finite."""
    n = 6
    L, d = np.eye(n), np.zeros(n)
    for j in range(n):
        dj = A[j, j]
        for q in range(j):
            dj = dj - (L[j, q] * L[j, q]) * d[q]
        if not (dj > PIVOT_TOL * A[j, j]) or not math.isfinite(dj):
            return None
        d[j] = dj
        for i in range(j + 1, n):
            v = A[i, j]
            for q in range(j):
                v = v - (L[i, q] * L[j, q]) * d[q]
            L[i, j] = v / dj
    z = np.zeros(n)
    for i in range(n):
        v = -g[i]
        for q in range(i):
            v = v - L[i, q] * z[q]
        z[i] = v
    xi = np.zeros(n)
    for i in reversed(range(n)):
        v = z[i] / d[i]
        for q in range(i + 1, n):
            v = v - L[q, i] * xi[q]
        xi[i] = v
    return xi if np.isfinite(xi).all() else None


def rodrigues(om):
    """exp([om]x) = I + (sin th / th) K + 1/2 (sin(th/2) / (th/2))^2 K^2, K = [om]x, th = |om|; I when th is 0."""
    th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    th = math.sqrt(th2)
    if not th > 0.0:
        return np.eye(3)
    ca = math.sin(th) / th
    h = math.sin(0.5 * th) / (0.5 * th)
    cb = 0.5 * (h * h)
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    return np.eye(3) + ca * K + cb * (K @ K)


def fgr_rows(a, b, distance_threshold, iterations=64, division_factor=1.4, decrease_every=4, how="fsum", order=None):
    """Steps 1-4 of the definition on the rows given.  Returns dict(R, t (denormalised), status, iterations, mu, s, E, W,
    trace (iterations x 4: mu, E, W, |xi| -- zero rows after a degenerate stop))."""
    if iterations < 1 or decrease_every < 1 or not division_factor > 1 or not math.isfinite(distance_threshold):
        raise ValueError("iterations >= 1, decrease_every >= 1, division_factor > 1 and a finite threshold are needed")
    ca, cb, s, x, y = normalise(a, b, how, order)
    R, t, mu = np.eye(3), np.zeros(3), 1.0
    mu_floor = (distance_threshold / s) * (distance_threshold / s)
    trace = np.zeros((iterations, 4))
    status, done, E, W = STATUS_OK, 0, 0.0, 0.0
    for it in range(iterations):
        tm, _ = terms(x, y, R, t, mu)
        A, g, E, W = unpack(_sum(tm, how, order))
        xi = solve_ldlt(A, g)
        if xi is None:
            status = STATUS_DEGENERATE
            break
        dR = rodrigues(xi[:3])
        R, t = dR @ R, dR @ t + xi[3:]
        trace[it] = mu, E, W, math.sqrt(float(np.dot(xi, xi)))
        done = it + 1
        if done % decrease_every == 0:
            mu = max(mu / division_factor, mu_floor)
    t_out = (s * t + cb) - R @ ca
    return dict(R=R, t=t_out, status=status, iterations=done, mu=mu, s=s, E=E, W=W, trace=trace)


def tuple_selection(a, b, tuple_count, tuple_scale=0.95, seed=72):
    """The paper's tuple test from K11's pieces: triples drawn by draw_stream, kept when every pair of edges agrees within
    tuple_scale; the match ids of the first tuple_count survivors, in draw order, duplicates kept."""
    from ransac_numpy import hypotheses

    m = a.shape[0]
    draws = draw_stream(np.random.default_rng(seed), m, 3, 100 * tuple_count)
    status = hypotheses(a, b, draws, tuple_scale)[0]
    keep = np.flatnonzero(status == 0)[:tuple_count]
    if keep.size < 1:
        raise ValueError("no triple of matches passed the tuple test")
    return draws[keep].reshape(-1).astype(np.int64)


def inlier_count(a, b, R, t, thr):
    return int(np.count_nonzero(np.linalg.norm(a.dot(R.T) + t - b, axis=1) <= thr))


def fast_global_registration(scan_idx, ref_idx, scan_kp, ref_kp, distance_threshold, iterations=64, division_factor=1.4,
                             decrease_every=4, tuple_count=0, tuple_scale=0.95, seed=72, how="fsum", order=None):
    """(inlier ratio over ALL matches, R, t, record dict) -- R not re-normalised."""
    a, b = matched_points(scan_idx, ref_idx, scan_kp, ref_kp)
    sel = tuple_selection(a, b, tuple_count, tuple_scale, seed) if tuple_count > 0 else None
    rows_a, rows_b = (a, b) if sel is None else (a[sel], b[sel])
    out = fgr_rows(rows_a, rows_b, distance_threshold, iterations, division_factor, decrease_every, how, order)
    if out["status"] != STATUS_OK:
        raise ValueError("degenerate: the weighted matched points do not determine a rigid motion")
    inl = inlier_count(a, b, out["R"], out["t"], distance_threshold)
    out.update(rows=rows_a.shape[0], inliers=inl, sel=sel)
    return inl / a.shape[0], out["R"], out["t"], out
