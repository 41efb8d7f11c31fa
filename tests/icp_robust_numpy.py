"""ICP with a robust loss (K17), stated in plain NumPy (float64).  What sf_icp_accumulate_robust (k_icp_sums, k_icp_means,
csrc/icp.hip) and shot_fpfh_amd.icp.icp_robust are held to -- not a test file, and the product does not import it.

One pass at (R, t) with the loss's scale k keeps the pairs of tests/icp_numpy.py / tests/gicp_numpy.py (the `d_max` gate first, and
unchanged) and gives each kept pair a weight w = psi(r) / r from its squared residual r2:
    mode 0 (point)        r2 = d2
    mode 1 (plane)        r2 = h h
    mode 2 (generalized)  r2 = the Mahalanobis term (r0 u0 + r1 u1) + r2 u2, clamped at 0
    none            w = 1
    Huber           a = sqrt(r2);  w = 1 if a <= k else k / a
    Cauchy          s = r2 / (k k);  w = 1 / (1 + s)
    Geman-McClure   c = 1 / (1 + s);  w = c c
    Tukey           w = (1 - s)(1 - s) if s <= 1 else 0
every operation rounded once, left to right, as the kernel forms it.  The 48 terms of a pair (the layout of sums[48]):
    [0] 1  [1..3] p  [4..6] q                     unweighted
    [7] w
    [8..36] the mode's terms of `icp_numpy.terms` / `gicp_numpy.terms`, the fit terms times w (one more rounding): [8..16] in mode 0,
            centred with the WEIGHTED centroids given (`means`); [8..34] in modes 1 and 2.  The residual slots stay as they are:
            [17] d2 (mode 0), [35] |h| (mode 1) or the Mahalanobis term (mode 2), [36] d2 (mode 2)
    [40..42] w p  [43..45] w q  [46] w r2  [47] 0
The device centres mode 0 with the weighted centroids IT formed (k_icp_means: sum w p / sum w in float64), which come back in
[40..45] and [7]; handed to `terms` as means = `device_means(raw)` -- the same IEEE division -- every term is the same number on
both sides and what is left to differ is the order of the additions.
"""
import math

import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

import gicp_numpy as G
import icp_numpy as I

N_SUMS = 48
POINT, PLANE, GICP = 0, 1, 2
MODES = {"point_to_point": POINT, "point_to_plane": PLANE, "generalized": GICP}
LOSSES = {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3, "tukey": 4}
WEIGHTED = {POINT: slice(8, 17), PLANE: slice(8, 35), GICP: slice(8, 35)}  # the fit terms: times w
UNUSED = {POINT: list(range(18, 40)) + [47], PLANE: list(range(36, 40)) + [47], GICP: list(range(37, 40)) + [47]}  # of no pass


def weight(loss, r2, k):
    """w of every squared residual in r2 at the scale k, operation by operation as robust_weight of csrc/icp.hip"""
    r2 = np.asarray(r2, dtype=np.float64)
    k = float(k)
    if loss == 0:
        return np.ones_like(r2)
    if loss == 1:
        a = np.sqrt(r2)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(a <= k, 1.0, k / a)
    kk = k * k
    s = r2 / kk
    if loss == 4:
        o = 1.0 - s
        return np.where(s <= 1.0, o * o, 0.0)
    c = 1.0 / (1.0 + s)
    return c if loss == 2 else c * c


def rho(loss, r2, k):
    """the loss itself, rho(r) with rho' = psi = w r (for the finite-difference check of the gradient; not what the device forms);
    none: r^2 / 2"""
    r2 = np.asarray(r2, dtype=np.float64)
    kk = float(k) * float(k)
    if loss == 0:
        return 0.5 * r2
    if loss == 1:
        a = np.sqrt(r2)
        return np.where(a <= k, 0.5 * r2, k * a - 0.5 * kk)
    if loss == 2:
        return 0.5 * kk * np.log1p(r2 / kk)
    if loss == 3:
        return 0.5 * r2 / (1.0 + r2 / kk)
    s = np.minimum(r2 / kk, 1.0)
    return kk / 6.0 * (1.0 - (1.0 - s) ** 3)


def base_terms(mode, a, na, ref, nref, R, t, d_max, eps=1e-3, means=None, tree=None):
    """the (n, 40) terms and magnitudes of the mode WITHOUT a loss: icp_numpy.terms or gicp_numpy.terms"""
    if mode == GICP:
        return G.terms(a, na, ref, nref, R, t, d_max, eps, tree)
    return I.terms(a, ref, nref, R, t, d_max, mode, means, tree)


def residual2(mode, tm, mg):
    """(r2, its magnitude) per pair from the mode's unweighted terms"""
    if mode == POINT:
        return tm[:, 17], mg[:, 17]
    if mode == PLANE:
        return tm[:, 35] * tm[:, 35], mg[:, 35] * mg[:, 35]  # |h| |h| is h h
    maha = tm[:, 35]
    return np.where(maha < 0.0, 0.0, maha), mg[:, 35]


def pass_a(mode, loss, k, a, na, ref, nref, R, t, d_max, eps=1e-3, tree=None):
    """(w, r2, r2's magnitude, p (n, 3), q (n, 3)) of the kept pairs: what pass A sums"""
    tm, mg = base_terms(mode, a, na, ref, nref, R, t, d_max, eps, np.zeros(6), tree)
    r2, r2m = residual2(mode, tm, mg)
    return weight(loss, r2, k), r2, r2m, tm[:, 1:4], tm[:, 4:7]


def weighted_centroids(w, p, q, how="fsum"):
    """sum w p / sum w, sum w q / sum w (6), zeros when sum w is not positive; by math.fsum, rounded once, or NumPy's sum"""
    cols = np.hstack([w[:, None], w[:, None] * p, w[:, None] * q])
    s = I._sum(cols, how)
    return s[1:7] / s[0] if s[0] > 0 else np.zeros(6)


def terms(mode, loss, k, a, na, ref, nref, R, t, d_max, eps=1e-3, means=None, tree=None, how="fsum"):
    """(n, 48) terms of one pass over the kept pairs and the (n, 48) magnitudes their roundings are relative to.  Mode 0 is centred
    with `means` (the six weighted centroids); without them, with the statement's own."""
    w, r2, r2m, p, q = pass_a(mode, loss, k, a, na, ref, nref, R, t, d_max, eps, tree)
    if mode == POINT and means is None:
        means = weighted_centroids(w, p, q, how)
    tm40, mg40 = base_terms(mode, a, na, ref, nref, R, t, d_max, eps, means, tree)
    n = tm40.shape[0]
    tm, mg = np.zeros((n, N_SUMS)), np.zeros((n, N_SUMS))
    tm[:, :40], mg[:, :40] = tm40, mg40
    cols = WEIGHTED[mode]
    tm[:, cols] = w[:, None] * tm40[:, cols]
    mg[:, cols] = w[:, None] * mg40[:, cols]
    tm[:, 7] = mg[:, 7] = w
    tm[:, 40:43], tm[:, 43:46] = w[:, None] * p, w[:, None] * q
    mg[:, 40:46] = np.abs(tm[:, 40:46])
    tm[:, 46], mg[:, 46] = w * r2, w * r2m
    return tm, mg


def sums(mode, loss, k, a, na, ref, nref, R, t, d_max, eps=1e-3, means=None, tree=None):
    """The 48 sums by math.fsum and the 48 sums of the magnitudes."""
    tm, mg = terms(mode, loss, k, a, na, ref, nref, R, t, d_max, eps, means, tree)
    return dict(vec=I._sum(tm, "fsum"), abs=mg.sum(axis=0), count=tm.shape[0])


def device_means(raw):
    """the weighted centroids k_icp_means leaves for pass B, from the numbers the call returns"""
    raw = np.asarray(raw, dtype=np.float64)
    return raw[40:46] / raw[7] if raw[7] > 0 else np.zeros(6)


def annealed_scale(scale, scale_start, division_factor, i):
    return max(scale, scale_start / division_factor**i)


def refine(scan, na, ref, nref, mode, loss, d_max, scale, scale_start=None, division_factor=1.4, R=None, t=None, eps=1e-3,
           max_iter=50, rms_threshold=1e-2, step_tolerance=1e-9, how="fsum"):
    """The loop of shot_fpfh_amd.icp._refine_robust: iteration i weights with the scale max(scale, scale_start / division_factor**i)
    (scale_start = d_max unless given), fits -- weighted Kabsch (mode 0), the linearised plane step (mode 1), the Gauss-Newton step
    with the exact exponential (mode 2) -- composes as the mode's statement does, and reports the mode's UNWEIGHTED residual of the
    pairs the step was fitted on.  It stops on rms < rms_threshold or, once the scale is `scale`, on a step below step_tolerance:
    max|xi| (modes 1, 2), max(|dR - I|, |dt|) (mode 0).  dict(R, t, rms, converged, iterations, rms_trace, steps, scales, counts).
    how="np" sums with NumPy's pairwise sum in row order."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    scale_start = d_max if scale_start is None else scale_start
    tree = cKDTree(ref)
    trace, steps, scales, counts, rms, converged = [], [], [], [], 0.0, False
    for i in range(max_iter):
        k = annealed_scale(scale, scale_start, division_factor, i)
        tm, _mg = terms(mode, loss, k, scan, na, ref, nref, R, t, d_max, eps, None, tree, how)
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
        trace.append(rms), steps.append(step), scales.append(k), counts.append(count)
        small = k == scale and step < step_tolerance
        if rms < rms_threshold or small:
            converged = True
            break
    return dict(R=R, t=t, rms=rms, converged=converged, iterations=len(trace), rms_trace=trace, steps=steps, scales=scales, counts=counts)


# ---- the set of the accuracy table -------------------------------------------------------------------------------------------------
CLUTTER = 375
D_MAX, SCALE, SCALE_TUKEY, FACTOR, ITERATIONS = 0.15, 0.006, 0.012, 1.4, 60  # 3 sigma of the noise; Tukey's cut-off twice that


def clutter_set(seed):
    """(scan, ref, R0, t0): `gicp_numpy.corner_set(seed)` (1 500 + 1 500 points, sigma = 0.002, 0.12 rad from the identity) with the
    scan extended by 375 points (25 %) the reference does not have: a patch hovering 0.04 above the z = 0 face, well inside
    d_max = 0.15."""
    scan, ref, R0, t0 = G.corner_set(seed)
    rng = np.random.default_rng(100 + seed)
    c = np.stack([0.2 + 0.4 * rng.random(CLUTTER), 0.2 + 0.4 * rng.random(CLUTTER), 0.04 + 0.002 * rng.standard_normal(CLUTTER)], 1)
    return np.vstack([scan, (c - t0) @ R0]), ref, R0, t0


def table_scales(mode, loss, eps=1e-3):
    """(scale, scale_start) of the table for a mode and a loss (names or numbers).  Modes 0 and 1 measure a length.  Mode 2's residual
    is the Mahalanobis distance, in which an offset h across two parallel surfaces counts as h / sqrt(2 eps) (M = 1 / (2 eps) along
    the common normal), so both scales are divided by sqrt(2 eps) there."""
    scale = SCALE_TUKEY if loss in ("tukey", LOSSES["tukey"]) else SCALE
    unit = math.sqrt(2.0 * eps) if mode in ("generalized", GICP) else 1.0
    return scale / unit, D_MAX / unit
