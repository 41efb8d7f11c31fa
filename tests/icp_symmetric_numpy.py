"""Symmetric point-to-plane ICP (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019), K19, stated in plain NumPy
(float64).  What sf_icp_accumulate_symmetric (k_icp_keys<3>, k_icp_sums<PASS, 3>, csrc/icp.hip) and shot_fpfh_amd.icp.icp_symmetric
are held to -- not a test file, and the product does not import it.

One pass at (R, t), for scan point a with normal na:
    p  = R a + t                                 ((R0 x + R1 y) + R2 z) + t per row, the order of k_transform
    b  = the nearest reference point (k = 1), nb its normal; the pair is kept iff sqrt(d2) <= d_max  (the gate first, and unchanged)
    m  = R na                                    (R0 x + R1 y) + R2 z per row, no t; m = na when R is None
    s  = +1 if (m0 nb0 + m1 nb1) + m2 nb2 >= 0 else -1       the sign of either normal cancels
    n  = 0.5 * (nb + s * m)                      per component: one addition; s * and 0.5 * are exact
    d  = b - p,  h = (dx nx + dy ny) + dz nz,  r2 = h h      the pair's squared residual (loss, trim)
    c  = p + b
    g  = [cy nz - cz ny, cz nx - cx nz, cx ny - cy nx, nx, ny, nz]
    w  = `icp_robust_numpy.weight(loss, r2, k)`;  used pairs: `icp_trimmed_numpy.used_pairs(r2, trim)`
The 48 terms of a used pair (the layout of sums[48]):
    [0] 1  [1..3] p  [4..6] b  [7] w  [8..28] w (g_a g_b) (a <= b, row by row)  [29..34] w (g_a h)  [35] |h|  [36] d2
    [40..42] w p  [43..45] w b  [46] w r2;  and of the pass [37] n0  [38] rank  [47] cut;  the rest zero.
Because of the factor 0.5, h is a length: for parallel unit normals it is point-to-plane's residual.  A zero normal row on one side
leaves n as half the other normal; zero rows on both sides give g = 0 and h = 0, and the pair is counted and fits nothing.

The host step from x = solve(sum w g g^T, sum w g h), a~ = x[:3], t~ = x[3:]:
    theta = atan |a~|,  e = a~ / |a~|,  R_h = exp([theta e]x)  (I when |a~| = 0),  dR = R_h R_h,
    l = (e0 t~0 + e1 t~1) + e2 t~2,  dt = R_h (cos theta t~ + ((1 - cos theta) l) e),   total <- (dR, dt) o total
the paper's rotate-translate-rotate step without its centring, with the translation's component ALONG the axis left unscaled.  The
linear system is exact for a rigid copy: b - p = a~ x (p + b) + t~ holds for b = C p + (I - [a~]x)^-1 t~ with C the Cayley rotation
by 2 atan|a~| about a~, and (I - [a~]x)^-1 t~ is R_h (cos theta t~) across the axis but t~ itself along it.  So on exact pairs this
step recovers the whole motion in one iteration, to rounding.  (The paper's R_h (cos theta t~), which drops the term
(1 - cos theta)(a . (p - b)) a of its linearisation, would leave the share 1 - cos theta of the component along the axis to the next
iteration; both steps have the same fixed points.)

Every per-pair expression is written out operation by operation, left to right, in the order the kernel forms it: NumPy rounds each
once (no fused multiply-add), as the library's -ffp-contract=off build does, so the pairs' terms are the same numbers on both sides
and what is left to differ is the order of the sums.
"""
import math

import numpy as np
from scipy.spatial import cKDTree

import gicp_numpy as G
import icp_numpy as I
import icp_robust_numpy as S
import icp_trimmed_numpy as T

N_SUMS = 48
TRIU = I.TRIU
SLOT_N0, SLOT_RANK, SLOT_CUT = T.SLOT_N0, T.SLOT_RANK, T.SLOT_CUT
UNUSED = [39]                    # of no pass ([37], [38], [47] belong to the selection)
WEIGHTED = slice(8, 35)          # the fit terms: times w
corner_set, clutter_set, knn_normals, rotation_error, true_motion = G.corner_set, S.clutter_set, G.knn_normals, G.rotation_error, G.true_motion


def mean_normal(nb, m):
    """n = 0.5 (nb + s m) per row, s the sign of (m0 nb0 + m1 nb1) + m2 nb2 with +1 at zero; and that dot product"""
    dot = (m[:, 0] * nb[:, 0] + m[:, 1] * nb[:, 1]) + m[:, 2] * nb[:, 2]
    s = np.where(dot >= 0.0, 1.0, -1.0)[:, None]
    return 0.5 * (nb + s * m), dot


def pairs(a, na, ref, nref, R, t, d_max, tree=None):
    """(p, b, n, d, d2, dot = m . nb) of the pairs inside d_max, in the scan's row order"""
    a, na = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(na, dtype=np.float64).reshape(-1, 3)
    p = G.move(R, t, a)
    if p.shape[0] == 0:
        return p, p, p, p, np.zeros(0), np.zeros(0)
    idx, d2 = G.nearest(p, ref, tree)
    with np.errstate(invalid="ignore"):
        keep = np.sqrt(d2) <= d_max
    p, idx, d2 = p[keep], idx[keep], d2[keep]
    m = na[keep] if R is None else G.rotate(R, na[keep])
    n, dot = mean_normal(np.asarray(nref, dtype=np.float64)[idx], m)
    return p, ref[idx], n, ref[idx] - p, d2, dot


def terms(loss, k, a, na, ref, nref, R, t, d_max, tree=None):
    """((n0, 48) terms of the pairs inside d_max, the (n0, 48) magnitudes of the products each term is made of, r2 (n0)): |term| for
    a single product, the sum of the products' magnitudes for h and d2.  The terms being the same numbers on both sides, this is
    what the rounding of the additions is relative to.  R = None is the identity, for the normals too."""
    p, b, n, d, d2, _dot = pairs(a, na, ref, nref, R, t, d_max, tree)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    x, y, z = b[:, 0], b[:, 1], b[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    h = (dx * nx + dy * ny) + dz * nz
    hm = (np.abs(dx * nx) + np.abs(dy * ny)) + np.abs(dz * nz)
    r2 = h * h
    w = S.weight(loss, r2, k)
    cx, cy, cz = px + x, py + y, pz + z
    g = [cy * nz - cz * ny, cz * nx - cx * nz, cx * ny - cy * nx, nx, ny, nz]
    one, zero = np.ones_like(px), np.zeros_like(px)
    cols = [one, px, py, pz, x, y, z, w]
    for i, j in TRIU:
        cols.append(w * (g[i] * g[j]))
    for i in range(6):
        cols.append(w * (g[i] * h))
    cols += [np.abs(h), d2, zero, zero, zero, w * px, w * py, w * pz, w * x, w * y, w * z, w * r2, zero]
    assert len(cols) == N_SUMS
    tm = np.stack(cols, axis=1)
    mg = np.abs(tm)
    mg[:, 35], mg[:, 46] = hm, w * (hm * hm)
    return tm, mg, r2


def sums(loss, k, trim, a, na, ref, nref, R, t, d_max, tree=None, how="fsum"):
    """dict(vec: the 48 numbers with [37], [38], [47] filled in, abs: the sums of the magnitudes (zero in those three), count: the
    used pairs, n0, rank, cut), the sums by math.fsum (how="np": NumPy's pairwise sum in row order)"""
    tm, mg, r2 = terms(loss, k, a, na, ref, nref, R, t, d_max, tree)
    n0, rank, cut, used = T.used_pairs(r2, trim)
    vec, mag = I._sum(tm[used], how), mg[used].sum(axis=0)
    vec[[SLOT_N0, SLOT_RANK, SLOT_CUT]] = (n0, rank, cut)
    mag[[SLOT_N0, SLOT_RANK, SLOT_CUT]] = 0.0
    return dict(vec=vec, abs=mag, count=int(np.count_nonzero(used)), n0=n0, rank=rank, cut=cut)


def unpack(v):
    """48 sums -> count, G^T W G (6, 6, symmetric), G^T W h (6), sum |h|, sum d2"""
    gtg = np.zeros((6, 6))
    for n, (i, j) in enumerate(TRIU):
        gtg[i, j] = gtg[j, i] = v[8 + n]
    return int(v[0]), gtg, np.array(v[29:35], dtype=np.float64), float(v[35]), float(v[36])


def step(x):
    """(dR, dt) of the solution x = [a~, t~]: theta = atan |a~|, e = a~ / |a~|, R_h the rotation by theta about e, dR = R_h R_h,
    dt = R_h (cos theta t~ + ((1 - cos theta)(e . t~)) e)"""
    x = np.asarray(x, dtype=np.float64)
    norm = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    if not norm > 0.0:
        return np.eye(3), x[3:6].copy()
    theta = math.atan(norm)
    half = G.rodrigues((theta / norm) * x[:3])
    e, c = x[:3] / norm, math.cos(theta)
    along = (e[0] * x[3] + e[1] * x[4]) + e[2] * x[5]
    return half @ half, half @ (c * x[3:6] + ((1.0 - c) * along) * e)


def refine(scan, na, ref, nref, d_max, loss=0, scale=None, scale_start=None, division_factor=1.4, overlap=1.0, anneal_iterations=10,
           R=None, t=None, max_iter=50, rms_threshold=1e-2, step_tolerance=1e-9, how="fsum"):
    """The loop of shot_fpfh_amd.icp.icp_symmetric: iteration i weights with `icp_robust_numpy.annealed_scale(.., i)` and fits the
    share `icp_trimmed_numpy.trimmed_overlap(.., i)` of its pairs; rms = sum |h| / count over the pairs used; it stops on
    rms < rms_threshold or, once scale and share have come down, on max|x| < step_tolerance.  Without a loss the scale is 1
    throughout.  dict(R, t, rms, converged, iterations, rms_trace, steps, shares, scales, counts)."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    if loss == 0:
        scale = scale_start = 1.0
    scale_start = d_max if scale_start is None else scale_start
    tree = cKDTree(ref)
    trace, steps, shares, scales, counts, rms, converged = [], [], [], [], [], 0.0, False
    for i in range(max_iter):
        k = S.annealed_scale(scale, scale_start, division_factor, i)
        share = T.trimmed_overlap(overlap, anneal_iterations, i)
        v = sums(loss, k, share, scan, na, ref, nref, R, t, d_max, tree, how)["vec"]
        count, gtg, gth, abs_h, _sq = unpack(v)
        if count == 0:
            raise np.linalg.LinAlgError("no scan point has a reference point within d_max")
        if not v[7] > 0:
            raise np.linalg.LinAlgError(f"every pair has weight zero at the scale {k!r}")
        x = np.linalg.solve(gtg, gth)
        dR, dt = step(x)
        R, t = I.compose(dR, dt, R, t)
        rms = abs_h / count
        trace.append(rms), steps.append(float(np.abs(x).max())), shares.append(share), scales.append(k), counts.append(count)
        small = k == scale and share == overlap and steps[-1] < step_tolerance
        if rms < rms_threshold or small:
            converged = True
            break
    return dict(R=R, t=t, rms=rms, converged=converged, iterations=len(trace), rms_trace=trace, steps=steps, shares=shares,
                scales=scales, counts=counts)


# ---- the curved patch of the parity table ------------------------------------------------------------------------------------------
def curved_surface(n, rng, sigma):
    """n points on the patch z = 0.12 sin(5 x) cos(4 y) + 0.5 x^2 - 0.3 y^2, (x, y) uniform in [-0.5, 0.5] x [-0.4, 0.4], plus
    isotropic noise: curved everywhere, and bumpy enough that no motion slides along it (a plain quadric patch of this size
    leaves every mode 2e-2 off at sigma = 0.002)"""
    x, y = rng.random(n) - 0.5, 0.8 * (rng.random(n) - 0.5)
    z = 0.12 * np.sin(5.0 * x) * np.cos(4.0 * y) + 0.5 * x * x - 0.3 * y * y
    return np.stack([x, y, z], axis=1) + sigma * rng.standard_normal((n, 3))


def curved_set(seed, n=1500, sigma=0.002):
    """(scan, ref, R0, t0) as `gicp_numpy.corner_set`: two independent samplings of the curved patch, 0.12 rad apart"""
    rng = np.random.default_rng(1000 + seed)
    ref = curved_surface(n, rng, sigma)
    world = curved_surface(n, rng, sigma)
    R0, t0 = G.true_motion()
    return (world - t0) @ R0, ref, R0, t0
