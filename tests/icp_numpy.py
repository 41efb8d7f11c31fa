"""One pass of point-to-point and point-to-plane ICP, stated in plain NumPy (float64).  What sf_icp_accumulate (k_icp_sums<1, 0>,
k_icp_sums<1, 1>, csrc/icp.hip) and the loop of shot_fpfh_amd.icp._refine are held to -- not a test file, and the product does not
import it.

One pass at (R, t), for scan point a:
    p = R a + t                                  ((R0 x + R1 y) + R2 z) + t per row, the order of k_transform; R = None leaves a alone
    q = the nearest reference point (k = 1), n its normal as stored (NOT normalised); d = q - p, d2 = (dx dx + dy dy) + dz dz
    the pair is kept iff sqrt(d2) <= d_max       (false for a NaN or negative d_max)
    pass A (both modes)   [0] 1  [1..3] p  [4..6] q
    mode 0 (point)        a = p - pm, b = q - qm with (pm, qm) the centroids GIVEN (`means`): [8..16] a_i b_j row-major, [17] d2
    mode 1 (plane)        g = [py nz - pz ny, pz nx - px nz, px ny - py nx, nx, ny, nz], h = (dx nx + dy ny) + dz nz:
                          [8..28] g_a g_b (a <= b, row by row), [29..34] g_a h, [35] |h|
    every other slot is zero: [7], [18..39] in mode 0, [36..39] in mode 1
and the sums over the kept pairs.  The device centres mode 0 with the centroids IT formed (k_icp_means: with every weight 1.0, as in
this call, sum / count in float64 from its own pass A sums), which come back in the first seven numbers; handed to `terms` as means = raw[1:7] / raw[0] -- the same
IEEE division -- every term is the same number on both sides.  Without `means` the centroids are the math.fsum ones, rounded once.

Every expression is written out operation by operation, left to right, as the kernel forms it: NumPy rounds each once (no fused
multiply-add), as the library's -ffp-contract=off build does, so what is left to differ is the order of the additions.
"""
import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

from gicp_numpy import fsum_cols, move, nearest

N_SUMS = 40
POINT, PLANE = 0, 1
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]
UNUSED = {POINT: [7] + list(range(18, 40)), PLANE: list(range(36, 40))}  # the slots that belong to no pass


def kept_pairs(a, ref, R, t, d_max, tree=None):
    """(p, idx, d, d2) of the kept pairs, in the scan's row order"""
    p = move(R, t, np.asarray(a, dtype=np.float64).reshape(-1, 3))
    if p.shape[0] == 0:
        return p, np.zeros(0, dtype=np.int64), p, np.zeros(0)
    idx, d2 = nearest(p, ref, tree)
    with np.errstate(invalid="ignore"):
        keep = np.sqrt(d2) <= d_max
    p, idx = p[keep], idx[keep]
    return p, idx, ref[idx] - p, d2[keep]


def centroids(p, q):
    """the six means of pass A by math.fsum, rounded once (what `terms` centres with when it is given none)"""
    if p.shape[0] == 0:
        return np.zeros(6)
    return fsum_cols(np.hstack([p, q])) / float(p.shape[0])


def terms(a, ref, nref, R, t, d_max, mode, means=None, tree=None):
    """(k, 40) terms of one pass over the kept pairs in the layout of sums[40], and the (k, 40) magnitudes of the products each term
    is made of: |term| for a single product, the sum of the products' magnitudes for h (|h|'s slot) and d2.  The terms being the
    same numbers on both sides, this is what the rounding of the additions is relative to."""
    p, idx, d, d2 = kept_pairs(a, ref, R, t, d_max, tree)
    q = ref[idx]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    one, zero = np.ones_like(px), np.zeros_like(px)
    cols = [one, px, py, pz, x, y, z, zero]
    mags = [one, np.abs(px), np.abs(py), np.abs(pz), np.abs(x), np.abs(y), np.abs(z), zero]
    if mode == POINT:
        pm = centroids(p, q) if means is None else np.asarray(means, dtype=np.float64)
        av = [px - pm[0], py - pm[1], pz - pm[2]]
        bv = [x - pm[3], y - pm[4], z - pm[5]]
        for i in range(3):
            for j in range(3):
                cols.append(av[i] * bv[j])
                mags.append(np.abs(av[i] * bv[j]))
        cols.append(d2)
        mags.append(d2)
    elif mode == PLANE:
        n = np.asarray(nref, dtype=np.float64)[idx]
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        g = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
        h = (dx * nx + dy * ny) + dz * nz
        hm = (np.abs(dx * nx) + np.abs(dy * ny)) + np.abs(dz * nz)
        for i, j in TRIU:
            cols.append(g[i] * g[j])
            mags.append(np.abs(g[i] * g[j]))
        for i in range(6):
            cols.append(g[i] * h)
            mags.append(np.abs(g[i] * h))
        cols.append(np.abs(h))
        mags.append(hm)
    else:
        raise ValueError(f"mode {mode}")
    cols += [zero] * (N_SUMS - len(cols))
    mags += [zero] * (N_SUMS - len(mags))
    return np.stack(cols, axis=1), np.stack(mags, axis=1)


def _sum(x, how):
    if how == "fsum":
        return fsum_cols(x) if x.shape[0] else np.zeros(x.shape[1])
    return np.sum(x, axis=0)  # "np": NumPy's pairwise sum in row order


def sums(a, ref, nref, R, t, d_max, mode, means=None, tree=None):
    """The 40 sums by math.fsum and the 40 sums of the magnitudes."""
    tm, mg = terms(a, ref, nref, R, t, d_max, mode, means, tree)
    return dict(vec=_sum(tm, "fsum"), abs=mg.sum(axis=0), count=tm.shape[0])


def device_means(raw):
    """the centroids k_icp_means leaves for pass B when every weight is 1.0, from the numbers the call returns: sum / count, zero without a pair"""
    raw = np.asarray(raw, dtype=np.float64)
    return raw[1:7] / raw[0] if raw[0] > 0 else np.zeros(6)


def unpack(v, mode):
    """40 sums -> what the host step reads: (count, sum p, sum q, cross-covariance (3, 3), sum d2) in mode 0,
    (count, sum p, sum q, G^T G (6, 6, symmetric), G^T h (6), sum |h|) in mode 1"""
    v = np.asarray(v, dtype=np.float64)
    if mode == POINT:
        return int(v[0]), v[1:4], v[4:7], v[8:17].reshape(3, 3), float(v[17])
    gtg = np.zeros((6, 6))
    for n, (i, j) in enumerate(TRIU):
        gtg[i, j] = gtg[j, i] = v[8 + n]
    return int(v[0]), v[1:4], v[4:7], gtg, np.array(v[29:35]), float(v[35])


def kabsch(cross_cov, pbar, qbar):
    """solver_point_to_point from its sums: the SVD and the reflection rule of kabsch_from_covariance"""
    u, _s, vt = np.linalg.svd(cross_cov)
    rot = vt.T @ u.T
    if np.linalg.det(rot) < 0:
        ut = u.T.copy()
        ut[-1] *= -1
        rot = vt.T @ ut
    return rot, qbar - rot.dot(pbar)


def compose(dR, dt, R, t):
    """(dR, dt) o (R, t) as RigidTransform.__matmul__ forms it: the product, then the rotation through a unit quaternion"""
    R2, t2 = dR @ R, dR @ t + dt
    quat = Rotation.from_matrix(R2).as_quat()
    return Rotation.from_quat(quat / np.linalg.norm(quat)).as_matrix(), t2


def refine(scan, ref, nref, mode, d_max, R=None, t=None, max_iter=50, rms_threshold=1e-2, how="fsum"):
    """The loop of shot_fpfh_amd.icp._refine for modes 0 and 1: the scan stays where it is, the running transform moves; the
    residual is the one of the pairs the step was fitted ON (before the update); stop on rms < rms_threshold.
    dict(R, t, rms, converged, iterations, rms_trace, counts).  how="np" sums with NumPy's pairwise sum in row order: on a
    row-permuted scan that is the statement's sensitivity to the order of its sums."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    tree = cKDTree(ref)
    trace, counts, rms = [], [], 0.0
    for _ in range(max_iter):
        if mode == POINT:
            # centroids first, by the same kind of sum, then the centred pass: the two passes of the device
            p, idx, _d, _d2 = kept_pairs(scan, ref, R, t, d_max, tree)
            if p.shape[0] == 0:
                raise np.linalg.LinAlgError("no scan point has a reference point within d_max")
            tm, _mg = terms(scan, ref, nref, R, t, d_max, mode, _sum(np.hstack([p, ref[idx]]), how) / float(p.shape[0]), tree)
            count, sp, sq, cov, sq_dist = unpack(_sum(tm, how), mode)
            dR, dt = kabsch(cov, sp / count, sq / count)
            rms = float(np.sqrt(sq_dist))
        else:
            tm, _mg = terms(scan, ref, nref, R, t, d_max, mode, None, tree)
            count, sp, sq, gtg, gth, abs_h = unpack(_sum(tm, how), mode)
            if count == 0:
                raise np.linalg.LinAlgError("no scan point has a reference point within d_max")
            sol = np.linalg.solve(gtg, gth)
            dR, dt = Rotation.from_euler("xyz", sol[:3]).as_matrix(), sol[3:6]
            rms = abs_h / count
        R, t = compose(dR, dt, R, t)
        trace.append(rms)
        counts.append(count)
        if rms < rms_threshold:
            break
    return dict(R=R, t=t, rms=rms, converged=rms < rms_threshold, iterations=len(trace), rms_trace=trace, counts=counts)
