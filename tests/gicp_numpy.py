"""Generalized (plane-to-plane) ICP (Segal, Haehnel, Thrun, RSS 2009), stated in plain NumPy (float64).  What
shot_fpfh_amd.icp.icp_generalized and K16 (k_icp_sums<1, 2>, csrc/icp.hip) are held to -- not a test file, and the product does not
import it.

A point with unit normal n has the covariance C = I - (1 - eps) n n^T (V diag(eps, 1, 1) V^T of PCL and Open3D; a zero normal
gives C = I, the sign of n cancels).  One pass at (R, t), for scan point a with normal na:
    p = R a + t                                  ((R0 x + R1 y) + R2 z) + t per row, the order of k_transform
    b = the nearest reference point (k = 1), nb its normal; the pair is kept iff sqrt(d2) <= d_max
    m = R na                                     the same order, without t
    S = 2 I - (1 - eps) (nb nb^T + m m^T),  M = S^-1 = adj(S) * (1 / det S)
    r = b - p,  J = [-[p]x, I]
    sums: count, sum p, sum b, H = sum J^T M J (upper triangle), g = sum J^T M r, sum r^T M r, sum |r|^2
and the host step xi = solve(H, g), dR = exp([xi[:3]]x), total <- (dR, xi[3:]) o total.

Every per-pair expression is written out operation by operation, left to right, in the order the kernel forms it: NumPy rounds
each once (no fused multiply-add), as the library's -ffp-contract=off build does, so the pairs' terms are the same numbers on both
sides and what is left to differ is the order of the sums.  The operation order of M, stated once:
    S_ii = 2 - c (nb_i nb_i + m_i m_i),  S_ij = -(c (nb_i nb_j + m_i m_j)),  c = 1 - eps
    adj00 = S11 S22 - S12 S12   adj01 = S02 S12 - S01 S22   adj02 = S01 S12 - S02 S11
    adj11 = S00 S22 - S02 S02   adj12 = S01 S02 - S00 S12   adj22 = S00 S11 - S01 S01
    det = (S00 adj00 + S01 adj01) + S02 adj02,  inv = 1 / det,  M_ij = adj_ij inv
"""
import math

import numpy as np
from scipy.spatial import cKDTree

N_SUMS = 40            # the layout of sf_icp_accumulate_gicp: [0] count, [1..3] sum p, [4..6] sum b, [8..28] H, [29..34] g, [35] rMr, [36] |r|^2
TRIU = [(i, j) for i in range(6) for j in range(i, 6)]
TRUE_AXIS = np.array([2.0, -1.0, 2.0]) / 3.0
TRUE_ANGLE = 0.12
TRUE_T = np.array([0.04, -0.03, 0.05])


def fsum_cols(x):
    return np.array([math.fsum(col.tolist()) for col in np.atleast_2d(x).T])


def _sum(x, how):
    if how == "fsum":
        return fsum_cols(x) if x.shape[0] else np.zeros(x.shape[1])
    return np.sum(x, axis=0)  # "np": NumPy's pairwise sum in row order


def rodrigues(om):
    """exp([om]x) = I + (sin th / th) K + 1/2 (sin(th/2) / (th/2))^2 K^2, K = [om]x, th = |om|; I when th is 0."""
    th = math.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    if not th > 0.0:
        return np.eye(3)
    ca = math.sin(th) / th
    h = math.sin(0.5 * th) / (0.5 * th)
    cb = 0.5 * (h * h)
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    return np.eye(3) + ca * K + cb * (K @ K)


def covariance(n, eps=1e-3):
    """C = I - (1 - eps) n n^T of one normal (unit, or zero)."""
    n = np.asarray(n, dtype=np.float64)
    return np.eye(3) - (1.0 - eps) * np.outer(n, n)


def rotate(R, v):
    """rows of v times R^T, in the operation order of k_transform"""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([(x * R[0, 0] + y * R[0, 1]) + z * R[0, 2],
                     (x * R[1, 0] + y * R[1, 1]) + z * R[1, 2],
                     (x * R[2, 0] + y * R[2, 1]) + z * R[2, 2]], axis=1)


def move(R, t, v):
    if R is None:
        return np.array(v, dtype=np.float64)
    return rotate(R, v) + np.asarray(t, dtype=np.float64)  # (.. + ..) + .. then + t: one more rounding per component


def information(nb, m, eps=1e-3):
    """The six unique entries (00, 01, 02, 11, 12, 22) of M = (2 I - (1 - eps)(nb nb^T + m m^T))^-1, per row, in the stated order."""
    c = 1.0 - eps
    b0, b1, b2 = nb[:, 0], nb[:, 1], nb[:, 2]
    m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
    s00 = 2.0 - c * (b0 * b0 + m0 * m0)
    s11 = 2.0 - c * (b1 * b1 + m1 * m1)
    s22 = 2.0 - c * (b2 * b2 + m2 * m2)
    s01 = -(c * (b0 * b1 + m0 * m1))
    s02 = -(c * (b0 * b2 + m0 * m2))
    s12 = -(c * (b1 * b2 + m1 * m2))
    a00 = s11 * s22 - s12 * s12
    a01 = s02 * s12 - s01 * s22
    a02 = s01 * s12 - s02 * s11
    a11 = s00 * s22 - s02 * s02
    a12 = s01 * s02 - s00 * s12
    a22 = s00 * s11 - s01 * s01
    det = (s00 * a00 + s01 * a01) + s02 * a02
    inv = 1.0 / det
    return a00 * inv, a01 * inv, a02 * inv, a11 * inv, a12 * inv, a22 * inv


def s_matrix(nb, m, eps=1e-3):
    """S of one pair as a 3 x 3 array (for the check of M against numpy.linalg.inv)."""
    return 2.0 * np.eye(3) - (1.0 - eps) * (np.outer(nb, nb) + np.outer(m, m))


def nearest(p, ref, tree=None):
    """index of the nearest reference point of each row of p, and d2 = (dx dx + dy dy) + dz dz as the kernel forms it"""
    tree = tree or cKDTree(ref)
    idx = tree.query(p, k=1)[1]
    d = ref[idx] - p
    return idx, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def terms(a, na, ref, nref, R, t, d_max, eps=1e-3, tree=None):
    """(k, 40) terms of one pass over the kept pairs, in the layout of the sums (column 0 is 1 per pair), and the (k, 40) sums of
    the magnitudes of the products each term is made of (a difference of two products adds the two magnitudes: what its rounding
    is relative to).  R = None is the identity, for the normals too."""
    a, na = np.asarray(a, dtype=np.float64), np.asarray(na, dtype=np.float64)
    p = move(R, t, a)
    idx, d2 = nearest(p, ref, tree)
    keep = np.sqrt(d2) <= d_max
    p, idx, d2 = p[keep], idx[keep], d2[keep]
    m = na[keep] if R is None else rotate(R, na[keep])
    b, nb = ref[idx], nref[idx]
    M00, M01, M02, M11, M12, M22 = information(nb, m, eps)
    M = [[M00, M01, M02], [M01, M11, M12], [M02, M12, M22]]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    r = [b[:, 0] - px, b[:, 1] - py, b[:, 2] - pz]
    Q, Qm = [[None] * 3 for _ in range(3)], [[None] * 3 for _ in range(3)]
    for j in range(3):
        Q[0][j], Qm[0][j] = py * M[2][j] - pz * M[1][j], np.abs(py * M[2][j]) + np.abs(pz * M[1][j])
        Q[1][j], Qm[1][j] = pz * M[0][j] - px * M[2][j], np.abs(pz * M[0][j]) + np.abs(px * M[2][j])
        Q[2][j], Qm[2][j] = px * M[1][j] - py * M[0][j], np.abs(px * M[1][j]) + np.abs(py * M[0][j])
    u = [(M[i][0] * r[0] + M[i][1] * r[1]) + M[i][2] * r[2] for i in range(3)]
    um = [(np.abs(M[i][0] * r[0]) + np.abs(M[i][1] * r[1])) + np.abs(M[i][2] * r[2]) for i in range(3)]
    one, z = np.ones_like(px), np.zeros_like(px)
    cols = [one, px, py, pz, b[:, 0], b[:, 1], b[:, 2], z]
    mags = [one, np.abs(px), np.abs(py), np.abs(pz), np.abs(b[:, 0]), np.abs(b[:, 1]), np.abs(b[:, 2]), z]

    def diff(x1, y1, x2, y2):  # x1 y1 - x2 y2
        cols.append(x1 * y1 - x2 * y2)
        mags.append(np.abs(x1 * y1) + np.abs(x2 * y2))

    def plain(c, mg):
        cols.append(c)
        mags.append(mg)

    # H row 0: T00 T01 T02 Q00 Q01 Q02, T = Q [p]x^T
    diff(py, Q[0][2], pz, Q[0][1]), diff(pz, Q[0][0], px, Q[0][2]), diff(px, Q[0][1], py, Q[0][0])
    plain(Q[0][0], Qm[0][0]), plain(Q[0][1], Qm[0][1]), plain(Q[0][2], Qm[0][2])
    # row 1: T11 T12 Q10 Q11 Q12
    diff(pz, Q[1][0], px, Q[1][2]), diff(px, Q[1][1], py, Q[1][0])
    plain(Q[1][0], Qm[1][0]), plain(Q[1][1], Qm[1][1]), plain(Q[1][2], Qm[1][2])
    # row 2: T22 Q20 Q21 Q22
    diff(px, Q[2][1], py, Q[2][0])
    plain(Q[2][0], Qm[2][0]), plain(Q[2][1], Qm[2][1]), plain(Q[2][2], Qm[2][2])
    # rows 3 .. 5: M
    for c in (M00, M01, M02, M11, M12, M22):
        plain(c, np.abs(c))
    # g = [p x u; u]
    diff(py, u[2], pz, u[1]), diff(pz, u[0], px, u[2]), diff(px, u[1], py, u[0])
    plain(u[0], um[0]), plain(u[1], um[1]), plain(u[2], um[2])
    plain((r[0] * u[0] + r[1] * u[1]) + r[2] * u[2], (np.abs(r[0] * u[0]) + np.abs(r[1] * u[1])) + np.abs(r[2] * u[2]))
    plain(d2, d2)
    cols += [z, z, z]
    mags += [z, z, z]
    assert len(cols) == N_SUMS
    return np.stack(cols, axis=1), np.stack(mags, axis=1)


def unpack(v):
    """40 sums -> count, H (6, 6, symmetric), g (6), sum r^T M r, sum |r|^2"""
    H = np.zeros((6, 6))
    for n, (i, j) in enumerate(TRIU):
        H[i, j] = H[j, i] = v[8 + n]
    return int(v[0]), H, np.array(v[29:35], dtype=np.float64), float(v[35]), float(v[36])


def sums(a, na, ref, nref, R, t, d_max, eps=1e-3, tree=None):
    """The 40 sums by math.fsum and the 40 sums of the magnitudes."""
    tm, mg = terms(a, na, ref, nref, R, t, d_max, eps, tree)
    return dict(vec=_sum(tm, "fsum"), abs=mg.sum(axis=0), count=tm.shape[0])


def fixed_pairs(a, na, ref, nref, R, t, idx, eps=1e-3):
    """(M (k, 3, 3), p, b) of the FIXED pairs (a_i, ref[idx_i]) with M held at (R, t)'s value: the cost g is the gradient of"""
    p = move(R, t, a)
    M00, M01, M02, M11, M12, M22 = information(nref[idx], rotate(R, na), eps)
    M = np.array([[M00, M01, M02], [M01, M11, M12], [M02, M12, M22]]).transpose(2, 0, 1)
    return M, p, ref[idx]


def icp_generalized(scan, na, ref, nref, d_max, R=None, t=None, eps=1e-3, max_iter=60, rms_threshold=0.0, step_tolerance=1e-9,
                    how="fsum"):
    """The loop of the definition.  dict(R, t, rms, converged, iterations, steps (max|xi| per iteration), counts).  how="np" sums
    with NumPy's pairwise sum in row order: on a row-permuted scan that is the statement's sensitivity to the order of its sums."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    tree = cKDTree(ref)
    steps, counts, rms, converged = [], [], 0.0, False
    for _ in range(max_iter):
        tm, _mg = terms(scan, na, ref, nref, R, t, d_max, eps, tree)
        count, H, g, _rmr, rr = unpack(_sum(tm, how))
        if count == 0:
            raise np.linalg.LinAlgError("no scan point has a reference point within d_max")
        xi = np.linalg.solve(H, g)
        dR = rodrigues(xi[:3])
        R, t = dR @ R, dR @ t + xi[3:]
        rms = math.sqrt(rr / count)
        steps.append(float(np.abs(xi).max()))
        counts.append(count)
        if rms < rms_threshold or steps[-1] < step_tolerance:
            converged = True
            break
    return dict(R=R, t=t, rms=rms, converged=converged, iterations=len(steps), steps=steps, counts=counts)


def icp_point_to_point(scan, ref, d_max, R=None, t=None, max_iter=60, step_tolerance=1e-9):
    """Point-to-point ICP: Kabsch over the kept pairs, until the step is small.  dict(R, t, iterations)."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    tree = cKDTree(ref)
    done = 0
    for _ in range(max_iter):
        p = scan @ R.T + t
        idx, d2 = nearest(p, ref, tree)
        keep = np.sqrt(d2) <= d_max
        p, q = p[keep], ref[idx[keep]]
        pm, qm = p.mean(axis=0), q.mean(axis=0)
        U, _s, Vt = np.linalg.svd((p - pm).T @ (q - qm))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
        dR = Vt.T @ D @ U.T
        dt = qm - dR @ pm
        R, t = dR @ R, dR @ t + dt
        done += 1
        if max(np.abs(dR - np.eye(3)).max(), np.abs(dt).max()) < step_tolerance:
            break
    return dict(R=R, t=t, iterations=done)


def icp_point_to_plane(scan, ref, nref, d_max, R=None, t=None, max_iter=60, step_tolerance=1e-9):
    """Point-to-plane ICP (linearised, exact exponential), until the step is small.  dict(R, t, iterations)."""
    R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
    t = np.zeros(3) if t is None else np.array(t, dtype=np.float64)
    tree = cKDTree(ref)
    done = 0
    for _ in range(max_iter):
        p = scan @ R.T + t
        idx, d2 = nearest(p, ref, tree)
        keep = np.sqrt(d2) <= d_max
        p, q, n = p[keep], ref[idx[keep]], nref[idx[keep]]
        G = np.hstack([np.cross(p, n), n])
        h = np.einsum("ij,ij->i", q - p, n)
        xi = np.linalg.solve(G.T @ G, G.T @ h)
        dR = rodrigues(xi[:3])
        R, t = dR @ R, dR @ t + xi[3:]
        done += 1
        if np.abs(xi).max() < step_tolerance:
            break
    return dict(R=R, t=t, iterations=done)


# ---- the sets of the parity table ------------------------------------------------------------------------------------------------
def true_motion():
    return rodrigues(TRUE_ANGLE * TRUE_AXIS), TRUE_T.copy()


def corner_surface(n, rng, sigma):
    """n points on three unequal planar patches meeting at the origin (z = 0: 1.0 x 0.8, y = 0: 1.0 x 0.6, x = 0: 0.8 x 0.6),
    uniform by area, plus isotropic noise."""
    area = np.array([1.0 * 0.8, 1.0 * 0.6, 0.8 * 0.6])
    which = rng.choice(3, n, p=area / area.sum())
    u, v = rng.random(n), rng.random(n)
    pts = np.where((which == 0)[:, None], np.stack([1.0 * u, 0.8 * v, 0 * u], 1),
                   np.where((which == 1)[:, None], np.stack([1.0 * u, 0 * u, 0.6 * v], 1), np.stack([0 * u, 0.8 * u, 0.6 * v], 1)))
    return pts + sigma * rng.standard_normal((n, 3))


def corner_set(seed, n=1500, sigma=0.002):
    """(scan, ref, R0, t0): scan and ref sample the surface independently; R0 scan + t0 lies on the reference's surface."""
    rng = np.random.default_rng(seed)
    ref = corner_surface(n, rng, sigma)
    world = corner_surface(n, rng, sigma)
    R0, t0 = true_motion()
    return (world - t0) @ R0, ref, R0, t0  # rows R0^T (w - t0)


def knn_normals(points, k=20):
    """unit normals: the eigenvector of the smallest eigenvalue of the covariance of the k nearest neighbours (the point included)"""
    idx = cKDTree(points).query(points, k=k)[1]
    nb = points[idx]
    d = nb - nb.mean(axis=1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", d, d) / k
    return np.ascontiguousarray(np.linalg.eigh(cov)[1][:, :, 0])


def rotation_error(R, R0):
    return float(np.linalg.norm(R - R0))
