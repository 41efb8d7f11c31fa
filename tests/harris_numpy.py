"""The NumPy statement of the Harris 3D definition (float64, KDTree.query_radius balls, math.fsum sums, numpy.linalg.eigvalsh):
what tests/test_harris_host.py checks on hand-made cases and tests/test_hip_harris.py holds the device to.

Balls follow the project's rule, B(i, r) = {j : |p_j - p_i|^2 <= r^2}, i included.

1. Tensor.  k = |B(i, r)|; S_ab = sum over B of n_j[a] n_j[b] for the six pairs xx yx zx yy zy zz (the storage order of the
   covariance sweep); C = S / k, one correctly rounded division per entry.  The normals are used as given -- not normalised, a
   zero row adds nothing -- and nothing is centred.  Each product is one float64 multiplication; the sums are math.fsum's.
2. Response by method, det = det C, tr = trace C:
     harris 0.04 + det - 0.04 tr^2      noble det / tr      lowe det / tr^2      tomasi the smallest eigenvalue of C
     curvature e3 / (e1 + e2 + e3) of the mean-centred POSITION covariance of the same ball, e1 >= e2 >= e3
     (iss_numpy.ball_eigenvalues: the numbers ISS decomposes; here tr = e1 + e2 + e3).
3. response[i] = -1.0 when k < min_neighbors, tr <= 0, the matrix is numerically rank-deficient (harris, noble, lowe:
   det <= 1e-12 tr^3; tomasi: lambda_min <= 1e-12 tr; curvature: e3 <= 1e-12 e1) or the value is not > threshold (a NaN is not).
4. i is a keypoint iff response[i] > 0, |B(i, r_n)| >= min_neighbors and no j in B(i, r_n) has a larger response (exact ties are
   all kept): iss_numpy.select, unchanged.  The result is the ascending int64 indices.  r_n defaults to r.
"""
import math

import numpy as np

import iss_numpy as N

FLOOR = 1e-12
METHODS = ("harris", "noble", "lowe", "tomasi", "curvature")
TENSOR_METHODS = METHODS[:4]
U = 2.0 ** -53  # the unit roundoff of float64


def tensor(points, normals, radius):
    """(k (n,), C (n, 6), A (n, 6)): ball sizes, the tensor of rule 1 and A_ab = sum |n_a n_b| / k, which the bounds need"""
    nb = N.balls(points, radius)
    n = points.shape[0]
    C, A = np.zeros((n, 6)), np.zeros((n, 6))
    for i, idx in enumerate(nb):
        m = normals[idx]
        x, y, z = m[:, 0], m[:, 1], m[:, 2]
        prod = np.stack([x * x, y * x, z * x, y * y, z * y, z * z])
        k = idx.size
        C[i] = [math.fsum(row) / k for row in prod.tolist()]
        A[i] = [math.fsum(row) / k for row in np.abs(prod).tolist()]
    return np.array([idx.size for idx in nb]), C, A


def trace(C):
    return (C[:, 0] + C[:, 3]) + C[:, 5]


def det(C):
    c11, c21, c31, c22, c32, c33 = C.T
    return (c11 * (c22 * c33 - c32 * c32) - c21 * (c21 * c33 - c32 * c31)) + c31 * (c21 * c32 - c22 * c31)


def full(C):
    """(n, 3, 3) symmetric matrices of the six stored entries"""
    c11, c21, c31, c22, c32, c33 = C.T
    return np.stack([np.stack([c11, c21, c31], -1), np.stack([c21, c22, c32], -1), np.stack([c31, c32, c33], -1)], -2)


def lambda_min(C):
    return np.linalg.eigvalsh(full(C))[:, 0]


def value_and_rank(method, C=None, e=None):
    """(value, tr, the matrix is above its rank floor) of rule 2 and of rule 3's floors; C for the tensor methods, e (n, 3)
    descending position eigenvalues for curvature"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if method == "curvature":
            tr = (e[:, 0] + e[:, 1]) + e[:, 2]
            return e[:, 2] / tr, tr, e[:, 2] > FLOOR * e[:, 0]
        tr = trace(C)
        if method == "tomasi":
            lam = lambda_min(C)
            return lam, tr, lam > FLOOR * tr
        d = det(C)
        ok = d > FLOOR * ((tr * tr) * tr)
        if method == "harris":
            return (0.04 + d) - 0.04 * (tr * tr), tr, ok
        if method == "noble":
            return d / tr, tr, ok
        if method == "lowe":
            return d / (tr * tr), tr, ok
    raise ValueError(method)


def response_from(method, counts, C=None, e=None, threshold=0.0, min_neighbors=5):
    if threshold < 0:
        raise ValueError("threshold must not be negative")
    value, tr, ok = value_and_rank(method, C, e)
    with np.errstate(invalid="ignore"):
        keep = (counts >= min_neighbors) & (tr > 0) & ok & (value > threshold)
    return np.where(keep, value, -1.0)


def scale(method, tr):
    """the magnitude a response of this method has for a matrix of trace tr: what `rel` of near_a_threshold is relative to"""
    return {"harris": 0.04 + 0.04 * tr * tr + tr ** 3, "noble": tr * tr, "lowe": tr, "tomasi": tr, "curvature": np.ones_like(tr)}[method]


def near_a_threshold(method, C=None, e=None, threshold=0.0, rel=1e-9):
    """points whose decision may fall either way under rounding: the quantity a floor tests (det against 1e-12 tr^3, lambda_min
    against 1e-12 tr, e3 against 1e-12 e1) lies within `rel` of the floor RELATIVE TO THE QUANTITY'S SCALE (tr^3, tr, e1: the
    rounding of a float64 sum is relative to that scale, not to the floor), or the value lies within `rel` of its scale of the
    user threshold.  A matrix of trace 0 (no normals at all, coincident points) is near nothing: it is rejected by tr > 0
    whatever the rounding."""
    value, tr, _ = value_and_rank(method, C, e)
    with np.errstate(invalid="ignore"):
        if method == "curvature":
            floor = np.abs(e[:, 2] - FLOOR * e[:, 0]) <= rel * e[:, 0]
        elif method == "tomasi":
            floor = np.abs(value - FLOOR * tr) <= rel * tr
        else:
            floor = np.abs(det(C) - FLOOR * tr ** 3) <= rel * tr ** 3
        return (tr > 0) & (floor | (np.abs(value - threshold) <= rel * scale(method, tr)))


def response(points, normals, radius, method="harris", threshold=0.0, min_neighbors=5):
    if method == "curvature":
        counts, e = N.ball_eigenvalues(points, radius)
        return response_from(method, counts, e=e, threshold=threshold, min_neighbors=min_neighbors)
    counts, C, _ = tensor(points, normals, radius)
    return response_from(method, counts, C=C, threshold=threshold, min_neighbors=min_neighbors)


def keypoints(points, normals, radius, non_max_radius=None, method="harris", threshold=0.0, min_neighbors=5):
    r_n = radius if non_max_radius is None else non_max_radius
    return N.select(points, response(points, normals, radius, method, threshold, min_neighbors), r_n, min_neighbors)


# ---- the bounds the device's numbers are held to (tests/test_hip_harris.py derives them) -------------------------------
def tensor_bound(k, A):
    """|C_dev - C| per entry.  Both sides round each product once, identically.  The device then makes at most k - 1 roundings
    in its sum (any order), the statement one (fsum), and each side one in the division: (k - 1) + 1 + 2 = k + 2 roundings, each
    at most 2^-53 of sum |n_a n_b| / k; the second order is inside the 1.01."""
    return 1.01 * (k[:, None] + 2) * U * A


def response_bound(method, k, tr):
    """|response_dev - response| where both sides accept the point (derivation: the docstring of test_hip_harris.py)"""
    det_b = (k + 5) * U * tr ** 3
    if method == "harris":
        return ((k + 5.15) * tr ** 3 + (0.08 * (k + 7) + 0.24) * tr ** 2 + 0.16) * U
    if method == "noble":
        return det_b / tr + (k + 9) / 27 * U * tr ** 2
    if method == "lowe":
        return det_b / tr ** 2 + (2 * k + 17) / 27 * U * tr
    if method == "tomasi":
        return 1e-9 * tr
    return np.full(tr.shape, 1e-9)
