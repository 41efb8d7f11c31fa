"""The NumPy statement of the ISS definition (float64, KDTree.query_radius balls, numpy.linalg.eigvalsh): what
tests/test_iss_host.py checks on hand-made cases and tests/test_hip_iss.py holds the device to.

1. saliency[i] = e3 of the mean-centred covariance (divided by the ball's size) of B_s(i) = {j : |p_j - p_i|^2 <= r_s^2}, i
   included, with eigenvalues e1 >= e2 >= e3 -- if |B_s(i)| >= min_neighbors, e2 / e1 < gamma_21, e3 / e2 < gamma_32, e1 > 0,
   e2 > 0 and e3 > 1e-12 e1; else -1.0.
2. i is a keypoint iff saliency[i] > 0, |B_n(i)| >= min_neighbors and no j in B_n(i) has saliency[j] > saliency[i] (strict:
   exact ties are all kept).
3. The result is the ascending int64 indices.
"""
import numpy as np
from sklearn.neighbors import KDTree

FLOOR = 1e-12


def balls(points, radius):
    return KDTree(points).query_radius(points, radius)


def ball_eigenvalues(points, radius):
    """(counts (n,), eigenvalues (n, 3) as e1 >= e2 >= e3)"""
    nb = balls(points, radius)
    cov = np.zeros((points.shape[0], 3, 3))
    for i, idx in enumerate(nb):
        c = points[idx] - points[idx].mean(axis=0)
        cov[i] = c.T @ c / idx.size
    return np.array([idx.size for idx in nb]), np.linalg.eigvalsh(cov)[:, ::-1]


def saliency_from(counts, e, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    e1, e2, e3 = e[:, 0], e[:, 1], e[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = (counts >= min_neighbors) & (e1 > 0) & (e2 > 0) & (e2 / e1 < gamma_21) & (e3 / e2 < gamma_32) & (e3 > FLOOR * e1)
    return np.where(ok, e3, -1.0)


def near_a_threshold(e, gamma_21=0.975, gamma_32=0.975, rel=1e-9):
    """points whose eigenvalues sit within `rel`, relative, of one of the three thresholds (a ball of coincident points,
    e1 == 0, is near none: it is rejected by e1 > 0 whatever the rounding)"""
    e1, e2, e3 = e[:, 0], e[:, 1], e[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (e1 > 0) & ((np.abs(e2 / e1 - gamma_21) <= rel * gamma_21) | (np.abs(e3 / e2 - gamma_32) <= rel * gamma_32)
                           | (np.abs(e3 - FLOOR * e1) <= rel * FLOOR * e1))


def saliency(points, radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    counts, e = ball_eigenvalues(points, radius)
    return saliency_from(counts, e, gamma_21, gamma_32, min_neighbors)


def select(points, score, radius, min_neighbors=5):
    nb = balls(points, radius)
    keep = [i for i, idx in enumerate(nb)
            if score[i] > 0 and idx.size >= min_neighbors and not (score[idx] > score[i]).any()]
    return np.array(keep, dtype=np.int64)


def keypoints(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    return select(points, saliency(points, salient_radius, gamma_21, gamma_32, min_neighbors), non_max_radius, min_neighbors)


def resolution(points):
    return float(KDTree(points).query(points, k=2)[0][:, 1].mean())


def bumpy_sphere(n=30000, seed=5):
    """Sphere of radius 0.4 about (0.5, 0.5, 0.5) with 40 Gaussian bumps (height 0.08, width 0.06) around random unit
    directions, float32-grid coordinates.  The generator draws the 40 bump directions first, then the n point directions."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((40, 3))
    c /= np.linalg.norm(c, axis=1)[:, None]
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    h = (0.08 * np.exp(-((d[:, None, :] - c[None, :, :]) ** 2).sum(axis=2) / (2 * 0.06 ** 2))).sum(axis=1)
    return (0.5 + 0.4 * d * (1.0 + h)[:, None]).astype(np.float32).astype(np.float64)
