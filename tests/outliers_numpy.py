"""The NumPy statement of the two outlier filters (K20): what tests/test_outliers_host.py checks on known clouds and
tests/test_hip_outliers.py holds the device to.  Both use the project's ball rule, ((dx*dx + dy*dy) + dz*dz) <= r*r in float64
without FMA, self included (sklearn's KDTree).

Statistical, k neighbours, std_ratio:
    d[i, 0..k]  the distances sqrt(d2) of the k + 1 nearest cloud points of point i (KDTree(p).query(p, k + 1)); the smallest is
                always 0, the point itself or an exact duplicate
    mean[i]     sum_j d[i, j] / k: the mean distance to the k nearest OTHER points (ties in d2 change which index is taken,
                never the distances)
    mu          fsum(mean) / n;   sigma = sqrt(fsum((mean - mu)^2) / (n - 1));   threshold = mu + std_ratio * sigma
    kept        mean[i] <= threshold (PCL's rule)
    needs n >= 2, 1 <= k <= n - 1, std_ratio finite
Radius, radius, min_neighbors:
    count[i]    the size of point i's ball, i included;   kept: count[i] - 1 >= min_neighbors
    needs radius > 0, min_neighbors >= 0
Both return the kept indices as ascending int64.
"""
import math

import numpy as np
from sklearn.neighbors import KDTree

from conftest import config1_cloud


def mean_distance(points, k):
    n = points.shape[0]
    if n < 2 or not 1 <= k <= n - 1:
        raise ValueError("n >= 2 and 1 <= k <= n - 1")
    d = KDTree(points).query(points, k + 1)[0]
    return d.sum(axis=1) / k


def stats(mean, std_ratio):
    """(mu, sigma, threshold) of a mean-distance array, the two sums by math.fsum"""
    if not math.isfinite(std_ratio):
        raise ValueError("std_ratio must be finite")
    n = mean.shape[0]
    mu = math.fsum(mean) / n
    sigma = math.sqrt(math.fsum((mean - mu) ** 2) / (n - 1))
    return mu, sigma, mu + std_ratio * sigma


def statistical(points, k, std_ratio):
    """(kept indices, mean, (mu, sigma, threshold))"""
    mean = mean_distance(points, k)
    st = stats(mean, std_ratio)
    return np.flatnonzero(mean <= st[2]).astype(np.int64), mean, st


def ball_counts(points, radius):
    if not radius > 0:
        raise ValueError("radius > 0")
    return KDTree(points).query_radius(points, radius, count_only=True)


def radius(points, radius_, min_neighbors):
    """(kept indices, counts)"""
    if min_neighbors < 0:
        raise ValueError("min_neighbors >= 0")
    counts = ball_counts(points, radius_)
    return np.flatnonzero(counts - 1 >= min_neighbors).astype(np.int64), counts


def contaminated_sphere(n, n_out, seed):
    """config1_cloud(n, seed)'s noisy sphere stacked with n_out strays, uniform in the cube [-0.25, 1.25)^3 on the float32 grid:
    rows n .. n + n_out - 1 are the strays."""
    rng = np.random.default_rng(seed + 100)
    strays = rng.random((n_out, 3), dtype=np.float32) * 1.5 - 0.25
    return np.vstack([config1_cloud(n, seed)[0], strays.astype(np.float64)])
