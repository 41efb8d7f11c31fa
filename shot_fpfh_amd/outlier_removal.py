"""Outlier removal, the step in front of the normals and the keypoints (no counterpart in the reference): the two filters PCL
(`StatisticalOutlierRemoval`, `RadiusOutlierRemoval`) and Open3D (`remove_statistical_outlier`, `remove_radius_outlier`) put
there, on the MI355X -- kernels K20.

Both return the KEPT indices, int64 and ascending, in the caller's numbering (the convention of `select_keypoints_iss`);
`points[kept]` is the filtered cloud.  Invalid arguments raise ValueError before any device call.
"""
from __future__ import annotations

import numpy as np
import numpy.typing as npt

from .engine import default_engine

__all__ = ["remove_statistical_outliers", "remove_radius_outliers"]


def _points(points) -> npt.NDArray[np.float64]:
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"expected an (N, 3) array, got shape {points.shape}")
    return points


def remove_statistical_outliers(
    points: npt.NDArray[np.float64],
    nb_neighbors: int = 20,
    std_ratio: float = 2.0,
    *,
    return_stats: bool = False,
    engine=None,
):
    """Keeps the points whose mean distance to their `nb_neighbors` nearest other points is at most mu + std_ratio sigma, mu and
    sigma being the mean and the (n - 1) standard deviation of that mean distance over the cloud (PCL's rule: `<=`; an exact
    duplicate is another point at distance 0).  Needs at least two points, 1 <= nb_neighbors <= n - 1 and a finite std_ratio.
    Returns the kept int64 indices, ascending [, the mean distance of every point and the array (mu, sigma, threshold)]."""
    points = _points(points)
    n = points.shape[0]
    if n < 2:
        raise ValueError(f"the statistical filter needs at least two points (got {n})")
    if int(nb_neighbors) != nb_neighbors or not 1 <= int(nb_neighbors) <= n - 1:
        raise ValueError(f"nb_neighbors must be an integer in 1..{n - 1}, the number of other points (got {nb_neighbors})")
    std_ratio = float(std_ratio)
    if not np.isfinite(std_ratio):
        raise ValueError(f"std_ratio must be finite (got {std_ratio})")
    cloud = (engine or default_engine()).cloud(points)
    try:
        return cloud.statistical_outliers(int(nb_neighbors), std_ratio, return_stats)
    finally:
        cloud.free()


def remove_radius_outliers(
    points: npt.NDArray[np.float64],
    radius: float,
    min_neighbors: int = 2,
    *,
    return_counts: bool = False,
    engine=None,
):
    """Keeps the points that have at least `min_neighbors` OTHER points within `radius` (the project's ball rule,
    ((dx*dx + dy*dy) + dz*dz) <= r*r in float64).  Needs radius > 0 and finite, min_neighbors >= 0.  Returns the kept int64
    indices, ascending [, the int32 ball sizes, each point itself included]."""
    points = _points(points)
    radius = float(radius)
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError(f"radius must be positive and finite (got {radius})")
    if int(min_neighbors) != min_neighbors or int(min_neighbors) < 0:
        raise ValueError(f"min_neighbors must be a non-negative integer (got {min_neighbors})")
    if points.shape[0] == 0:
        empty = np.zeros(0, dtype=np.int64)
        return (empty, np.zeros(0, dtype=np.int32)) if return_counts else empty
    cloud = (engine or default_engine()).cloud(points)
    try:
        return cloud.radius_outliers(radius, int(min_neighbors), return_counts)
    finally:
        cloud.free()
