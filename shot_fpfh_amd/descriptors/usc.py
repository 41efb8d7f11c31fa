"""Unique Shape Context on the GPU (K21; Tombari, Salti, Di Stefano 2010, pcl::UniqueShapeContext).  Not in the reference.

The 3-D shape context in SHOT's local reference frame: per keypoint a histogram over azimuth x elevation x log-radial bins of
its neighbours within `radius`, each weighted by the inverse of the local point density (the number of cloud points within
`density_radius` of the neighbour) and of the cube root of its bin's volume.  It needs no normals.

Steps (all on device): the density weights (K2's count sweep on a grid of its own, first: it rebuilds the grid) -> K1 + K2 radius
search of the keypoints -> K4 frames (from lists at `local_rf_radius` when that differs from `radius`) -> K21.
"""
from __future__ import annotations

import math
import operator
from typing import Optional

import numpy as np
import numpy.typing as npt

from .. import _ffi
from ..engine import Cloud, Engine, default_engine

__all__ = ["compute_usc_descriptor"]


def compute_usc_descriptor(
    point_cloud: npt.NDArray[np.float64],
    keypoints: npt.NDArray[np.float64],
    radius: float,
    *,
    min_radius: Optional[float] = None,
    density_radius: Optional[float] = None,
    azimuth_bins: int = 14,
    elevation_bins: int = 14,
    radius_bins: int = 10,
    local_rf_radius: Optional[float] = None,
    normalize: bool = False,
    min_neighborhood_size: int = 0,
    engine: Optional[Engine] = None,
) -> npt.NDArray[np.float64]:
    """The (m, azimuth_bins * elevation_bins * radius_bins) rows of `keypoints` (m x 3 coordinates) in `point_cloud` (n x 3),
    bin (l, k, j) at (l * elevation_bins + k) * radius_bins + j.

    min_radius: the first radial edge (radius / 10), 0 < min_radius < radius; density_radius: radius / 5; azimuth_bins even;
    at most 4096 bins in all; local_rf_radius: the frame's support (radius).  A keypoint with at most min_neighborhood_size
    neighbours at non-zero distance gets a row of zeros; normalize divides a row by its L2 norm.
    """
    radius = float(radius)
    if not (radius > 0 and math.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite (got {radius})")
    min_radius = radius / 10 if min_radius is None else float(min_radius)
    density_radius = radius / 5 if density_radius is None else float(density_radius)
    local_rf_radius = radius if local_rf_radius is None else float(local_rf_radius)
    if not 0 < min_radius < radius:
        raise ValueError(f"min_radius must lie strictly between 0 and the radius {radius} (got {min_radius})")
    for name, value in (("density_radius", density_radius), ("local_rf_radius", local_rf_radius)):
        if not (value > 0 and math.isfinite(value)):
            raise ValueError(f"{name} must be positive and finite (got {value})")
    L, K, J = operator.index(azimuth_bins), operator.index(elevation_bins), operator.index(radius_bins)
    if L < 2 or L % 2:
        raise ValueError(f"azimuth_bins must be even and at least 2 (got {L})")
    if K < 1 or J < 1:
        raise ValueError(f"elevation_bins and radius_bins must be at least 1 (got {K}, {J})")
    if L * K * J > _ffi.USC_MAX_BINS:
        raise ValueError(f"{L} x {K} x {J} bins make rows longer than {_ffi.USC_MAX_BINS}")
    pts = np.ascontiguousarray(point_cloud, dtype=np.float64)
    kp = np.ascontiguousarray(keypoints, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or kp.ndim != 2 or kp.shape[1] != 3:
        raise ValueError(f"point_cloud and keypoints must be (N, 3) arrays, got {pts.shape} and {kp.shape}")
    m, D = kp.shape[0], L * K * J
    if pts.shape[0] == 0 or m == 0:
        return np.zeros((m, D))
    eng = engine or default_engine()
    cloud = Cloud(eng, pts)
    held = []
    try:
        weights = cloud.usc_weights(density_radius, out=eng.empty((cloud.n,)))  # (first: it rebuilds the grid)
        held.append(weights)
        frames = None
        if local_rf_radius != radius:
            frames = eng.empty((m, 9))
            held.append(frames)
            support = cloud.radius_search(kp, local_rf_radius)
            try:
                support.shot_lrf(out=frames)
            finally:
                support.free()
        nbrs = cloud.radius_search(kp, radius)
        try:
            return nbrs.usc(weights, min_radius, lrf=frames, azimuth_bins=L, elevation_bins=K, radius_bins=J, normalize=normalize,
                            min_neighborhood_size=min_neighborhood_size)
        finally:
            nbrs.free()
    finally:
        for a in held:
            a.free()
        cloud.free()
