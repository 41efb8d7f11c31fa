"""Point Feature Histograms on the GPU (K22; Rusu, Blodow, Marton, Beetz 2008, pcl::PFHEstimation).  Not in the reference,
which has only its fast approximation, FPFH.

Per keypoint a histogram over n_bins^3 bins of the three Darboux angles of EVERY pair of points within `radius` of it --
k (k - 1) / 2 pairs for a ball of k points, where FPFH bins the k pairs through the centre.  Bin contents are integers, so a row
is exact: a function of the cloud alone, the same bits on every call.  The definition is tests/pfh_numpy.py.

Steps (all on device): K1 + K2 radius search of the keypoints -> K22.
"""
from __future__ import annotations

import math
import operator
from typing import Optional

import numpy as np
import numpy.typing as npt

from .. import _ffi
from ..engine import Cloud, Engine, default_engine

__all__ = ["compute_pfh_descriptor"]


def compute_pfh_descriptor(
    keypoints_indices: npt.NDArray[np.integer],
    cloud_points: npt.NDArray[np.float64],
    normals: npt.NDArray[np.float64],
    radius: float,
    n_bins: int = 5,
    *,
    engine: Optional[Engine] = None,
) -> npt.NDArray[np.float64]:
    """The (M, n_bins**3) float64 rows of the keypoints `keypoints_indices` (indices into `cloud_points`, or a boolean mask
    over it) -- the positional shape of compute_fpfh_descriptor.  row[b1 + S b2 + S^2 b3] = 100 x (pairs of the ball in bins
    (b1, b2, b3) of (theta, alpha, phi)) / (k (k - 1) / 2); a keypoint with fewer than two points in its ball gets zeros.
    1 <= n_bins <= 16.  Work is quadratic in the ball size."""
    radius = float(radius)
    if not (radius > 0 and math.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite (got {radius})")
    S = operator.index(n_bins)
    if not 1 <= S <= _ffi.PFH_MAX_BINS:
        raise ValueError(f"n_bins must be in 1..{_ffi.PFH_MAX_BINS}, got {S}")
    pts = np.ascontiguousarray(cloud_points, dtype=np.float64)
    nrm = np.ascontiguousarray(normals, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or nrm.shape != pts.shape:
        raise ValueError(f"cloud_points and normals must be (N, 3) arrays of one shape, got {pts.shape} and {nrm.shape}")
    kp = np.asarray(keypoints_indices)
    if kp.dtype == bool:  # NumPy boolean-mask indexing
        if kp.shape != (pts.shape[0],):
            raise ValueError(f"a boolean mask must have one entry per cloud point, got {kp.shape}")
        kp = np.flatnonzero(kp)
    kp = np.ascontiguousarray(kp, dtype=np.int64)
    if kp.ndim != 1:
        raise ValueError(f"keypoints_indices must be one-dimensional, got {kp.shape}")
    if kp.size and (kp.min() < -pts.shape[0] or kp.max() >= pts.shape[0]):
        raise ValueError("keypoints_indices out of range")
    if pts.shape[0] == 0 or kp.shape[0] == 0:
        return np.zeros((kp.shape[0], S ** 3))
    eng = engine or default_engine()
    cloud = Cloud(eng, pts, nrm)
    try:
        nbrs = cloud.radius_search(pts[kp], radius)
        try:
            return nbrs.pfh(S)
        finally:
            nbrs.free()
    finally:
        cloud.free()
