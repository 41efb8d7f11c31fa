"""Spin images on the GPU (K24; Johnson, Hebert 1999, pcl::SpinImageEstimation).  Not in the reference.

Per keypoint a small 2-D image of its ball's points in cylindrical coordinates about the keypoint's normal: alpha, the distance
from the normal line, and beta, the signed height along it, spread bilinearly over (W + 1) x (2 W + 1) nodes.  No local
reference frame: the image depends on the keypoint's normal alone.  The bilinear fractions are quantised to 2^-16 of a bin, so
bin contents are integers and a row is exact: a function of the cloud alone, the same bits on every call.  The definition is
tests/spin_numpy.py.

Steps (all on device): K1 + K2 radius search of the keypoints -> K24.

Not built: PCL's angular and radial image domains, a rotation axis other than the keypoint's own normal, compressed (PCA) images.
"""
from __future__ import annotations

import math
import operator
from typing import Optional

import numpy as np
import numpy.typing as npt

from .. import _ffi
from ..engine import Cloud, Engine, default_engine

__all__ = ["compute_spin_image_descriptor"]


def compute_spin_image_descriptor(
    keypoints_indices: npt.NDArray[np.integer],
    cloud_points: npt.NDArray[np.float64],
    normals: npt.NDArray[np.float64],
    radius: float,
    image_width: int = 8,
    *,
    signed_beta: bool = True,
    min_cos: Optional[float] = None,
    normalize: bool = False,
    min_neighborhood_size: int = 0,
    engine: Optional[Engine] = None,
) -> npt.NDArray[np.float64]:
    """The (M, D) float64 spin images of the keypoints `keypoints_indices` (indices into `cloud_points`, negative ones from the
    end, or a boolean mask over it) -- the positional shape of compute_pfh_descriptor.  The axis of a keypoint is its own
    normal, `normals[keypoints_indices]`, expected of unit length and used as given.  The image covers the cylinder of radius
    and half-height radius / sqrt 2 about it in image_width bins (1 .. 44): node (iu, iv) at iu NV + iv.

    signed_beta=True (the default here, PCL's image): beta keeps its sign, NV = 2 W + 1, D = (W + 1)(2 W + 1) = 153 at W = 8;
    it needs consistently oriented normals.  signed_beta=False folds the image over beta = 0, NV = W + 1, D = (W + 1)^2: no
    normal's sign changes a bit of it -- the choice for the normals of compute_normals, whose sign is arbitrary (and the default
    of RegistrationPipeline.compute_spin_image_descriptor).  min_cos: keep only neighbours whose normal makes an angle of cosine
    >= min_cos with the axis (|cosine| when unsigned).  normalize: rows sum to 1.  A keypoint with at most
    min_neighborhood_size contributing neighbours gets a row of zeros."""
    radius = float(radius)
    if not (radius > 0 and math.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite (got {radius})")
    W = operator.index(image_width)
    if not 1 <= W <= _ffi.SPIN_MAX_WIDTH:
        raise ValueError(f"image_width must be in 1..{_ffi.SPIN_MAX_WIDTH}, got {W}")
    if min_cos is not None and not -1.0 <= float(min_cos) <= 1.0:
        raise ValueError(f"min_cos must lie in [-1, 1] (got {min_cos})")
    min_nb = operator.index(min_neighborhood_size)
    D = (W + 1) * (2 * W + 1 if signed_beta else W + 1)
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
        return np.zeros((kp.shape[0], D))
    axes = nrm[kp]
    if not np.isfinite(axes).all():
        raise ValueError("the keypoints' normals must be finite")
    eng = engine or default_engine()
    cloud = Cloud(eng, pts, nrm)
    try:
        nbrs = cloud.radius_search(pts[kp], radius)
        try:
            return nbrs.spin_images(axes, W, signed_beta=signed_beta, min_cos=min_cos, normalize=normalize,
                                    min_neighborhood_size=min_nb)
        finally:
            nbrs.free()
    finally:
        cloud.free()
