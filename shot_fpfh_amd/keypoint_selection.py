"""Keypoint selection, the step in front of the descriptor kernels (mirrors shot_fpfh/keypoint_selection.py).

Same names, arguments and results as the reference.  Wherever the reference builds a KDTree and calls
query_radius, the lists come from the uniform-grid radius search on the MI355X (kernels K1 + K2); the
remaining logic is index bookkeeping and stays on the host.

`select_keypoints_iss` (with `cloud_resolution` and `iss_saliency`) has no counterpart in the reference: the ISS
detector (Zhong 2009, the rule of PCL's and Open3D's detectors), which looks at the geometry -- kernels K10.  Nor have
`harris_response` and `select_keypoints_harris`: the Harris 3D detector of PCL, which scores how the normals of a ball turn
-- kernels K23, with K10's suppression.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import numpy.typing as npt

from .core import grid_subsampling, voxel_closest_to_barycentre
from .engine import default_engine, harris_method_id

__all__ = [
    "select_keypoints_iteratively",
    "select_keypoints_subsampling",
    "select_keypoints_randomly",
    "select_query_indices_randomly",
    "select_keypoints_with_density_threshold",
    "cloud_resolution",
    "iss_saliency",
    "select_keypoints_iss",
    "harris_response",
    "select_keypoints_harris",
]

# module-level generator with the reference's seed (keypoint_selection.py:8); its state persists across calls
rng = np.random.default_rng(seed=1)

_BLOCK = 1 << 18  # query points per device search when sweeping a whole cloud (bounds the exported CSR)


def select_keypoints_iteratively(points: npt.NDArray[np.float64], radius: float) -> npt.NDArray[np.int64]:
    """Greedy cover (keypoint_selection.py:11-31): take the first point not yet visited, mark its spherical
    neighbourhood visited, repeat.  The neighbourhoods of ALL points are searched on the device, block by
    block; the sweep itself is sequential by definition and runs on the exported lists."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    n = points.shape[0]
    selected = np.zeros(n, dtype=bool)
    visited = np.zeros(n, dtype=bool)
    if n == 0:
        return selected.nonzero()[0]
    cloud = default_engine().cloud(points)
    try:
        for begin in range(0, n, _BLOCK):
            end = min(begin + _BLOCK, n)
            off, idx = cloud.radius_search(points[begin:end], float(radius)).export()
            for i in range(begin, end):  # the first unvisited index only moves forward
                if not visited[i]:
                    selected[i] = True
                    visited[idx[off[i - begin] : off[i - begin + 1]]] = True
    finally:
        cloud.free()
    return selected.nonzero()[0]


def select_keypoints_subsampling(points: npt.NDArray[np.float64], voxel_size: float) -> npt.NDArray[np.int64]:
    """Point closest to the barycentre of every occupied voxel (keypoint_selection.py:34-44)."""
    return grid_subsampling(points, voxel_size)


def select_keypoints_randomly(points: npt.NDArray[np.float64], n_feature_points: int) -> npt.NDArray[np.float64]:
    """Random subset of the POINTS themselves, drawn from the module-level generator (keypoint_selection.py:47-53)."""
    return rng.choice(points, n_feature_points, replace=False, shuffle=False)


def select_query_indices_randomly(n_points: int, n_feature_points: int) -> npt.NDArray[np.int64]:
    """Random subset of indices from NumPy's global generator (keypoint_selection.py:56-62)."""
    return np.random.choice(n_points, n_feature_points, replace=False)


def select_keypoints_with_density_threshold(
    points: npt.NDArray[np.float64],
    voxel_size: float,
    density_threshold_value: int,
    density_threshold_radius: Optional[float] = None,
) -> npt.NDArray[np.int64]:
    """Voxel subsampling that keeps a voxel's representative only where the cloud is dense
    (keypoint_selection.py:65-122): more than `density_threshold_value` points in the voxel itself when the
    radius is the voxel size (or None), else within `density_threshold_radius` of the representative --
    counted by one device radius search over all representatives."""
    points = np.ascontiguousarray(points, dtype=np.float64)
    picked, counts = voxel_closest_to_barycentre(points, voxel_size)
    if density_threshold_radius is None:
        density_threshold_radius = voxel_size
    if density_threshold_radius == voxel_size:
        return picked[counts > density_threshold_value]
    cloud = default_engine().cloud(points)
    try:
        density = cloud.radius_search(points[picked], float(density_threshold_radius)).counts()
    finally:
        cloud.free()
    return picked[density > density_threshold_value]


# ---- ISS (Intrinsic Shape Signatures): saliency + non-maximum suppression on the device (K10) ------------------------
def _iss_points(points) -> npt.NDArray[np.float64]:
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"expected an (N, 3) array, got shape {points.shape}")
    return points


def _iss_radius(name: str, value) -> float:
    value = float(value)
    if not (np.isfinite(value) and value > 0.0):
        raise ValueError(f"{name} must be positive and finite (got {value})")
    return value


def _iss_rule(gamma_21: float, gamma_32: float, min_neighbors: int) -> None:
    for name, g in (("gamma_21", gamma_21), ("gamma_32", gamma_32)):
        if not 0.0 < float(g) <= 1.0:
            raise ValueError(f"{name} must lie in (0, 1] (got {g})")
    if int(min_neighbors) < 1:
        raise ValueError(f"min_neighbors must be at least 1 (got {min_neighbors})")


def cloud_resolution(points: npt.NDArray[np.float64], *, engine=None) -> float:
    """Mean over all points of the distance to the nearest OTHER point (the k = 2 self query, second column: exact
    duplicates contribute 0)."""
    points = _iss_points(points)
    if points.shape[0] < 2:
        raise ValueError("the resolution of a cloud needs at least two points")
    cloud = (engine or default_engine()).cloud(points)
    try:
        return cloud.resolution(points)
    finally:
        cloud.free()


def iss_saliency(
    points: npt.NDArray[np.float64],
    salient_radius: float,
    gamma_21: float = 0.975,
    gamma_32: float = 0.975,
    min_neighbors: int = 5,
    *,
    engine=None,
) -> npt.NDArray[np.float64]:
    """ISS saliency of every point: with e1 >= e2 >= e3 the eigenvalues of the covariance of the ball of `salient_radius`
    around it (the point included; mean-centred, divided by the ball's size), e3 if the ball holds at least
    `min_neighbors` points, e2 / e1 < gamma_21, e3 / e2 < gamma_32, e1 > 0, e2 > 0 and e3 > 1e-12 e1 -- else -1.0."""
    points = _iss_points(points)
    salient_radius = _iss_radius("salient_radius", salient_radius)
    _iss_rule(gamma_21, gamma_32, min_neighbors)
    if points.shape[0] == 0:
        return np.zeros(0, dtype=np.float64)
    cloud = (engine or default_engine()).cloud(points)
    try:
        return cloud.iss_saliency(salient_radius, gamma_21, gamma_32, min_neighbors)
    finally:
        cloud.free()


def select_keypoints_iss(
    points: npt.NDArray[np.float64],
    salient_radius: Optional[float] = None,
    non_max_radius: Optional[float] = None,
    gamma_21: float = 0.975,
    gamma_32: float = 0.975,
    min_neighbors: int = 5,
    *,
    return_saliency: bool = False,
    engine=None,
):
    """ISS keypoints: the points whose saliency (iss_saliency) is positive, that have at least `min_neighbors` points
    within `non_max_radius` (themselves included) and none among them with a strictly larger saliency -- exact ties are all
    kept.  int64 indices into `points`, ascending [, the saliency of every point].  A radius left None is 6 (salient) resp.
    4 (non-maximum) times the cloud's resolution (cloud_resolution); a resolution of 0 or fewer than two points then
    raise ValueError."""
    points = _iss_points(points)
    if salient_radius is not None:
        salient_radius = _iss_radius("salient_radius", salient_radius)
    if non_max_radius is not None:
        non_max_radius = _iss_radius("non_max_radius", non_max_radius)
    _iss_rule(gamma_21, gamma_32, min_neighbors)
    n = points.shape[0]
    if n == 0:
        empty = np.zeros(0, dtype=np.int64)
        return (empty, np.zeros(0, dtype=np.float64)) if return_saliency else empty
    automatic = salient_radius is None or non_max_radius is None
    if automatic and n < 2:
        raise ValueError("automatic ISS radii need at least two points")
    cloud = (engine or default_engine()).cloud(points)
    try:
        if automatic:
            rho = cloud.resolution(points)
            if not rho > 0.0:
                raise ValueError("automatic ISS radii need a cloud resolution above 0 (every point has an exact duplicate)")
            salient_radius = 6.0 * rho if salient_radius is None else salient_radius
            non_max_radius = 4.0 * rho if non_max_radius is None else non_max_radius
        return cloud.iss_keypoints(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, return_saliency)
    finally:
        cloud.free()


# ---- Harris 3D: the response of the normals' tensor + K10's non-maximum suppression on the device (K23) ---------------
def _harris_rule(method: str, threshold: float, min_neighbors: int) -> None:
    harris_method_id(method)  # (ValueError for an unknown one)
    if not (np.isfinite(float(threshold)) and float(threshold) >= 0.0):
        raise ValueError(f"threshold must be finite and not negative (got {threshold}): the suppression only considers responses above 0")
    if int(min_neighbors) < 1:
        raise ValueError(f"min_neighbors must be at least 1 (got {min_neighbors})")


def _harris_normals(points, normals, method: str):
    """the normals as an (N, 3) float64 array, or None where the method needs none"""
    if normals is None:
        if method != "curvature":
            raise ValueError(f'method "{method}" is computed from the normals: pass them, or use method="curvature"')
        return None
    normals = np.ascontiguousarray(normals, dtype=np.float64)
    if normals.shape != points.shape:
        raise ValueError(f"normals must have the shape of points {points.shape}, got {normals.shape}")
    if not np.isfinite(normals).all():
        raise ValueError("normals hold a non-finite component")
    return normals


def harris_response(
    points: npt.NDArray[np.float64],
    normals: Optional[npt.NDArray[np.float64]],
    radius: float,
    *,
    method: str = "harris",
    threshold: float = 0.0,
    min_neighbors: int = 5,
    engine=None,
) -> npt.NDArray[np.float64]:
    """Harris 3D response of every point (pcl::HarrisKeypoint3D's rule).  With C the mean of n n^T over the ball of `radius`
    around the point (itself included; the normals as given, their sign does not matter): "harris" 0.04 + det C - 0.04 tr(C)^2,
    "noble" det C / tr C, "lowe" det C / tr(C)^2, "tomasi" the smallest eigenvalue of C, "curvature" the surface variation
    e3 / (e1 + e2 + e3) of the ball's position covariance (`normals` may be None) -- or -1.0 where the ball holds fewer than
    `min_neighbors` points, the matrix is numerically rank-deficient (a flat patch) or the value is not above `threshold`."""
    points = _iss_points(points)
    radius = _iss_radius("radius", radius)
    _harris_rule(method, threshold, min_neighbors)
    normals = _harris_normals(points, normals, method)
    if points.shape[0] == 0:
        return np.zeros(0, dtype=np.float64)
    cloud = (engine or default_engine()).cloud(points, normals)
    try:
        return cloud.harris_response(radius, method, threshold, min_neighbors)
    finally:
        cloud.free()


def select_keypoints_harris(
    points: npt.NDArray[np.float64],
    normals: Optional[npt.NDArray[np.float64]] = None,
    radius: Optional[float] = None,
    non_max_radius: Optional[float] = None,
    *,
    method: str = "harris",
    threshold: float = 0.0,
    min_neighbors: int = 5,
    return_response: bool = False,
    engine=None,
):
    """Harris 3D keypoints: the points whose response (harris_response) is positive, that have at least `min_neighbors`
    points within `non_max_radius` (themselves included) and none among them with a strictly larger response -- exact ties are
    all kept.  int64 indices into `points`, ascending [, the response of every point].  `radius` None: 6 times the cloud's
    resolution (cloud_resolution), as ISS; `non_max_radius` None: `radius`, as PCL uses one radius.  `normals` None is accepted
    for method="curvature" alone."""
    points = _iss_points(points)
    if radius is not None:
        radius = _iss_radius("radius", radius)
    if non_max_radius is not None:
        non_max_radius = _iss_radius("non_max_radius", non_max_radius)
    _harris_rule(method, threshold, min_neighbors)
    normals = _harris_normals(points, normals, method)
    n = points.shape[0]
    if n == 0:
        empty = np.zeros(0, dtype=np.int64)
        return (empty, np.zeros(0, dtype=np.float64)) if return_response else empty
    if radius is None and n < 2:
        raise ValueError("an automatic Harris radius needs at least two points")
    cloud = (engine or default_engine()).cloud(points, normals)
    try:
        if radius is None:
            rho = cloud.resolution(points)
            if not rho > 0.0:
                raise ValueError("an automatic Harris radius needs a cloud resolution above 0 (every point has an exact duplicate)")
            radius = 6.0 * rho
        return cloud.harris_keypoints(radius, non_max_radius, method, threshold, min_neighbors, return_response)
    finally:
        cloud.free()
