"""ICP refinement on the GPU -- drop-in for shot_fpfh.icp (icp.py:20-189) and core.solvers.compute_point_to_point_error
(solvers.py:51-62).

How an iteration is split.  The reference does everything in NumPy around a KDTree query: transform the working points,
query their nearest reference points, mask the pairs farther than `d_max`, build the centred 3x3 cross-covariance
(point-to-point) or the 6x6 normal equations (point-to-plane) from the masked arrays, solve, compose.  Here the working
points and the reference cloud live in HBM for the whole run and ONE device call per iteration (`sf_icp_accumulate`,
csrc/icp.hip) does the transform, the nearest-neighbour search (grid k-NN kernel, k = 1), the `d_max` filter and the
reductions; what crosses the bus per iteration is a 12-number transform one way and ~30 sums the other.  The host keeps
only the tiny dense step -- a 3x3 SVD (`_rigid_fit`) or a 6x6 solve (`_plane_fit`) on those sums -- and the bookkeeping of
the running transform.  `_Registration` is that device state; the public functions differ only in which rows they
feed it, which fit they ask for and what they return.

`icp_generalized` (K16) has no counterpart in the reference: generalized, or plane-to-plane, ICP (Segal, Haehnel, Thrun, RSS
2009).  Every point carries the covariance C = I - (1 - epsilon) n n^T of its unit normal, a pair (a, b) is weighted by
M = (C_b + R C_a R^T)^-1, and the device call (`sf_icp_accumulate_gicp`, the same chain in its third mode) returns the
6x6 Gauss-Newton system of sum r^T M r; the host solves it and applies the exact exponential of the step (`_gicp_fit`).

`icp_robust` (K17) runs any of the three with a robust loss: the device call (`sf_icp_accumulate_robust`) weights every pair inside
`d_max` by psi(r) / r of its residual (Huber, Cauchy, Geman-McClure, Tukey) and returns the weighted sums; the host solves the
same small systems and anneals the loss's scale from `scale_start` down to `scale`, the graduated scheme of
`fast_global_registration`.  From a coarse start a fixed small scale is no better than no loss at all, so the annealing is part of it.

`icp_trimmed` (K18) runs any of the three, with or without a loss, as trimmed ICP (Chetverikov, Stepanov, Krsek 2002/2005): the device
call (`sf_icp_accumulate_trimmed`) finds the exact order statistic of the residuals of the pairs inside `d_max` that bounds their
best-fitting share (a radix selection, csrc/select.hip) and sums over the pairs up to it only.  The share comes down from 1 to
`overlap` over the first iterations: a fixed share from a coarse start is worse than no trimming, the same lesson as the scale's.

`icp_symmetric` (K19) has no counterpart in the reference either: the symmetric point-to-plane objective (Rusinkiewicz, SIGGRAPH
2019).  A pair's residual is taken along the mean of its two normals and its lever arm is p + b, so it vanishes whenever the pair
lies on a common second-order patch, not only on a common plane; the 6x6 system is point-to-plane's, with no per-pair inverse.  The
device call (`sf_icp_accumulate_symmetric`, the chain in its fourth mode) carries a loss and a trim of its own, and the host applies
the paper's rotate-translate-rotate step (`_symmetric_fit`).

Deviation, on purpose: the reference's `icp_point_to_point` computes its RMS from `ref[neighbors]` (all queried points,
shape (n, 1, 3)) instead of `ref[inliers_neighbors]` (icp.py:122-124); the broadcast yields an array, and formatting it for
the progress bar raises TypeError on the first iteration, so that function cannot run there at all.  Here the RMS is taken
over the inlier pairs, as in `icp_point_to_point_with_sampling`.
"""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import Optional

import numpy as np
import numpy.typing as npt
from scipy.spatial.transform import Rotation

from . import _ffi
from .core import RigidTransform, grid_subsampling
from .core.geometry import kabsch_from_covariance
from .descriptors.normals import compute_normals
from .engine import Cloud, DeviceArray, Engine, default_engine

__all__ = [
    "icp_point_to_point_with_sampling",
    "icp_point_to_point",
    "icp_point_to_plane",
    "icp_generalized",
    "icp_robust",
    "icp_trimmed",
    "icp_symmetric",
    "compute_point_to_point_error",
    "nearest_within",
]

_POINT, _PLANE, _GICP = 0, 1, 2
# The chain's fourth mode has a call of its own (sf_icp_accumulate_symmetric) and is NOT a `mode` of the shared calls, which keep
# rejecting 3: `_MODES` stays their three, and `pairs` tells the symmetric objective by this marker, never by a number.
_SYMMETRIC = "symmetric"
_TRIU = np.triu_indices(6)
_MODES = {"point_to_point": _POINT, "point_to_plane": _PLANE, "generalized": _GICP}
LOSSES = {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3, "tukey": 4}  # the `loss` of sf_icp_accumulate_robust


def _checked_rows(rows, n: int) -> np.ndarray:
    """A row selection as the int64 array the device reads (it gathers pts[3 * rows[i]] unchecked): one-dimensional, every
    id in 0 .. n-1, repeats allowed; an empty selection stays empty."""
    ids = np.asarray(rows)
    if ids.ndim != 1:
        raise ValueError(f"rows: expected a one-dimensional selection, got shape {ids.shape}")
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError(f"rows: expected integer ids, got dtype {ids.dtype}")
    bad = np.flatnonzero((ids < 0) | (ids >= n)) if ids.size else ids[:0]  # (compared in the caller's dtype: a uint64 id >= 2^63 is caught)
    if bad.size:
        raise IndexError(f"rows[{int(bad[0])}] = {int(ids[bad[0]])} is not a row of the {n} working points (0 .. {n - 1})")
    return np.ascontiguousarray(ids, dtype=np.int64)


class _PairSums:
    """What one device pass returns about the inlier pairs (p = moved working point, q = its nearest reference point).  The 48
    numbers of a pass with a robust loss have every fit term weighted, and the weight's own sums behind them."""

    def __init__(self, raw: np.ndarray, mode: int):
        self.raw = raw
        if raw.shape[0] == 48:
            self.sum_w = float(raw[7])                # sum w
            self.sum_wp, self.sum_wq = raw[40:43], raw[43:46]
            self.sum_wr2 = float(raw[46])             # sum w r2 (r2: the mode's squared residual)
            # a trimmed pass (sf_icp_accumulate_trimmed): `count` is the USED pairs; zero otherwise
            self.inside, self.rank, self.cut = int(raw[37]), int(raw[38]), float(raw[47])
        self.count = int(raw[0])
        self.sum_p, self.sum_q = raw[1:4], raw[4:7]
        if mode == _POINT:
            self.cross_cov = raw[8:17].reshape(3, 3)  # sum (p - pbar)(q - qbar)^T
            self.sq_dist = float(raw[17])             # sum |p - q|^2
        else:
            self.gtg = np.zeros((6, 6))
            self.gtg[_TRIU] = raw[8:29]
            self.gtg = self.gtg + np.triu(self.gtg, 1).T
            self.gth = raw[29:35]
            if mode == _PLANE:
                self.abs_h = float(raw[35])           # sum |(q - p) . n|
            elif mode == _SYMMETRIC:                  # gtg = sum w g g^T, gth = sum w g h, g = [(p + q) x n, n], n the mean normal
                self.abs_h = float(raw[35])           # sum |(q - p) . n|
                self.sq_dist = float(raw[36])         # sum |q - p|^2
            else:                                     # generalized: gtg = sum J^T M J, gth = sum J^T M r, J = [-[p]x, I], r = q - p
                self.mahalanobis = float(raw[35])     # sum r^T M r
                self.sq_dist = float(raw[36])         # sum |r|^2

    def require_pairs(self) -> None:
        if self.count == 0:
            raise np.linalg.LinAlgError("ICP: no scan point has a reference point within d_max")

    def require_weight(self, scale: float) -> None:
        self.require_pairs()
        if not self.sum_w > 0.0:
            raise np.linalg.LinAlgError(f"ICP: all {self.count} pairs within d_max have weight zero at the loss's scale {scale!r}: "
                                        "every residual lies beyond it")


def _rigid_fit(s: _PairSums) -> RigidTransform:
    """Kabsch from the centred cross-covariance (core/solvers.py:9-30: same SVD, same reflection rule)."""
    s.require_pairs()
    return kabsch_from_covariance(s.cross_cov, s.sum_p / s.count, s.sum_q / s.count)


def _weighted_rigid_fit(s: _PairSums) -> RigidTransform:
    """Kabsch on the weighted cross-covariance and the weighted centroids the device centred it with."""
    return kabsch_from_covariance(s.cross_cov, s.sum_wp / s.sum_w, s.sum_wq / s.sum_w)


def _plane_fit(s: _PairSums) -> RigidTransform:
    """Linearised point-to-plane step from G^T G and G^T h (core/solvers.py:33-48)."""
    s.require_pairs()
    s.step = sol = np.linalg.solve(s.gtg, s.gth)
    return RigidTransform(Rotation.from_euler("xyz", sol[:3]).as_matrix(), sol[3:6])


def _rodrigues(omega: np.ndarray) -> np.ndarray:
    """exp([omega]x) = I + (sin th / th) K + 1/2 (sin(th/2) / (th/2))^2 K^2, K = [omega]x, th = |omega|."""
    th = math.sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
    if not th > 0.0:
        return np.eye(3)
    ca = math.sin(th) / th
    h = math.sin(0.5 * th) / (0.5 * th)
    K = np.array([[0.0, -omega[2], omega[1]], [omega[2], 0.0, -omega[0]], [-omega[1], omega[0], 0.0]])
    return np.eye(3) + ca * K + (0.5 * (h * h)) * (K @ K)


def _gicp_fit(s: _PairSums) -> RigidTransform:
    """Gauss-Newton step of sum r^T M r from H = sum J^T M J and g = sum J^T M r: the EXACT exponential of the rotation part
    (`_plane_fit`'s Euler product is the reference's and stays with it)."""
    s.require_pairs()
    s.step = np.linalg.solve(s.gtg, s.gth)
    return RigidTransform(_rodrigues(s.step[:3]), s.step[3:6])


def _symmetric_fit(s: _PairSums) -> RigidTransform:
    """The step of the symmetric objective from x = solve(sum w g g^T, sum w g h) = [a~, t~]: theta = atan |a~|, R_h the rotation
    by theta about e = a~ / |a~|, and p <- R_h (R_h p + cos(theta) t~ + (1 - cos(theta))(e . t~) e) -- the paper's rotate, translate,
    rotate, without its centring, and with t~'s component along the axis left unscaled: that is (I - [a~]x)^-1 t~ turned by R_h^-1,
    the exact translation of the linear system, so a rigid copy with exact pairs is recovered in ONE step (the paper's cos(theta) t~
    leaves the share 1 - cos(theta) of that component to the next iteration; the fixed points are the same)."""
    s.require_pairs()
    s.step = np.linalg.solve(s.gtg, s.gth)
    norm = math.sqrt((s.step[0] * s.step[0] + s.step[1] * s.step[1]) + s.step[2] * s.step[2])
    if not norm > 0.0:
        return RigidTransform(np.eye(3), s.step[3:6])
    theta = math.atan(norm)
    half = _rodrigues((theta / norm) * s.step[:3])
    e, c = s.step[:3] / norm, math.cos(theta)
    along = (e[0] * s.step[3] + e[1] * s.step[4]) + e[2] * s.step[5]
    return RigidTransform(half @ half, half @ (c * s.step[3:6] + ((1.0 - c) * along) * e))


class _Registration:
    """Working points + reference cloud resident on one GPU for the length of an ICP run; for generalized ICP also the
    working points' normals (`scan_normals`, one unit or zero row per point)."""

    def __init__(self, points, ref, ref_normals=None, engine: Optional[Engine] = None, scan_normals=None):
        self.engine = engine or default_engine()
        self.ref = Cloud(self.engine, ref, ref_normals)
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise ValueError(f"expected an (N, 3) array, got shape {pts.shape}")
        self.n = pts.shape[0]
        self.points: DeviceArray = self.engine.empty((max(self.n, 1), 3)).from_host(pts if self.n else np.zeros((1, 3)))
        self.rows: Optional[DeviceArray] = None
        self.normals: Optional[DeviceArray] = None
        if scan_normals is not None:
            nrm = np.ascontiguousarray(scan_normals, dtype=np.float64)
            if nrm.shape != pts.shape:
                self.close()
                raise ValueError(f"scan normals of shape {nrm.shape} for points of shape {pts.shape}")
            self.normals = self.engine.empty((max(self.n, 1), 3)).from_host(nrm if self.n else np.zeros((1, 3)))

    def pairs(self, mode: int, d_max: float, moved_by: Optional[RigidTransform] = None, rows=None,
              epsilon: float = 1e-3, loss: Optional[int] = None, scale: float = 1.0, trim: float = 1.0) -> _PairSums:
        """Inlier-pair sums of the working points (all of them, or the given `rows`) after `moved_by`; with a `loss` (0 .. 4,
        `LOSSES`) the 48 weighted sums of sf_icp_accumulate_robust at `scale`; with a `trim` below 1 the 48 sums of
        sf_icp_accumulate_trimmed over that share of the pairs (a trim of 1.0 is the call without one).  The symmetric mode has
        one call, sf_icp_accumulate_symmetric, for all of it: always 48 numbers, no loss being loss 0."""
        m, sel = self.n, None
        if rows is not None:
            rows = _checked_rows(rows, self.n)
            m = rows.shape[0]
            if self.rows is None or self.rows.shape[0] < m:
                if self.rows is not None:
                    self.rows.free()
                self.rows = self.engine.empty((max(m, 1),), np.int64)
            if m:
                _ffi.check(self.engine.lib.sf_h2d(self.engine.h, self.rows.ptr, rows.ctypes.data_as(C.c_void_p), m * 8), "sf_h2d")
            sel = self.rows.ptr
        rt = None if moved_by is None else np.ascontiguousarray(moved_by.as_row12())
        if mode in (_GICP, _SYMMETRIC) and self.normals is None:
            raise ValueError(f"{'generalized' if mode == _GICP else 'symmetric'} ICP needs the normals of the working points")
        trimmed = float(trim) != 1.0
        raw = np.zeros(40 if loss is None and not trimmed and mode != _SYMMETRIC else 48)
        head = (self.engine.h, self.ref.h, self.points.ptr)
        rows_and_motion = (sel, m, None if rt is None else rt.ctypes.data_as(C.c_void_p), float(d_max))
        out = raw.ctypes.data_as(C.c_void_p)
        if mode == _SYMMETRIC:
            name, args = "sf_icp_accumulate_symmetric", (*head, self.normals.ptr, *rows_and_motion, int(loss or 0), float(scale),
                                                         float(trim), out)
        elif trimmed:
            name, args = "sf_icp_accumulate_trimmed", (*head, self.normals.ptr if mode == _GICP else None, *rows_and_motion, int(mode),
                                                       float(epsilon), int(loss or 0), float(scale), float(trim), out)
        elif loss is not None:
            name, args = "sf_icp_accumulate_robust", (*head, self.normals.ptr if mode == _GICP else None, *rows_and_motion, int(mode),
                                                      float(epsilon), int(loss), float(scale), out)
        elif mode == _GICP:  # without a loss the plain entry points and their 40 numbers
            name, args = "sf_icp_accumulate_gicp", (*head, self.normals.ptr, *rows_and_motion, float(epsilon), out)
        else:
            name, args = "sf_icp_accumulate", (*head, *rows_and_motion, mode, out)
        _ffi.check(getattr(self.engine.lib, name)(*args), name)
        return _PairSums(raw, mode)

    def move(self, transform: RigidTransform) -> None:
        """points <- transform[points], in place in HBM."""
        rt = np.ascontiguousarray(transform.as_row12())
        _ffi.check(self.engine.lib.sf_transform_points(self.engine.h, self.points.ptr, self.n, rt.ctypes.data_as(C.c_void_p)),
                   "sf_transform_points")

    def download(self) -> np.ndarray:
        return self.points.to_host()[: self.n]

    def close(self) -> None:
        for obj in (self.points, self.rows, self.normals, self.ref):
            if obj is not None:
                obj.free()


def icp_point_to_point_with_sampling(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    d_max: float,
    max_iter: int = 100,
    rms_threshold: float = 1e-2,
    sampling_limit: int = 100,
    disable_progress_bar: bool = False,
) -> tuple[npt.NDArray[np.float64], float, bool]:
    """Point-to-point ICP fitted on a fresh random subset per iteration and applied to ALL points (icp.py:20-78).
    Subsets are drawn from NumPy's global generator exactly as the reference draws them.
    Returns (aligned points, rms of the last fit = sqrt(sum of squared inlier distances), converged)."""
    reg = _Registration(scan, ref)
    limit = min(sampling_limit, reg.n)
    rms = 0.0
    try:
        for _ in range(max_iter):
            subset = np.random.choice(reg.n, limit, replace=False)
            found = reg.pairs(_POINT, d_max, rows=subset)
            reg.move(_rigid_fit(found))
            rms = float(np.sqrt(found.sq_dist))
            if rms < rms_threshold:
                break
    except KeyboardInterrupt:
        logging.info("ICP interrupted by user.")
    try:
        return reg.download(), rms, rms < rms_threshold
    finally:
        reg.close()


def _refine(reg: _Registration, start: RigidTransform, mode: int, d_max: float, max_iter: int, rms_threshold: float,
            epsilon: float = 1e-3, step_tolerance: float = 0.0):
    """The loop shared by icp_point_to_point, icp_point_to_plane and icp_generalized: the working points stay where they are,
    the running transform is what moves (icp.py:103-130, 155-189).  Generalized ICP also stops, converged, once no component of
    its step reaches `step_tolerance`."""
    total, rms, small_step = start, 0.0, False
    fit = {_POINT: _rigid_fit, _PLANE: _plane_fit, _GICP: _gicp_fit}[mode]
    try:
        for _ in range(max_iter):
            found = reg.pairs(mode, d_max, moved_by=total, epsilon=epsilon)
            total = fit(found) @ total
            # residual of the pairs the fit was computed FROM (before this iteration's update), as in the reference
            if mode == _POINT:
                rms = float(np.sqrt(found.sq_dist))
            elif mode == _PLANE:
                rms = found.abs_h / found.count
            else:
                rms = float(np.sqrt(found.sq_dist / found.count))
                small_step = bool(np.abs(found.step).max() < step_tolerance)
            if rms < rms_threshold:
                logging.info("RMS threshold reached.")
                break
            if small_step:
                logging.info("Step tolerance reached.")
                break
    except KeyboardInterrupt:
        logging.info("ICP interrupted by user.")
    return total, rms, rms < rms_threshold or small_step


def icp_point_to_point(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    transformation_init: RigidTransform,
    d_max: float,
    voxel_size: float = 0.2,
    max_iter: int = 100,
    rms_threshold: float = 1e-2,
    disable_progress_bar: bool = False,
) -> tuple[RigidTransform, float, bool]:
    """Point-to-point ICP on the voxel-subsampled scan (icp.py:81-130; see the module note on its RMS)."""
    scan = np.asarray(scan)
    reg = _Registration(scan[grid_subsampling(scan, voxel_size)], ref)
    try:
        return _refine(reg, transformation_init, _POINT, d_max, max_iter, rms_threshold)
    finally:
        reg.close()


def icp_point_to_plane(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    ref_normals: npt.NDArray[np.float64],
    transformation_init: RigidTransform,
    d_max: float,
    voxel_size: float = 0.2,
    max_iter: int = 50,
    rms_threshold: float = 1e-2,
    disable_progress_bar: bool = False,
) -> tuple[RigidTransform, float, bool]:
    """Point-to-plane ICP (icp.py:133-189): the returned rms is the mean |(inlier - neighbour) . normal| of the pairs
    the last step was fitted on."""
    scan = np.asarray(scan)
    reg = _Registration(scan[grid_subsampling(scan, voxel_size)], ref, ref_normals)
    try:
        return _refine(reg, transformation_init, _PLANE, d_max, max_iter, rms_threshold)
    finally:
        reg.close()


def _unit_rows(normals, n: int, what: str) -> np.ndarray:
    """(n, 3) float64 rows scaled to unit length on the host; zero rows stay zero."""
    nrm = np.array(normals, dtype=np.float64)
    if nrm.shape != (n, 3):
        raise ValueError(f"{what} of shape {nrm.shape}: expected ({n}, 3), one row per point")
    length = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    return np.ascontiguousarray(nrm / np.where(length > 0.0, length, 1.0)[:, None])


def _both_normals(scan, ref, scan_normals, ref_normals, k_normals: int):
    """Unit normals of both clouds for generalized ICP: the given ones scaled to unit length, the others from `k_normals`
    neighbours of the full cloud."""
    given = [None if nrm is None else _unit_rows(nrm, a.shape[0], f"{name} normals")
             for name, a, nrm in (("scan", scan, scan_normals), ("ref", ref, ref_normals))]
    for name, a, nrm in (("scan", scan, given[0]), ("ref", ref, given[1])):
        if nrm is None and not 3 <= int(k_normals) <= a.shape[0]:
            raise ValueError(f"k_normals={k_normals} must be between 3 and the number of {name} points ({a.shape[0]})")
    return tuple(nrm if nrm is not None else _unit_rows(compute_normals(a, a, k=int(k_normals)), a.shape[0], "normals")
                 for a, nrm in ((scan, given[0]), (ref, given[1])))


def icp_generalized(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    transformation_init: RigidTransform,
    d_max: float,
    *,
    scan_normals: Optional[npt.NDArray[np.float64]] = None,
    ref_normals: Optional[npt.NDArray[np.float64]] = None,
    k_normals: int = 20,
    epsilon: float = 1e-3,
    voxel_size: float = 0.2,
    max_iter: int = 50,
    rms_threshold: float = 1e-2,
    step_tolerance: float = 1e-9,
) -> tuple[RigidTransform, float, bool]:
    """Generalized (plane-to-plane) ICP, K16: every pair is weighted by the local surface of BOTH clouds, a point's covariance
    being I - (1 - epsilon) n n^T of its unit normal.  Normals that are not given are computed on the full clouds from
    `k_normals` neighbours; the scan is then voxel-subsampled like its siblings' and its normals follow the selection.
    Returns (transform, rms = sqrt(mean squared distance) of the pairs the last step was fitted on, converged); converged
    means rms < rms_threshold or a step whose largest component is below step_tolerance."""
    scan, ref = np.asarray(scan, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    for name, a in (("scan", scan), ("ref", ref)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: expected an (N, 3) array, got shape {a.shape}")
    if not 0.0 < epsilon <= 1.0:
        raise ValueError(f"epsilon={epsilon} must lie in (0, 1]")
    if not step_tolerance >= 0.0:
        raise ValueError(f"step_tolerance={step_tolerance} must not be negative")
    scan_normals, ref_normals = _both_normals(scan, ref, scan_normals, ref_normals, k_normals)
    keep = grid_subsampling(scan, voxel_size)
    reg = _Registration(scan[keep], ref, ref_normals, scan_normals=scan_normals[keep])
    try:
        return _refine(reg, transformation_init, _GICP, d_max, max_iter, rms_threshold, epsilon, step_tolerance)
    finally:
        reg.close()


def annealed_scale(scale: float, scale_start: float, division_factor: float, iteration: int) -> float:
    """The loss's scale of iteration i: max(scale, scale_start / division_factor**i)."""
    try:
        return max(scale, scale_start / division_factor**iteration)
    except OverflowError:  # division_factor**i beyond the doubles: the quotient is long below any scale
        return scale


def trimmed_overlap(overlap: float, anneal_iterations: int, iteration: int) -> float:
    """The share of the pairs iteration i of trimmed ICP uses: max(overlap, 1 - (1 - overlap) i / anneal_iterations), from 1 down to
    `overlap` in `anneal_iterations` equal steps; `anneal_iterations=0` uses `overlap` throughout."""
    if anneal_iterations <= 0:
        return overlap
    return max(overlap, 1.0 - (1.0 - overlap) * iteration / anneal_iterations)


def _refine_robust(reg: _Registration, start: RigidTransform, mode: int, d_max: float, loss: int, scale: float, scale_start: float,
                   division_factor: float, max_iter: int, rms_threshold: float, epsilon: float, step_tolerance: float,
                   overlap: float = 1.0, anneal_iterations: int = 0):
    """The loop of `_refine` with a weight per pair: the scale of iteration i is `annealed_scale(.., i)`, the residual reported is
    the mode's unweighted one, and a small step stops the run only once the scale has come down to `scale`.  With an `overlap`
    below 1 (K18) iteration i fits the share `trimmed_overlap(.., i)` of the pairs, the residual is over the pairs used, and a
    small step stops the run only once the share, too, has come down to `overlap`."""
    total, rms, small_step = start, 0.0, False
    fit = {_POINT: _weighted_rigid_fit, _PLANE: _plane_fit, _GICP: _gicp_fit, _SYMMETRIC: _symmetric_fit}[mode]
    try:
        for i in range(max_iter):
            k = annealed_scale(scale, scale_start, division_factor, i)
            share = trimmed_overlap(overlap, anneal_iterations, i)
            found = reg.pairs(mode, d_max, moved_by=total, epsilon=epsilon, loss=loss, scale=k, trim=share)
            found.require_weight(k)
            step = fit(found)
            total = step @ total
            if mode == _POINT:
                rms = float(np.sqrt(found.sq_dist))
                size = max(float(np.abs(step.rotation - np.eye(3)).max()), float(np.abs(step.translation).max()))
            else:
                rms = found.abs_h / found.count if mode in (_PLANE, _SYMMETRIC) else float(np.sqrt(found.sq_dist / found.count))
                size = float(np.abs(found.step).max())
            small_step = k == scale and share == overlap and size < step_tolerance
            if rms < rms_threshold:
                logging.info("RMS threshold reached.")
                break
            if small_step:
                logging.info("Step tolerance reached.")
                break
    except KeyboardInterrupt:
        logging.info("ICP interrupted by user.")
    return total, rms, rms < rms_threshold or small_step


def icp_robust(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    transformation_init: RigidTransform,
    d_max: float,
    *,
    mode: str = "point_to_plane",
    loss: str = "cauchy",
    scale: float,
    scale_start: Optional[float] = None,
    division_factor: float = 1.4,
    ref_normals: Optional[npt.NDArray[np.float64]] = None,
    scan_normals: Optional[npt.NDArray[np.float64]] = None,
    k_normals: int = 20,
    epsilon: float = 1e-3,
    voxel_size: float = 0.2,
    max_iter: int = 50,
    rms_threshold: float = 1e-2,
    step_tolerance: float = 1e-9,
) -> tuple[RigidTransform, float, bool]:
    """Point-to-point, point-to-plane or generalized ICP with a robust loss, K17: every pair within `d_max` is weighted by
    psi(r) / r of its residual r -- the distance, the distance along the reference normal, or the Mahalanobis distance
    sqrt(r^T M r) of generalized ICP -- so that what the scan sees and the reference does not (clutter, another object, the part
    without overlap) stops pulling the fit.  `loss`: "none", "huber", "cauchy", "geman_mcclure", "tukey".  `scale` is the loss's
    k in the residual's unit (a few sigma of the noise); iteration i uses max(scale, scale_start / division_factor**i), with
    `scale_start` = `d_max` unless given, and `scale_start=scale` switches the annealing off.
    "point_to_plane" needs `ref_normals`; "generalized" treats normals as `icp_generalized` does.
    Returns (transform, rms, converged) with the mode's own UNWEIGHTED rms (see its function), so that runs with and without a
    loss compare; converged means rms < rms_threshold, or, once the scale has reached `scale`, a step below `step_tolerance`:
    max|xi| of the 6-vector step, max(|dR - I|, |dt|) for point-to-point.  When every pair has weight zero (Tukey with all
    residuals beyond the scale) numpy.linalg.LinAlgError names the scale."""
    if mode not in _MODES:
        raise ValueError(f"mode={mode!r}: expected one of {sorted(_MODES)}")
    if loss not in LOSSES:
        raise ValueError(f"loss={loss!r}: expected one of {sorted(LOSSES)}")
    if scale is None or not 0.0 < float(scale) < math.inf:
        raise ValueError(f"scale={scale!r} must be positive and finite")
    scale_start = d_max if scale_start is None else scale_start
    if not 0.0 < float(scale_start) < math.inf:
        raise ValueError(f"scale_start={scale_start!r} must be positive and finite (it defaults to d_max)")
    if not 1.0 < float(division_factor) < math.inf:
        raise ValueError(f"division_factor={division_factor!r} must be greater than 1 (scale_start=scale switches the annealing off)")
    if not 0.0 < epsilon <= 1.0:
        raise ValueError(f"epsilon={epsilon} must lie in (0, 1]")
    if not step_tolerance >= 0.0:
        raise ValueError(f"step_tolerance={step_tolerance} must not be negative")
    scan, ref = np.asarray(scan, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    for name, a in (("scan", scan), ("ref", ref)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: expected an (N, 3) array, got shape {a.shape}")
    kind = _MODES[mode]
    if kind == _PLANE and ref_normals is None:
        raise ValueError("mode='point_to_plane' needs ref_normals")
    if kind == _GICP:
        scan_normals, ref_normals = _both_normals(scan, ref, scan_normals, ref_normals, k_normals)
    keep = grid_subsampling(scan, voxel_size)
    reg = _Registration(scan[keep], ref, ref_normals if kind != _POINT else None,
                        scan_normals=scan_normals[keep] if kind == _GICP else None)
    try:
        return _refine_robust(reg, transformation_init, kind, d_max, LOSSES[loss], float(scale), float(scale_start),
                              float(division_factor), max_iter, rms_threshold, epsilon, step_tolerance)
    finally:
        reg.close()


def icp_trimmed(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    transformation_init: RigidTransform,
    d_max: float,
    *,
    overlap: float,
    anneal_iterations: int = 10,
    mode: str = "point_to_plane",
    loss: str = "none",
    scale: Optional[float] = None,
    scale_start: Optional[float] = None,
    division_factor: float = 1.4,
    ref_normals: Optional[npt.NDArray[np.float64]] = None,
    scan_normals: Optional[npt.NDArray[np.float64]] = None,
    k_normals: int = 20,
    epsilon: float = 1e-3,
    voxel_size: float = 0.2,
    max_iter: int = 50,
    rms_threshold: float = 1e-2,
    step_tolerance: float = 1e-9,
) -> tuple[RigidTransform, float, bool]:
    """Trimmed point-to-point, point-to-plane or generalized ICP, K18 (Chetverikov, Stepanov, Krsek 2002/2005): every iteration
    fits only the best-fitting share of its pairs, those whose squared residual -- the mode's own, as in `icp_robust` -- is at most
    the ceil(share * n0)-th smallest of the n0 pairs within `d_max`, ties at that value included.  `overlap` in (0, 1] is that
    share: roughly how much of the scan the reference also sees.  It is a share of the pairs INSIDE `d_max`; with `d_max = inf`
    every scan point has a pair and it is Chetverikov's share of the scan.  It needs no scale and no unit.
    Iteration i uses max(overlap, 1 - (1 - overlap) i / anneal_iterations): from a coarse start what the reference does not have
    may fit better than what it has, and a fixed share is then worse than no trimming; `anneal_iterations=0` switches the
    annealing off.  An overestimated overlap buys little; point-to-point gains least from trimming (README, K18).
    A `loss` other than "none" weights the pairs used as `icp_robust` does and needs its `scale`; the other arguments are
    `icp_robust`'s.  Returns (transform, rms, converged) with the mode's own rms over the pairs USED by the last fit; converged
    means rms < rms_threshold, or a step below `step_tolerance` once the share has reached `overlap` (and the scale `scale`).
    `overlap=1.0` with loss "none" returns what the plain function of the mode returns."""
    if mode not in _MODES:
        raise ValueError(f"mode={mode!r}: expected one of {sorted(_MODES)}")
    if loss not in LOSSES:
        raise ValueError(f"loss={loss!r}: expected one of {sorted(LOSSES)}")
    if overlap is None or not 0.0 < float(overlap) <= 1.0:
        raise ValueError(f"overlap={overlap!r} must lie in (0, 1]")
    if int(anneal_iterations) != anneal_iterations or anneal_iterations < 0:
        raise ValueError(f"anneal_iterations={anneal_iterations!r} must be a non-negative integer (0 switches the annealing off)")
    if loss == "none":
        scale = scale_start = 1.0  # no weight looks at it
    elif scale is None or not 0.0 < float(scale) < math.inf:
        raise ValueError(f"scale={scale!r} must be positive and finite (loss={loss!r} needs one)")
    scale_start = d_max if scale_start is None else scale_start
    if not 0.0 < float(scale_start) < math.inf:
        raise ValueError(f"scale_start={scale_start!r} must be positive and finite (it defaults to d_max)")
    if not 1.0 < float(division_factor) < math.inf:
        raise ValueError(f"division_factor={division_factor!r} must be greater than 1 (scale_start=scale switches the annealing off)")
    if not 0.0 < epsilon <= 1.0:
        raise ValueError(f"epsilon={epsilon} must lie in (0, 1]")
    if not step_tolerance >= 0.0:
        raise ValueError(f"step_tolerance={step_tolerance} must not be negative")
    scan, ref = np.asarray(scan, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    for name, a in (("scan", scan), ("ref", ref)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: expected an (N, 3) array, got shape {a.shape}")
    kind = _MODES[mode]
    if kind == _PLANE and ref_normals is None:
        raise ValueError("mode='point_to_plane' needs ref_normals")
    if kind == _GICP:
        scan_normals, ref_normals = _both_normals(scan, ref, scan_normals, ref_normals, k_normals)
    keep = grid_subsampling(scan, voxel_size)
    reg = _Registration(scan[keep], ref, ref_normals if kind != _POINT else None,
                        scan_normals=scan_normals[keep] if kind == _GICP else None)
    try:
        return _refine_robust(reg, transformation_init, kind, d_max, LOSSES[loss], float(scale), float(scale_start),
                              float(division_factor), max_iter, rms_threshold, epsilon, step_tolerance, float(overlap),
                              int(anneal_iterations))
    finally:
        reg.close()


def icp_symmetric(
    scan: npt.NDArray[np.float64],
    ref: npt.NDArray[np.float64],
    transformation_init: RigidTransform,
    d_max: float,
    *,
    scan_normals: Optional[npt.NDArray[np.float64]] = None,
    ref_normals: Optional[npt.NDArray[np.float64]] = None,
    k_normals: int = 20,
    loss: str = "none",
    scale: Optional[float] = None,
    scale_start: Optional[float] = None,
    division_factor: float = 1.4,
    overlap: float = 1.0,
    anneal_iterations: int = 10,
    voxel_size: float = 0.2,
    max_iter: int = 50,
    rms_threshold: float = 1e-2,
    step_tolerance: float = 1e-9,
) -> tuple[RigidTransform, float, bool]:
    """Symmetric point-to-plane ICP, K19 (Rusinkiewicz, SIGGRAPH 2019): a pair's residual is h = (b - p) . n along the mean
    n = (nb + s R na) / 2 of the reference point's normal and the moved scan point's (s = +-1 makes them agree in sign, so the
    orientation of either normal does not matter), and its lever arm is p + b.  h vanishes whenever the pair lies on a common
    second-order patch, not only on a common plane, at point-to-plane's cost: the same 6x6 system, no per-pair inverse, no
    epsilon.  Normals are treated as `icp_generalized` treats them: computed from `k_normals` neighbours of the full clouds when
    not given, normalised when given, zero rows kept (n is then half the other normal).
    `loss` and `scale` (.. `scale_start`, `division_factor`) weight the pairs as `icp_robust` does, from h h, in point-to-plane's
    unit; `overlap` below 1 (.. `anneal_iterations`) fits only that share of them as `icp_trimmed` does.
    Returns (transform, rms = mean |h| of the pairs the last step was fitted on, converged); converged means rms < rms_threshold,
    or a step x = [a~, t~] with max|x| < step_tolerance once scale and share have come down."""
    if loss not in LOSSES:
        raise ValueError(f"loss={loss!r}: expected one of {sorted(LOSSES)}")
    if overlap is None or not 0.0 < float(overlap) <= 1.0:
        raise ValueError(f"overlap={overlap!r} must lie in (0, 1]")
    if int(anneal_iterations) != anneal_iterations or anneal_iterations < 0:
        raise ValueError(f"anneal_iterations={anneal_iterations!r} must be a non-negative integer (0 switches the annealing off)")
    if loss == "none":
        scale = scale_start = 1.0  # no weight looks at it
    elif scale is None or not 0.0 < float(scale) < math.inf:
        raise ValueError(f"scale={scale!r} must be positive and finite (loss={loss!r} needs one)")
    scale_start = d_max if scale_start is None else scale_start
    if not 0.0 < float(scale_start) < math.inf:
        raise ValueError(f"scale_start={scale_start!r} must be positive and finite (it defaults to d_max)")
    if not 1.0 < float(division_factor) < math.inf:
        raise ValueError(f"division_factor={division_factor!r} must be greater than 1 (scale_start=scale switches the annealing off)")
    if not step_tolerance >= 0.0:
        raise ValueError(f"step_tolerance={step_tolerance} must not be negative")
    scan, ref = np.asarray(scan, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    for name, a in (("scan", scan), ("ref", ref)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: expected an (N, 3) array, got shape {a.shape}")
    scan_normals, ref_normals = _both_normals(scan, ref, scan_normals, ref_normals, k_normals)
    keep = grid_subsampling(scan, voxel_size)
    reg = _Registration(scan[keep], ref, ref_normals, scan_normals=scan_normals[keep])
    try:
        return _refine_robust(reg, transformation_init, _SYMMETRIC, d_max, LOSSES[loss], float(scale), float(scale_start),
                              float(division_factor), max_iter, rms_threshold, 1.0, step_tolerance, float(overlap),
                              int(anneal_iterations))
    finally:
        reg.close()


def compute_point_to_point_error(
    scan: npt.NDArray[np.float64], ref: npt.NDArray[np.float64], transformation: RigidTransform
) -> tuple[float, npt.NDArray[np.float64]]:
    """RMS nearest-neighbour distance of the transformed scan to the reference cloud, and the transformed scan
    (core/solvers.py:51-62).  Every point counts: no d_max."""
    reg = _Registration(scan, ref)
    try:
        found = reg.pairs(_POINT, np.inf, moved_by=transformation)
    finally:
        reg.close()
    return float(np.sqrt(found.sq_dist / max(found.count, 1))), transformation[np.asarray(scan)]


def nearest_within(points: npt.NDArray[np.float64], against: npt.NDArray[np.float64], distance: float) -> int:
    """How many of `points` have a point of `against` within `distance` (the `KDTree(ref).query(...)[0] <= thr` masks
    of pipeline.py:560-587, summed) -- counted on the device."""
    reg = _Registration(points, against)
    try:
        return reg.pairs(_POINT, distance).count
    finally:
        reg.close()
