"""Geometric-consistency filter of a set of descriptor matches -- a stage between matching and the coarse registration, not in the
reference.

A rigid motion keeps lengths, so two matches i and j can both be true only if |a_i - a_j| on the scan side equals |b_i - b_j| on
the reference side within the noise (the pairwise test of PCL's GeometricConsistencyGrouping, the first-order compatibility graph
of TEASER and SC2-PCR).  True matches are compatible with each other, a wrong one with a few per cent of anything.  The m^2 pair
tests run on the device (K13, csrc/consistency.hip), the whole chain queued back to back with one host wait.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import numpy.typing as npt

from ..engine import Engine, default_engine
from .ransac import _matched_points_on_device

__all__ = ["geometric_consistency_filter", "ConsistencyRecord"]

_STATUS = {0: "done", 1: "no consistent pair"}
_TOO_FEW = "fewer than two matches"


@dataclass
class ConsistencyRecord:
    """What `geometric_consistency_filter` found."""

    status: str = "done"
    seed: int = -1          # the match compatible with the most others (the lowest such position)
    group_size: int = 0     # matches compatible with the seed, the seed included
    keep: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))             # ascending positions into the input
    degree: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.uint32))          # compatible matches, per match
    group_degree: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.uint32))    # ... counted inside the group only


def geometric_consistency_filter(
    scan_descriptors_indices: npt.NDArray[np.integer],
    ref_descriptors_indices: npt.NDArray[np.integer],
    scan_keypoints: npt.NDArray[np.float64],
    ref_keypoints: npt.NDArray[np.float64],
    *,
    distance_threshold: float,
    min_edge: Optional[float] = None,
    group_share: float = 0.4,
    verbose: bool = False,
    engine: Optional[Engine] = None,
) -> tuple[np.ndarray, np.ndarray, ConsistencyRecord]:
    """The matches that agree with each other on lengths: (scan indices kept, reference indices kept, ConsistencyRecord), the
    kept ones in input order -- directly the first two arguments of `ransac_on_matches`, `ransac_prerejective` or
    `fast_global_registration`.

    With a = scan_keypoints[scan_indices], b = ref_keypoints[ref_indices], dp(i,j) = |a_i - a_j| and dq(i,j) = |b_i - b_j|:
      compat(i,j) = i != j and |dp - dq| <= distance_threshold and min(dp, dq) >= min_edge (default: distance_threshold -- two
      matches that share a keypoint, or sit closer than the noise, constrain nothing and do not vote for each other);
      1. degree[i] = the number of j compatible with i; the seed is the first match of the largest degree;
      2. the group is the seed and the g - 1 matches compatible with it;
      3. a member is kept when it is compatible with at least group_share (g - 1) members.
    Rows that are not finite are compatible with nothing.  Fewer than two matches, or no compatible pair, give empty vectors and
    the record's status says which; nothing is raised for them.
    Raises ValueError for index vectors of different lengths, a distance_threshold or min_edge that is negative or not finite,
    and a group_share outside (0, 1]."""
    scan_idx, ref_idx = np.asarray(scan_descriptors_indices), np.asarray(ref_descriptors_indices)
    n_matches = int(scan_idx.shape[0])
    thr = float(distance_threshold)
    edge = thr if min_edge is None else float(min_edge)
    share = float(group_share)
    if not (math.isfinite(thr) and thr >= 0.0):
        raise ValueError(f"distance_threshold must be finite and not negative, got {distance_threshold}")
    if not (math.isfinite(edge) and edge >= 0.0):
        raise ValueError(f"min_edge must be finite and not negative, got {min_edge}")
    if not 0.0 < share <= 1.0:
        raise ValueError(f"group_share must lie in (0, 1], got {group_share}")
    if ref_idx.shape[0] != n_matches:
        raise ValueError(f"{n_matches} scan indices for {ref_idx.shape[0]} reference indices")
    if n_matches < 2:
        zeros = np.zeros(n_matches, dtype=np.uint32)
        return scan_idx[:0], ref_idx[:0], ConsistencyRecord(status=_TOO_FEW, degree=zeros, group_degree=zeros.copy())
    eng = engine or default_engine()
    held: list = []
    matched = _matched_points_on_device(eng, np.asarray(scan_keypoints), scan_idx, np.asarray(ref_keypoints), ref_idx)
    try:
        for dtype in (np.uint32, np.uint8, np.uint32):
            held.append(eng.empty((n_matches,), dtype))
        ddeg, dmember, dgdeg = held
        _, _, _, info = eng.consistency_group_device(matched.a, matched.b, n_matches, thr, edge, ddeg, dmember, dgdeg)
        degree, member, gdeg = ddeg.to_host()[:n_matches], dmember.to_host()[:n_matches], dgdeg.to_host()[:n_matches]
    finally:
        for h in held:
            h.free()
        matched.free()
    status, g = int(info[3]), int(info[2])
    if status != 0:
        keep = np.zeros(0, dtype=np.int64)
    else:
        keep = np.flatnonzero((member != 0) & (gdeg.astype(np.float64) >= np.float64(share) * np.float64(g - 1))).astype(np.int64)
    record = ConsistencyRecord(status=_STATUS.get(status, str(status)), seed=int(info[0]), group_size=g, keep=keep,
                               degree=np.asarray(degree, dtype=np.uint32), group_degree=np.asarray(gdeg, dtype=np.uint32))
    if verbose:
        logging.info(f"seed {record.seed} of degree {int(info[1])}, group of {g}: {keep.shape[0]} matches kept out of {n_matches}")
    return scan_idx[keep], ref_idx[keep], record
