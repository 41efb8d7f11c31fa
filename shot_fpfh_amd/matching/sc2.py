"""Second-order consistency filter of a set of descriptor matches (SC2; Chen, Sun, Yang, Tao, CVPR 2022) -- a stage between
matching and the coarse registration, not in the reference.

`geometric_consistency_filter` seeds its group with the match compatible with the most others.  With a few per cent of true
matches that count no longer separates: a wrong match is compatible with about 2 % of everything by accident, which at 5 000
matches outweighs the few dozen true votes.  The second-order measure counts, for a match i, the PAIRS (j, k) compatible with i
and with each other -- twice the triangles through i in the compatibility graph.  True matches form a clique, accidental
agreements do not.  The m^2 pair tests and the m^3 triangle count (an integer GEMM on the int8 matrix cores) run on the device
(K14, csrc/consistency.hip), the whole chain queued back to back with one host wait.
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

__all__ = ["second_order_consistency_filter", "SecondOrderRecord", "SC2_MAX_MATCHES"]

SC2_MAX_MATCHES = Engine.SC2_MAX_MATCHES  # the m x m byte matrix is 1 GiB there
_STATUS = {0: "done", 1: "no consistent triple"}
_TOO_FEW = "fewer than three matches"


@dataclass
class SecondOrderRecord:
    """What `second_order_consistency_filter` found."""

    status: str = "done"
    seed: int = -1          # the match of the largest second-order score (the lowest such position)
    seed_score: int = 0     # its score
    group_size: int = 0     # matches compatible with the seed, the seed included
    keep: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))              # ascending positions into the input
    second_degree: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.uint32))    # the score, per match
    seed_row: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.uint32))         # SC2[seed, .]


def second_order_consistency_filter(
    scan_descriptors_indices: npt.NDArray[np.integer],
    ref_descriptors_indices: npt.NDArray[np.integer],
    scan_keypoints: npt.NDArray[np.float64],
    ref_keypoints: npt.NDArray[np.float64],
    *,
    distance_threshold: float,
    min_edge: Optional[float] = None,
    group_share: float = 0.5,
    verbose: bool = False,
    engine: Optional[Engine] = None,
) -> tuple[np.ndarray, np.ndarray, SecondOrderRecord]:
    """The matches that agree with each other on lengths, chosen by second-order consistency: (scan indices kept, reference
    indices kept, SecondOrderRecord), the kept ones in input order -- directly the first two arguments of `ransac_on_matches`,
    `ransac_prerejective` or `fast_global_registration`.

    With compat(i,j) as in `geometric_consistency_filter` (min_edge defaults to distance_threshold) and C its 0/1 matrix:
      1. N[i,j] = sum_k C[i,k] C[j,k], SC2[i,j] = C[i,j] N[i,j], the score s2[i] = sum_j SC2[i,j]; the seed is the first match
         of the largest score;
      2. the group is the seed and the g - 1 matches compatible with it;
      3. a member j is kept when SC2[seed,j] >= 1 and SC2[seed,j] >= group_share * max SC2[seed,.]; the seed is kept.
    Rows that are not finite are compatible with nothing.  Fewer than three matches, or no three matches compatible with each
    other, give empty vectors and the record's status says which; nothing is raised for them.
    Raises ValueError for index vectors of different lengths, a distance_threshold or min_edge that is negative or not finite, a
    group_share outside (0, 1], and more than SC2_MAX_MATCHES matches (the matrix is m^2 bytes: put `ratio_test_matching` or
    `geometric_consistency_filter` in front)."""
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
    if n_matches > SC2_MAX_MATCHES:
        raise ValueError(f"{n_matches} matches, at most {SC2_MAX_MATCHES}: the second-order measure works on an m x m matrix; thin "
                         "the matches first with ratio_test_matching or geometric_consistency_filter")
    if n_matches < 3:
        zeros = np.zeros(n_matches, dtype=np.uint32)
        return scan_idx[:0], ref_idx[:0], SecondOrderRecord(status=_TOO_FEW, second_degree=zeros, seed_row=zeros.copy())
    eng = engine or default_engine()
    held: list = []
    matched = _matched_points_on_device(eng, np.asarray(scan_keypoints), scan_idx, np.asarray(ref_keypoints), ref_idx)
    try:
        for dtype in (np.uint32, np.uint8, np.uint32):
            held.append(eng.empty((n_matches,), dtype))
        ds2, dmember, dgdeg = held
        _, _, _, info = eng.consistency_sc2_group_device(matched.a, matched.b, n_matches, thr, edge, ds2, dmember, dgdeg)
        s2, member, gdeg = ds2.to_host()[:n_matches], dmember.to_host()[:n_matches], dgdeg.to_host()[:n_matches]
    finally:
        for h in held:
            h.free()
        matched.free()
    status, seed, g = int(info[3]), int(info[0]), int(info[2])
    row = np.zeros(n_matches, dtype=np.uint32)
    if status != 0:
        keep = np.zeros(0, dtype=np.int64)
    else:
        # the degree over the member columns counts the seed too, and every other member is compatible with it: SC2[seed, j] is
        # one less
        inside = member != 0
        inside[seed] = False
        row[inside] = gdeg[inside] - 1
        top = np.float64(row.max(initial=0))
        kept = (row >= 1) & (row.astype(np.float64) >= np.float64(share) * top)
        kept[seed] = True
        keep = np.flatnonzero(kept).astype(np.int64)
    record = SecondOrderRecord(status=_STATUS.get(status, str(status)), seed=seed, seed_score=int(info[1]), group_size=g, keep=keep,
                               second_degree=np.asarray(s2, dtype=np.uint32), seed_row=row)
    if verbose:
        logging.info(f"seed {record.seed} of score {record.seed_score}, group of {g}: {keep.shape[0]} matches kept out of {n_matches}")
    return scan_idx[keep], ref_idx[keep], record
