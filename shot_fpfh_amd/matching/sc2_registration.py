"""Coarse registration from many second-order seeds (the hypothesis half of SC2-PCR; Chen, Sun, Yang, Tao, CVPR 2022) -- a fourth
estimator beside `ransac_on_matches`, `ransac_prerejective` and `fast_global_registration`, not in the reference.

`second_order_consistency_filter` grows one group from one seed, the first maximum of the second-order score s2, and everything
behind it trusts that seed.  With a few true matches in thousands the largest score can belong to an accidental clique.  Here
the n_seeds best-scored matches each get a consensus set from their own row of the second-order matrix (the filter's rule), one
Kabsch fit each, and the fits are ranked by their inlier count over ALL matches: a seed in a true clique wins on inliers even
where it loses on s2.  The matrix, the scores, the seed rows (a thin integer GEMM on the int8 matrix cores), the fits, the scoring
(K9) and the first maximum run on the device (K15, csrc/consistency.hip), queued back to back with one host wait; the winner is
then refitted over all its inliers as `ransac_prerejective` does.
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import numpy.typing as npt

from ..core import RigidTransform
from ..engine import Engine, default_engine
from .ransac import _matched_points_on_device, _refit_over_inliers
from .sc2 import SC2_MAX_MATCHES

__all__ = ["sc2_registration", "Sc2RegistrationRecord", "SC2_MAX_SEEDS"]

SC2_MAX_SEEDS = Engine.SC2_MAX_SEEDS
_TOO_FEW, _NO_TRIPLE, _NO_FIT = "fewer than three matches", "no consistent triple", "no seed gave a fit"


@dataclass
class Sc2RegistrationRecord:
    """What `sc2_registration` did: the seeds, how each fared, who won and the inlier counts after each refit that was kept."""

    status: str = "done"
    seeds: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))           # match positions, by descending score
    seed_status: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.uint8))     # 0 scored, 1 fewer than 3 members, 2 degenerate
    seed_size: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int32))       # members of each seed's consensus set
    seed_inliers: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))    # inliers over all matches (-1: not scored)
    n_too_small: int = 0
    n_degenerate: int = 0
    n_scored: int = 0
    winner_seed: int = -1      # the winning seed's match position
    winner_rank: int = -1      # its position among the seeds
    winner_size: int = 0       # its consensus size
    winner_inliers: int = 0
    refit_inliers: list = field(default_factory=list)
    second_degree: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.uint32))  # the score s2, per match


def sc2_registration(
    scan_descriptors_indices: npt.NDArray[np.integer],
    ref_descriptors_indices: npt.NDArray[np.integer],
    scan_keypoints: npt.NDArray[np.float64],
    ref_keypoints: npt.NDArray[np.float64],
    *,
    distance_threshold: float,
    min_edge: Optional[float] = None,
    n_seeds: int = 256,
    group_share: float = 0.5,
    refit_iterations: int = 2,
    verbose: bool = False,
    engine: Optional[Engine] = None,
) -> tuple[float, RigidTransform, Sc2RegistrationRecord]:
    """(inlier ratio, RigidTransform with a re-normalised rotation, Sc2RegistrationRecord) -- the first two are what
    `ransac_prerejective` returns.

    With compat, C and the score s2 as in `second_order_consistency_filter` (min_edge defaults to distance_threshold):
      1. the seeds are the n_seeds matches of the largest s2 > 0, by descending score and ascending position;
      2. a seed's row is row[j] = C[seed,j] sum_k C[seed,k] C[j,k]; its consensus set is the seed and every j with row[j] >= 1
         and row[j] >= group_share * max row -- the filter's rule; fewer than three members: the seed is left out;
      3. one Kabsch fit per seed over its members; a set without a unique rotation is left out;
      4. the fits are scored, in seed order, by the inlier count |a R^T + t - b| <= distance_threshold over ALL matches; the
         first maximum wins;
      5. the refit of `ransac_prerejective`, refit_iterations times.
    Raises ValueError for index vectors of different lengths, a distance_threshold or min_edge that is negative or not finite, a
    group_share outside (0, 1], an n_seeds outside 1 .. SC2_MAX_SEEDS, a negative refit_iterations, more than SC2_MAX_MATCHES
    matches (put `ratio_test_matching` or `geometric_consistency_filter` in front) -- and, as `ransac_prerejective` does when no
    draw survives, when nothing was scored: fewer than three matches, no consistent triple, or no seed gave a fit."""
    scan_idx, ref_idx = np.asarray(scan_descriptors_indices), np.asarray(ref_descriptors_indices)
    n_matches = int(scan_idx.shape[0])
    thr = float(distance_threshold)
    edge = thr if min_edge is None else float(min_edge)
    share = float(group_share)
    n_seeds, refit_iterations = int(n_seeds), int(refit_iterations)
    if not (math.isfinite(thr) and thr >= 0.0):
        raise ValueError(f"distance_threshold must be finite and not negative, got {distance_threshold}")
    if not (math.isfinite(edge) and edge >= 0.0):
        raise ValueError(f"min_edge must be finite and not negative, got {min_edge}")
    if not 0.0 < share <= 1.0:
        raise ValueError(f"group_share must lie in (0, 1], got {group_share}")
    if not 1 <= n_seeds <= SC2_MAX_SEEDS:
        raise ValueError(f"n_seeds must be 1 .. {SC2_MAX_SEEDS}, got {n_seeds}")
    if refit_iterations < 0:
        raise ValueError(f"refit_iterations must not be negative, got {refit_iterations}")
    if ref_idx.shape[0] != n_matches:
        raise ValueError(f"{n_matches} scan indices for {ref_idx.shape[0]} reference indices")
    if n_matches > SC2_MAX_MATCHES:
        raise ValueError(f"{n_matches} matches, at most {SC2_MAX_MATCHES}: the second-order measure works on an m x m matrix; thin "
                         "the matches first with ratio_test_matching or geometric_consistency_filter")
    if n_matches < 3:
        raise ValueError(f"nothing to fit: {_TOO_FEW} ({n_matches})")
    eng = engine or default_engine()
    held: list = []
    matched = _matched_points_on_device(eng, np.asarray(scan_keypoints), scan_idx, np.asarray(ref_keypoints), ref_idx)
    try:
        for shape, dtype in (((n_matches,), np.uint32), ((n_seeds,), np.int32), ((n_seeds,), np.uint8), ((n_seeds,), np.int32),
                             ((n_seeds,), np.int64), ((n_seeds,), np.int64)):
            held.append(eng.empty(shape, dtype))
        ds2, dseeds, dstatus, dsize, dmap, dcounts = held
        result, best = eng.sc2_registration_device(matched.a, matched.b, n_matches, thr, edge, n_seeds, share, s2=ds2, seeds=dseeds,
                                                   status=dstatus, size=dsize, slot_seed=dmap, counts=dcounts)
        found, scored = int(result[0]), int(result[3])
        seed_inliers = np.full(found, -1, dtype=np.int64)
        slot_seed = dmap.to_host()[:scored]
        seed_inliers[slot_seed] = dcounts.to_host()[:scored]
        record = Sc2RegistrationRecord(
            seeds=dseeds.to_host()[:found].astype(np.int64), seed_status=dstatus.to_host()[:found], seed_size=dsize.to_host()[:found],
            seed_inliers=seed_inliers, n_too_small=int(result[1]), n_degenerate=int(result[2]), n_scored=scored,
            winner_seed=int(result[4]), winner_rank=int(result[6]), winner_size=int(result[7]), winner_inliers=int(result[5]),
            second_degree=np.asarray(ds2.to_host()[:n_matches], dtype=np.uint32))
        if scored == 0:
            record.status = _NO_TRIPLE if found == 0 else _NO_FIT
            raise ValueError(f"nothing to fit: {record.status} ({found} seeds: {record.n_too_small} with fewer than three members, "
                             f"{record.n_degenerate} degenerate)")
        current, count, record.refit_inliers = _refit_over_inliers(eng, matched, n_matches, best, record.winner_inliers, thr,
                                                                   refit_iterations)
    finally:
        for h in held:
            h.free()
        matched.free()
    if verbose:
        logging.info(f"Seed {record.winner_seed} (rank {record.winner_rank} of {found}, consensus of {record.winner_size}), "
                     f"{record.n_scored} scored: {record.winner_inliers} inliers, after refits {record.refit_inliers}, out of {n_matches}")
    transform = RigidTransform(current[:9].reshape(3, 3).copy(), current[9:].copy())
    transform.normalize_rotation()
    return count / n_matches, transform, record
