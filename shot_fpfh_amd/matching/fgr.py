"""Fast global registration over descriptor matches (Zhou, Park, Koltun, ECCV 2016) -- a third coarse registration beside
`ransac_on_matches` and `ransac_prerejective`, not in the reference.

It draws nothing: a scaled Geman-McClure cost over ALL matches is minimised by graduated non-convexity, a fixed sequence of
weighted Gauss-Newton steps that runs entirely on the device (K12, csrc/fgr.hip: one pass over the matches and one 6 x 6 solve per
iteration, queued back to back, one host wait at the end).  The result is a pure function of the input.
"""
from __future__ import annotations

import logging
import math
import operator
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import numpy.typing as npt

from ..core import RigidTransform
from ..engine import Engine, default_engine
from .ransac import _matched_points_on_device, draw_stream

__all__ = ["fast_global_registration", "FgrRecord"]

_STATUS = {0: "done", 1: "degenerate", 2: "no extent"}


@dataclass
class FgrRecord:
    """What `fast_global_registration` did."""

    status: str = "done"
    iterations: int = 0     # Gauss-Newton steps taken
    mu: float = 1.0         # final mu, in normalised units
    scale: float = 0.0      # s: the largest distance of a matched point from its side's centroid
    rows: int = 0           # rows fitted: all matches, or 3 per surviving tuple
    inliers: int = 0        # matches within distance_threshold of the returned transform, out of ALL matches
    trace: np.ndarray = field(default_factory=lambda: np.zeros((0, 4)))  # per iteration: mu, E, W, |xi|


def _tuple_selection(eng: Engine, matched, n_matches: int, tuple_count: int, tuple_scale: float, seed: int, held: list) -> np.ndarray:
    """The paper's tuple test from K11's pieces: triples of matches whose three pairs of edges agree within tuple_scale; the match
    ids of the first tuple_count survivors in draw order, duplicates kept."""
    n_draws = 100 * tuple_count
    draws = draw_stream(np.random.default_rng(seed), n_matches, 3, n_draws)
    ddraws = eng.empty((n_draws, 3), np.int64)
    held.append(ddraws)
    status = eng.empty((n_draws,), np.uint8)
    held.append(status)
    rt = eng.empty((n_draws, 12))
    held.append(rt)
    ddraws.from_host(draws)
    eng.ransac_hypotheses_device(matched.a, matched.b, n_matches, ddraws, n_draws, 3, float(tuple_scale), status, rt)
    keep = np.flatnonzero(status.to_host()[:n_draws] == 0)[:tuple_count]
    if keep.size < 1:
        raise ValueError(f"none of {n_draws} triples of matches passed the tuple test at scale {tuple_scale}")
    return np.ascontiguousarray(draws[keep].reshape(-1), dtype=np.int64)


def fast_global_registration(
    scan_descriptors_indices: npt.NDArray[np.integer],
    ref_descriptors_indices: npt.NDArray[np.integer],
    scan_keypoints: npt.NDArray[np.float64],
    ref_keypoints: npt.NDArray[np.float64],
    *,
    distance_threshold: float,
    iterations: int = 64,
    division_factor: float = 1.4,
    decrease_every: int = 4,
    tuple_count: int = 0,
    tuple_scale: float = 0.95,
    seed: int = 72,
    verbose: bool = False,
    engine: Optional[Engine] = None,
) -> tuple[float, RigidTransform, FgrRecord]:
    """Fast global registration: (inlier ratio, RigidTransform with a re-normalised rotation, FgrRecord).

    With a = scan_keypoints[scan_indices], b = ref_keypoints[ref_indices] (all matches, or the rows of the tuple test):
      1. ca, cb the means, s = max(max |a - ca|, max |b - cb|), x = (a - ca) / s, y = (b - cb) / s;
      2. R = I, t = 0, mu = 1; `iterations` times one Gauss-Newton step on sum mu r.r / (mu + r.r), r = R x + t - y (weights
         (mu / (mu + r.r))^2, exact rotation update); after every decrease_every-th step mu <- max(mu / division_factor,
         (distance_threshold / s)^2);
      3. t is taken back to the keypoints' units; the inlier ratio is the share of ALL matches with |a R^T + t - b| <=
         distance_threshold.
    tuple_count > 0: 100 tuple_count triples of matches are drawn from np.random.default_rng(seed), those whose edge lengths
    agree within tuple_scale on both sides survive, and the first tuple_count survivors' matches are what is fitted.  With
    tuple_count = 0 (the default) nothing is drawn and `seed` is not used.
    Raises ValueError for fewer than 3 matches, bad parameters, no surviving tuple, matched points without extent, and when the
    weighted points do not determine a rigid motion: a pivot d_j of the 6 x 6 system's LDL^T with d_j <= 1e-12 A_jj, which is what
    rounding leaves of an exact zero.  That is points on one line, or closer to one than about 1e-6 of their extent; thin slabs
    and needles a thousand times longer than wide are fitted."""
    scan_idx, ref_idx = np.asarray(scan_descriptors_indices), np.asarray(ref_descriptors_indices)
    n_matches = int(scan_idx.shape[0])
    try:
        iterations, decrease_every, tuple_count = (operator.index(v) for v in (iterations, decrease_every, tuple_count))
    except TypeError as exc:
        raise ValueError(f"iterations, decrease_every and tuple_count must be integers: {exc}") from None
    thr = float(distance_threshold)
    if not math.isfinite(thr):
        raise ValueError(f"distance_threshold must be finite, got {distance_threshold}")
    if iterations < 1 or decrease_every < 1:
        raise ValueError(f"iterations and decrease_every must be at least 1, got {iterations} and {decrease_every}")
    if not division_factor > 1.0:
        raise ValueError(f"division_factor must exceed 1, got {division_factor}")
    if tuple_count < 0 or not 0.0 <= tuple_scale < 1.0:
        raise ValueError(f"tuple_count must not be negative and tuple_scale must lie in [0, 1), got {tuple_count} and {tuple_scale}")
    if ref_idx.shape[0] != n_matches:
        raise ValueError(f"{n_matches} scan indices for {ref_idx.shape[0]} reference indices")
    if n_matches < 3:
        raise ValueError(f"{n_matches} matches: at least 3 are needed")
    eng = engine or default_engine()
    held: list = []
    matched = _matched_points_on_device(eng, np.asarray(scan_keypoints), scan_idx, np.asarray(ref_keypoints), ref_idx)
    try:
        dsel, rows = None, n_matches
        if tuple_count > 0:
            sel = _tuple_selection(eng, matched, n_matches, tuple_count, tuple_scale, seed, held)
            rows = int(sel.shape[0])
            dsel = eng.empty((rows,), np.int64)
            held.append(dsel)
            dsel.from_host(sel)
        rt, info, trace = eng.fgr_device(matched.a, matched.b, n_matches, thr, iterations, decrease_every, float(division_factor),
                                         sel=dsel, k=rows)
        status = int(info[0])
        record = FgrRecord(status=_STATUS.get(status, str(status)), iterations=int(info[1]), mu=float(info[2]), scale=float(info[3]),
                           rows=rows, trace=np.array(trace, dtype=np.float64).reshape(-1, 4)[:iterations])
        if status == 2:
            raise ValueError("the matched points have no extent (or are not finite)")
        if status != 0 or not np.isfinite(rt).all():
            raise ValueError(f"degenerate after {record.iterations} iterations: the weighted matched points do not determine a "
                             "rigid motion")
        record.inliers = int(eng.ransac_refit_sums(matched.a, matched.b, n_matches, rt, thr)[0])
    finally:
        for h in held:
            h.free()
        matched.free()
    if verbose:
        logging.info(f"{record.iterations} iterations over {rows} rows, mu {record.mu:.3g}: {record.inliers} inliers out of {n_matches}")
    transform = RigidTransform(rt[:9].reshape(3, 3).copy(), rt[9:].copy())
    transform.normalize_rotation()
    return record.inliers / n_matches, transform, record
