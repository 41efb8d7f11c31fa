"""Descriptor-based registration of two point clouds: keypoints -> descriptors -> matches -> RANSAC -> ICP.

Mirrors the stage methods of the reference's RegistrationPipeline (shot_fpfh/pipeline.py:34-608) -- same method
names, parameters, defaults and stored attributes -- so that a script written against it runs unchanged, with
every stage's heavy step on the MI355X: radius / k-NN search (K1 + K2), SHOT (K4 + K5), FPFH (K6 + K7),
brute-force matching (K8), RANSAC scoring (K9), the ICP nearest-neighbour queries (k-NN kernel).  The plotting
helper of the reference (`analyze_matches` with the 'double' algorithm) is not provided.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Callable, Literal, Optional

import numpy as np
import numpy.typing as npt

from . import keypoint_selection as _ks
from .core import RigidTransform
from .descriptors import (
    ShotMultiprocessor,
    compute_fpfh_descriptor,
    compute_pfh_descriptor,
    compute_spin_image_descriptor,
    compute_usc_descriptor,
)
from .helpers import write_ply
from .icp import icp_generalized, icp_point_to_plane, icp_point_to_point, icp_robust, icp_symmetric, icp_trimmed, nearest_within
from .matching import (
    basic_matching,
    double_matching_with_rejects,
    match_descriptors,
    fast_global_registration,
    geometric_consistency_filter,
    ransac_on_matches,
    ransac_prerejective,
    sc2_registration,
    ratio_test_matching,
    second_order_consistency_filter,
    threshold_filter,
)
from .outlier_removal import remove_radius_outliers, remove_statistical_outliers

__all__ = ["RegistrationPipeline"]


@dataclass
class RegistrationPipeline:
    """State of one registration: the two clouds with unit normals, then whatever the stages have produced.
    A stage leaves an already-filled attribute alone unless `force_recompute` is set (as in the reference)."""

    scan: npt.NDArray[np.float64]
    scan_normals: npt.NDArray[np.float64]
    ref: npt.NDArray[np.float64]
    ref_normals: npt.NDArray[np.float64]

    scan_keypoints: Optional[np.ndarray] = None
    ref_keypoints: Optional[np.ndarray] = None
    scan_descriptors: Optional[npt.NDArray[np.float64]] = None
    ref_descriptors: Optional[npt.NDArray[np.float64]] = None
    matches: Optional[tuple[np.ndarray, np.ndarray]] = None
    # remove_outliers: the indices of the points its last call kept, into the clouds as they stood before that call
    scan_kept: Optional[np.ndarray] = None
    ref_kept: Optional[np.ndarray] = None

    # ---- helpers: run one function on both sides, honouring the cache ---------------------------------
    def _fill(self, attr: str, force: bool, make: Callable[[str], np.ndarray]) -> None:
        for side in ("scan", "ref"):
            if getattr(self, f"{side}_{attr}") is None or force:
                setattr(self, f"{side}_{attr}", make(side))

    def _cloud(self, side: str):
        return getattr(self, side), getattr(self, f"{side}_normals"), getattr(self, f"{side}_keypoints")

    # ---- stage 0: outlier removal (not in the reference) ---------------------------------------------------
    def remove_outliers(
        self,
        method: Literal["statistical", "radius"],
        *,
        nb_neighbors: int = 20,
        std_ratio: float = 2.0,
        radius: float | None = None,
        min_neighbors: int = 2,
        force_recompute: bool = False,
    ) -> None:
        """Filters both clouds and their normals by `remove_statistical_outliers(nb_neighbors, std_ratio)` or
        `remove_radius_outliers(radius, min_neighbors)`; `scan_kept` / `ref_kept` hold the kept indices.  Keypoints, descriptors
        and matches index into the clouds: once any of them is filled the call raises ValueError, unless `force_recompute`,
        which clears them."""
        pick = {
            "statistical": lambda p: remove_statistical_outliers(p, nb_neighbors, std_ratio),
            "radius": lambda p: remove_radius_outliers(p, radius, min_neighbors),
        }.get(method)
        if pick is None:
            raise ValueError("Incorrect outlier removal method.")
        if method == "radius" and radius is None:
            raise ValueError('remove_outliers("radius") needs a radius')
        derived = ("scan_keypoints", "ref_keypoints", "scan_descriptors", "ref_descriptors", "matches")
        filled = [a for a in derived if getattr(self, a) is not None]
        if filled and not force_recompute:
            raise ValueError(f"{', '.join(filled)} index into the clouds: remove the outliers first, or pass force_recompute=True "
                             "to clear them")
        logging.info(f"-- Removing outliers: {method} --")
        kept = {side: pick(getattr(self, side)) for side in ("scan", "ref")}  # (both filters run before anything is replaced)
        for a in derived:
            setattr(self, a, None)
        for side, idx in kept.items():
            total = getattr(self, side).shape[0]
            setattr(self, side, getattr(self, side)[idx])
            setattr(self, f"{side}_normals", getattr(self, f"{side}_normals")[idx])
            setattr(self, f"{side}_kept", idx)
            logging.info(f"{idx.shape[0]} points kept on {side} out of {total}.")

    # ---- stage 1: keypoints (pipeline.py:53-130) ---------------------------------------------------------
    def select_keypoints(
        self,
        selection_algorithm: Literal["random", "iterative", "subsampling", "subsampling_with_density", "iss", "harris"],
        *,
        neighborhood_size: float | None = None,
        min_n_neighbors: int | None = None,
        proportion_picked: float = 0.5,
        force_recompute: bool = False,
        iss_non_max_radius: float | None = None,
        iss_gamma_21: float = 0.975,
        iss_gamma_32: float = 0.975,
        harris_method: str = "harris",
        harris_threshold: float = 0.0,
        harris_non_max_radius: float | None = None,
    ) -> None:
        """"iss" (not in the reference): `neighborhood_size` is the salient radius, `iss_non_max_radius` the suppression
        radius (None: 6 resp. 4 times the cloud's resolution), `min_n_neighbors` the smallest ball when given (else 5).
        "harris" (not in the reference either): Harris 3D on each side's stored normals -- `neighborhood_size` is the radius of
        the tensor (None: 6 times the cloud's resolution), `harris_non_max_radius` that of the suppression (None: the same),
        `harris_method` one of harris / noble / lowe / tomasi / curvature (the last needs no normals), `harris_threshold` the
        smallest response kept, `min_n_neighbors` as for "iss"."""
        if selection_algorithm == "random":
            assert 0 <= proportion_picked <= 1, "Incorrect proportion passed."
        if selection_algorithm == "harris" and harris_method != "curvature":
            for side in ("scan", "ref"):
                if getattr(self, f"{side}_normals") is None:
                    raise ValueError(f'select_keypoints("harris", harris_method="{harris_method}") is computed from the normals '
                                     f'and {side}_normals is None: pass normals, or use harris_method="curvature"')
        min_ball = 5 if min_n_neighbors is None else min_n_neighbors
        pick = {  # (points, normals of a side; only "harris" looks at the normals)
            "random": lambda p, nr: _ks.select_query_indices_randomly(p.shape[0], int(p.shape[0] * proportion_picked)),
            "iterative": lambda p, nr: _ks.select_keypoints_iteratively(p, neighborhood_size),
            "subsampling": lambda p, nr: _ks.select_keypoints_subsampling(p, neighborhood_size),
            "subsampling_with_density": lambda p, nr: _ks.select_keypoints_with_density_threshold(p, neighborhood_size, min_n_neighbors),
            "iss": lambda p, nr: _ks.select_keypoints_iss(p, neighborhood_size, iss_non_max_radius, iss_gamma_21, iss_gamma_32, min_ball),
            "harris": lambda p, nr: _ks.select_keypoints_harris(
                p, None if harris_method == "curvature" else nr, neighborhood_size, harris_non_max_radius, method=harris_method,
                threshold=harris_threshold, min_neighbors=min_ball),
        }.get(selection_algorithm)
        if pick is None:
            raise ValueError("Incorrect keypoint selection algorithm.")
        logging.info(f"-- Selecting keypoints: {selection_algorithm} --")
        self._fill("keypoints", force_recompute, lambda side: pick(getattr(self, side), getattr(self, f"{side}_normals")))
        for side in ("scan", "ref"):
            logging.info(f"{getattr(self, side + '_keypoints').shape[0]} descriptors selected on {side} out of "
                         f"{getattr(self, side).shape[0]} points.")

    # ---- stage 2: descriptors (pipeline.py:132-349) --------------------------------------------------------
    def _shot(self, force: bool, config: dict, call: Callable[[ShotMultiprocessor, np.ndarray, np.ndarray, np.ndarray], np.ndarray]):
        with ShotMultiprocessor(**config) as shot_multiprocessor:
            def make(side):
                points, normals, kp = self._cloud(side)
                return call(shot_multiprocessor, points, points[kp], normals)
            self._fill("descriptors", force, make)

    def compute_shot_descriptor_single_scale(self, radius: float, subsampling_voxel_size: float | None = None,
                                             force_recompute: bool = False, **shot_multiprocessor_config) -> None:
        logging.info("-- Computing single-scale SHOT descriptors --")
        self._shot(force_recompute, shot_multiprocessor_config, lambda sm, pts, kp, nrm: sm.compute_descriptor_single_scale(
            point_cloud=pts, keypoints=kp, normals=nrm, radius=radius, subsampling_voxel_size=subsampling_voxel_size))

    def compute_shot_descriptor_bi_scale(self, local_rf_radius: float, shot_radius: float,
                                         subsampling_voxel_size: float | None = None, force_recompute: bool = False,
                                         **shot_multiprocessor_config) -> None:
        logging.info("-- Computing SHOT descriptors with two scales (local RF and SHOT) --")
        self._shot(force_recompute, shot_multiprocessor_config, lambda sm, pts, kp, nrm: sm.compute_descriptor_bi_scale(
            point_cloud=pts, keypoints=kp, normals=nrm, local_rf_radius=local_rf_radius, shot_radius=shot_radius,
            subsampling_voxel_size=subsampling_voxel_size))

    def compute_shot_descriptor_multiscale(self, radii, voxel_sizes=None, weights=None, force_recompute: bool = False,
                                           **shot_multiprocessor_config) -> None:
        logging.info("-- Computing multi-scale SHOT descriptors --")
        self._shot(force_recompute, shot_multiprocessor_config, lambda sm, pts, kp, nrm: sm.compute_descriptor_multiscale(
            point_cloud=pts, keypoints=kp, normals=nrm, radii=radii, voxel_sizes=voxel_sizes, weights=weights))

    def compute_usc_descriptor(self, radius: float, *, min_radius: float | None = None, density_radius: float | None = None,
                               azimuth_bins: int = 14, elevation_bins: int = 14, radius_bins: int = 10,
                               local_rf_radius: float | None = None, normalize: bool = False, min_neighborhood_size: int = 0,
                               force_recompute: bool = False) -> None:
        """Unique Shape Context rows (`compute_usc_descriptor`, K21; not in the reference) of both clouds' keypoints; the
        normals are not used."""
        logging.info("-- Computing Unique Shape Context descriptors --")

        def make(side):
            points, _, kp = self._cloud(side)
            return compute_usc_descriptor(points, points[kp], radius, min_radius=min_radius, density_radius=density_radius,
                                          azimuth_bins=azimuth_bins, elevation_bins=elevation_bins, radius_bins=radius_bins,
                                          local_rf_radius=local_rf_radius, normalize=normalize,
                                          min_neighborhood_size=min_neighborhood_size)
        self._fill("descriptors", force_recompute, make)

    def compute_pfh_descriptor(self, radius: float, n_bins: int = 5, force_recompute: bool = False) -> None:
        """Point Feature Histogram rows (`compute_pfh_descriptor`, K22; not in the reference) of both clouds' keypoints."""
        logging.info("-- Computing Point Feature Histogram descriptors --")

        def make(side):
            points, normals, kp = self._cloud(side)
            return compute_pfh_descriptor(kp, points, normals, radius, n_bins)
        self._fill("descriptors", force_recompute, make)

    def compute_spin_image_descriptor(self, radius: float, image_width: int = 8, signed: bool = False, *,
                                      min_cos: float | None = None, normalize: bool = False, min_neighborhood_size: int = 0,
                                      force_recompute: bool = False) -> None:
        """Spin images (`compute_spin_image_descriptor`, K24; not in the reference) of both clouds' keypoints about their own
        normals.  The default here is the UNSIGNED image (signed=False, rows of (W + 1)^2), because a pipeline's normals usually
        come from compute_normals, whose sign is arbitrary; the function's own default is PCL's signed image, for consistently
        oriented normals.  min_cos, normalize and min_neighborhood_size reach the descriptor through this method only:
        compute_descriptors(descriptor_choice="spin") passes the radius, spin_width and spin_signed and leaves these three at
        their defaults here (its own normalize and min_neighborhood_size are SHOT's, with SHOT's defaults, as for "usc" and "pfh")."""
        logging.info("-- Computing spin image descriptors --")

        def make(side):
            points, normals, kp = self._cloud(side)
            return compute_spin_image_descriptor(kp, points, normals, radius, image_width, signed_beta=signed, min_cos=min_cos,
                                                 normalize=normalize, min_neighborhood_size=min_neighborhood_size)
        self._fill("descriptors", force_recompute, make)

    def compute_descriptors(
        self,
        radius: float,
        descriptor_choice: Literal["fpfh", "shot_single_scale", "shot_bi_scale", "shot_multiscale", "usc", "pfh", "spin"] = "shot_single_scale",
        fpfh_n_bins: int = 5,
        phi: float = 3.0,
        rho: float = 10.0,
        n_scales: int = 2,
        subsample_support: bool = True,
        normalize: bool = True,
        share_local_rfs: bool = True,
        min_neighborhood_size: int = 100,
        n_procs: int = 8,
        disable_progress_bars: bool = False,
        verbose: bool = True,
        force_recompute: bool = False,
        *,
        pfh_n_bins: int = 5,
        spin_width: int = 8,
        spin_signed: bool = False,
    ) -> None:
        shot_config = dict(normalize=normalize, share_local_rfs=share_local_rfs, min_neighborhood_size=min_neighborhood_size,
                           n_procs=n_procs, disable_progress_bar=disable_progress_bars, verbose=verbose)
        voxel = radius / rho if subsample_support else None
        if descriptor_choice == "shot_single_scale":
            self.compute_shot_descriptor_single_scale(radius=radius, subsampling_voxel_size=voxel,
                                                      force_recompute=force_recompute, **shot_config)
        elif descriptor_choice == "shot_bi_scale":
            self.compute_shot_descriptor_bi_scale(local_rf_radius=radius, shot_radius=radius * phi, subsampling_voxel_size=voxel,
                                                  force_recompute=force_recompute, **shot_config)
        elif descriptor_choice in ("shot_multi_scale", "shot_multiscale"):  # the reference tests the first spelling (:321)
            scales = radius * phi ** np.arange(n_scales)
            self.compute_shot_descriptor_multiscale(radii=scales, voxel_sizes=scales / rho, force_recompute=force_recompute,
                                                    **shot_config)
        elif descriptor_choice == "fpfh":
            def make(side):
                points, normals, kp = self._cloud(side)
                return compute_fpfh_descriptor(kp, points, normals, radius=radius, n_bins=fpfh_n_bins,
                                               disable_progress_bars=disable_progress_bars, verbose=verbose)
            self._fill("descriptors", force_recompute, make)
        elif descriptor_choice == "usc":  # (its own parameters at their defaults: compute_usc_descriptor takes them)
            self.compute_usc_descriptor(radius, force_recompute=force_recompute)
        elif descriptor_choice == "pfh":
            self.compute_pfh_descriptor(radius, n_bins=pfh_n_bins, force_recompute=force_recompute)
        elif descriptor_choice == "spin":  # (unsigned by default; normalize / min_neighborhood_size above are SHOT's and not passed on)
            self.compute_spin_image_descriptor(radius, image_width=spin_width, signed=spin_signed, force_recompute=force_recompute)
        else:
            raise ValueError("Incorrect descriptor choice")

    # ---- stage 3: matching (pipeline.py:351-412) -------------------------------------------------------------
    def find_descriptors_matches(
        self,
        matching_algorithm: Literal["simple", "double", "threshold", "ratio"],
        *,
        reject_threshold: float,
        threshold_multiplier: float,
        debug_mode: bool = False,
        force_recompute: bool = False,
    ) -> None:
        run = {
            "simple": lambda: basic_matching(self.scan_descriptors, self.ref_descriptors),
            "double": lambda: double_matching_with_rejects(self.scan_descriptors, self.ref_descriptors, reject_threshold),
            "threshold": lambda: match_descriptors(self.scan_descriptors, self.ref_descriptors, threshold_filter,
                                                   threshold_multiplier=threshold_multiplier),
            # Lowe's ratio test with reject_threshold as the ratio (what "double" is meant to do; the reference's raises)
            "ratio": lambda: ratio_test_matching(self.scan_descriptors, self.ref_descriptors, reject_threshold),
        }.get(matching_algorithm)
        if run is None:
            raise ValueError("Incorrect matching algorithm selection.")
        logging.info(f"-- Matching descriptors: {matching_algorithm} --")
        if self.matches is None or force_recompute:
            self.matches = run()
        if debug_mode:
            gap = np.linalg.norm(self.scan_descriptors[self.matches[0]] - self.ref_descriptors[self.matches[1]], axis=0)
            logging.info(f"Maximum distance between the descriptors matched: {gap.max(initial=0):.2f}")

    def filter_matches_by_consistency(self, distance_threshold: float, min_edge: float | None = None,
                                      group_share: float = 0.4) -> None:
        """Keeps the matches that agree with each other on lengths within `distance_threshold` (`geometric_consistency_filter`,
        not in the reference): `self.matches` is replaced by the kept ones, in their order."""
        logging.info("-- Filtering the matches by geometric consistency --")
        total = self.matches[0].shape[0]
        scan_kept, ref_kept, record = geometric_consistency_filter(
            *self.matches, self.scan[self.scan_keypoints], self.ref[self.ref_keypoints], distance_threshold=distance_threshold,
            min_edge=min_edge, group_share=group_share)
        self.matches = (scan_kept, ref_kept)
        logging.info(f"{scan_kept.shape[0]} matches kept out of {total} ({record.status}, group of {record.group_size})")

    def filter_matches_by_second_order_consistency(self, distance_threshold: float, min_edge: float | None = None,
                                                   group_share: float = 0.5) -> None:
        """Keeps the matches that `second_order_consistency_filter` (not in the reference) selects -- the group around the match
        that lies in the most triangles of the compatibility graph, which still finds the true matches where they are a per
        cent of the set: `self.matches` is replaced by the kept ones, in their order."""
        logging.info("-- Filtering the matches by second-order consistency --")
        total = self.matches[0].shape[0]
        scan_kept, ref_kept, record = second_order_consistency_filter(
            *self.matches, self.scan[self.scan_keypoints], self.ref[self.ref_keypoints], distance_threshold=distance_threshold,
            min_edge=min_edge, group_share=group_share)
        self.matches = (scan_kept, ref_kept)
        logging.info(f"{scan_kept.shape[0]} matches kept out of {total} ({record.status}, group of {record.group_size})")

    # ---- stage 4: coarse registration (pipeline.py:445-486) ----------------------------------------------------
    def run_ransac(self, *, n_draws: int = 10000, draw_size: int = 4, max_inliers_distance: float = 2,
                   exact_transformation: RigidTransform | None = None,
                   disable_progress_bar: bool = False, method: Literal["reference", "prerejective", "fgr", "sc2"] = "reference",
                   edge_similarity: float = 0.9, refit_iterations: int = 2, fgr_iterations: int = 64,
                   fgr_tuple_count: int = 0, sc2_seeds: int = 256) -> tuple[RigidTransform, float]:
        """method="reference": the reference's RANSAC.  method="prerejective": draws that fail the edge-length test at
        `edge_similarity` are dropped unscored and the winner is refitted over its inliers `refit_iterations` times (three
        points determine the fit: pass draw_size=3 there, the default of `ransac_prerejective` itself).  method="fgr": fast global
        registration, which draws nothing -- `max_inliers_distance` is its threshold, `n_draws` and `draw_size` are ignored,
        `fgr_iterations` Gauss-Newton steps are taken over all matches (or over `fgr_tuple_count` tuples of them).
        method="sc2": `sc2_registration`, one fit per second-order seed -- `max_inliers_distance` is its threshold, `sc2_seeds`
        the number of seeds, the winner is refitted `refit_iterations` times, `n_draws` and `draw_size` are ignored."""
        logging.info(" -- Aligning the point clouds by RANSAC-ing the matches --")
        if method == "reference":
            inliers_ratio, transformation = ransac_on_matches(
                *self.matches, self.scan[self.scan_keypoints], self.ref[self.ref_keypoints], n_draws=n_draws,
                draw_size=draw_size, distance_threshold=max_inliers_distance,
                disable_progress_bar=disable_progress_bar)
        elif method == "prerejective":
            inliers_ratio, transformation, record = ransac_prerejective(
                *self.matches, self.scan[self.scan_keypoints], self.ref[self.ref_keypoints], n_draws=n_draws,
                draw_size=draw_size, distance_threshold=max_inliers_distance,
                edge_similarity=edge_similarity, refit_iterations=refit_iterations)
            logging.info(f"{record.n_scored} of {record.n_draws} draws scored, inliers {record.winner_inliers} -> {record.refit_inliers}")
        elif method == "fgr":
            inliers_ratio, transformation, fgr_record = fast_global_registration(
                *self.matches, self.scan[self.scan_keypoints], self.ref[self.ref_keypoints],
                distance_threshold=max_inliers_distance, iterations=fgr_iterations, tuple_count=fgr_tuple_count)
            logging.info(f"{fgr_record.iterations} iterations over {fgr_record.rows} rows, {fgr_record.inliers} inliers")
        elif method == "sc2":
            inliers_ratio, transformation, sc2_record = sc2_registration(
                *self.matches, self.scan[self.scan_keypoints], self.ref[self.ref_keypoints],
                distance_threshold=max_inliers_distance, n_seeds=sc2_seeds, refit_iterations=refit_iterations)
            logging.info(f"{sc2_record.n_scored} of {sc2_record.seeds.shape[0]} seeds scored, inliers {sc2_record.winner_inliers} -> "
                         f"{sc2_record.refit_inliers}")
        else:
            raise ValueError("Incorrect RANSAC method selected.")
        if exact_transformation is not None:
            cosine = (np.trace(exact_transformation.rotation @ transformation.rotation.T) - 1) / 2
            logging.info(f"Norm of the angle between the two rotations: {abs(np.arccos(cosine)):.2f}\n"
                         f"Norm of the difference between the two translation: "
                         f"{np.linalg.norm(exact_transformation.translation - transformation.translation):.2f}")
        return transformation, inliers_ratio

    # ---- stage 5: fine registration (pipeline.py:488-542) ---------------------------------------------------------
    def run_icp(self, icp_type: Literal["point_to_point", "point_to_plane", "generalized", "symmetric"], transformation_init: RigidTransform, *,
                d_max: float, voxel_size: float = 0.2, max_iter: int = 30, rms_threshold: float = 1e-2,
                disable_progress_bar: bool = False, gicp_neighbors: int = 20,
                gicp_epsilon: float = 1e-3, robust_loss: Optional[str] = None, robust_scale: Optional[float] = None,
                robust_scale_start: Optional[float] = None, trim_overlap: Optional[float] = None,
                trim_anneal_iterations: int = 10) -> tuple[RigidTransform, float, bool]:
        """"generalized" (K16, no counterpart in the reference): plane-to-plane ICP with the pipeline's reference normals and
        scan normals from `gicp_neighbors` neighbours of the full scan (the scan's stored normals when it has them).
        `robust_loss` ("huber", "cauchy", "geman_mcclure", "tukey", "none"; K17) runs the chosen `icp_type` through `icp_robust` with
        the loss's scale `robust_scale`, annealed from `robust_scale_start` (`d_max` unless given); None is the call of before.
        `trim_overlap` (K18) runs it through `icp_trimmed`, fitting only that share of the pairs within `d_max`, annealed from 1 over
        `trim_anneal_iterations` iterations; it combines with `robust_loss`.  None is the call of before.
        "symmetric" (K19, no counterpart in the reference): `icp_symmetric`, the residual along the mean of both clouds' normals, with
        the normals treated as "generalized" treats them (`gicp_neighbors` for the missing ones); it takes `robust_loss` and
        `trim_overlap` itself."""
        if icp_type == "symmetric":
            if robust_loss not in (None, "none") and robust_scale is None:
                raise ValueError(f"robust_loss={robust_loss!r} needs robust_scale, the loss's scale in the residual's unit")
            if robust_loss is None and (robust_scale is not None or robust_scale_start is not None):
                raise ValueError("robust_scale and robust_scale_start need a robust_loss")
            return icp_symmetric(self.scan, self.ref, transformation_init, d_max, scan_normals=self.scan_normals,
                                 ref_normals=self.ref_normals, k_normals=gicp_neighbors, loss=robust_loss or "none",
                                 scale=robust_scale, scale_start=robust_scale_start,
                                 overlap=1.0 if trim_overlap is None else trim_overlap, anneal_iterations=trim_anneal_iterations,
                                 voxel_size=voxel_size, max_iter=max_iter, rms_threshold=rms_threshold)
        if trim_overlap is not None:
            if robust_loss not in (None, "none") and robust_scale is None:
                raise ValueError(f"robust_loss={robust_loss!r} needs robust_scale, the loss's scale in the residual's unit")
            if robust_loss is None and (robust_scale is not None or robust_scale_start is not None):
                raise ValueError("robust_scale and robust_scale_start need a robust_loss")
            return icp_trimmed(self.scan, self.ref, transformation_init, d_max, overlap=trim_overlap,
                               anneal_iterations=trim_anneal_iterations, mode=icp_type, loss=robust_loss or "none", scale=robust_scale,
                               scale_start=robust_scale_start, ref_normals=self.ref_normals,
                               scan_normals=self.scan_normals if icp_type == "generalized" else None, k_normals=gicp_neighbors,
                               epsilon=gicp_epsilon, voxel_size=voxel_size, max_iter=max_iter, rms_threshold=rms_threshold)
        if robust_loss is not None:
            if robust_scale is None:
                raise ValueError(f"robust_loss={robust_loss!r} needs robust_scale, the loss's scale in the residual's unit")
            return icp_robust(self.scan, self.ref, transformation_init, d_max, mode=icp_type, loss=robust_loss, scale=robust_scale,
                              scale_start=robust_scale_start, ref_normals=self.ref_normals,
                              scan_normals=self.scan_normals if icp_type == "generalized" else None, k_normals=gicp_neighbors,
                              epsilon=gicp_epsilon, voxel_size=voxel_size, max_iter=max_iter, rms_threshold=rms_threshold)
        if robust_scale is not None or robust_scale_start is not None:
            raise ValueError("robust_scale and robust_scale_start need a robust_loss")
        common = dict(d_max=d_max, voxel_size=voxel_size, max_iter=max_iter, rms_threshold=rms_threshold,
                      disable_progress_bar=disable_progress_bar)
        if icp_type == "point_to_point":
            return icp_point_to_point(self.scan, self.ref, transformation_init, **common)
        if icp_type == "point_to_plane":
            return icp_point_to_plane(self.scan, self.ref, self.ref_normals, transformation_init, **common)
        if icp_type == "generalized":
            return icp_generalized(self.scan, self.ref, transformation_init, d_max, scan_normals=self.scan_normals,
                                   ref_normals=self.ref_normals, k_normals=gicp_neighbors, epsilon=gicp_epsilon,
                                   voxel_size=voxel_size, max_iter=max_iter, rms_threshold=rms_threshold)
        raise ValueError("Incorrect ICP type selected.")

    # ---- evaluation / output (pipeline.py:544-608) ---------------------------------------------------------------------
    def compute_metrics_post_icp(self, transformation_icp: RigidTransform, distance_threshold: float) -> tuple[float, float]:
        """(overlap of the aligned scan with ref, ratio of aligned scan keypoints that have a ref keypoint within
        the threshold)."""
        aligned = transformation_icp[self.scan]
        return (nearest_within(aligned, self.ref, distance_threshold) / aligned.shape[0],
                nearest_within(aligned[self.scan_keypoints], self.ref[self.ref_keypoints], distance_threshold)
                / self.scan_keypoints.shape[0])

    def write_alignments(self, *args: tuple[str, RigidTransform]) -> None:
        """One PLY per (file_name, transform): the transformed scan stacked on ref, with an `is_scan` column."""
        is_scan = np.hstack((np.ones(self.scan.shape[0], dtype=bool), np.zeros(self.ref.shape[0], dtype=bool)))[:, None]
        for file_name, transform in args:
            write_ply(file_name, [np.hstack((np.vstack((transform[self.scan], self.ref)), is_scan))], ["x", "y", "z", "is_scan"])
