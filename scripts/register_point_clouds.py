#!/usr/bin/env python3
"""Register two binary-PLY point clouds end to end on one MI355X (the counterpart of the reference's
scripts/register_point_clouds.py, with plain argparse flags instead of its YAML configuration layer).

    python scripts/register_point_clouds.py scan.ply ref.ply --radius 0.05 --descriptor shot_single_scale \
        --keypoints subsampling --keypoint-size 0.03 --ransac-threshold 0.01 --icp point_to_plane --icp-dmax 0.05

Stages: read PLY (optionally --outliers: stray points removed; + PCA normals, k nearest neighbours) -> keypoints -> SHOT / FPFH / USC / PFH descriptors -> matching ->
RANSAC -> ICP -> overlap metrics; optionally writes the aligned pair as PLY.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shot_fpfh_amd import compute_normals  # noqa: E402
from shot_fpfh_amd.helpers import get_data, read_ply  # noqa: E402
from shot_fpfh_amd.outlier_removal import remove_radius_outliers, remove_statistical_outliers  # noqa: E402
from shot_fpfh_amd.pipeline import RegistrationPipeline  # noqa: E402


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("scan"), p.add_argument("ref")
    p.add_argument("--normals-k", type=int, default=30, help="neighbours for the PCA normals (reference default 30)")
    p.add_argument("--keep-stored-normals", action="store_true", help="use the file's normals instead of recomputing them")
    p.add_argument("--outliers", default="none", choices=["none", "statistical", "radius"],
                   help="remove stray points from both clouds right after loading, before the normals are computed: statistical "
                        "(mean distance to --outlier-neighbors neighbours above mean + --outlier-std-ratio sigma) or radius (fewer "
                        "than --outlier-min-neighbors other points within --outlier-radius)")
    p.add_argument("--outlier-neighbors", type=int, default=20, metavar="K")
    p.add_argument("--outlier-std-ratio", type=float, default=2.0, metavar="S")
    p.add_argument("--outlier-radius", type=float, default=None, metavar="R")
    p.add_argument("--outlier-min-neighbors", type=int, default=2, metavar="N")
    p.add_argument("--keypoints", default="subsampling", choices=["random", "iterative", "subsampling", "subsampling_with_density", "iss", "harris"],
                   help="iss: Intrinsic Shape Signatures on the positions; harris: Harris 3D on the normals (corners and creases)")
    p.add_argument("--keypoint-size", type=float, default=None,
                   help="sphere / voxel size of the keypoint selection (iss: the salient radius, harris: the radius of the tensor; "
                        "default for both 6 x the cloud's resolution)")
    p.add_argument("--iss-non-max-radius", type=float, default=None, help="iss: suppression radius (default 4 x the cloud's resolution)")
    p.add_argument("--iss-gamma21", type=float, default=0.975), p.add_argument("--iss-gamma32", type=float, default=0.975)
    p.add_argument("--harris-method", default="harris", choices=["harris", "noble", "lowe", "tomasi", "curvature"],
                   help="harris: the response -- 0.04 + det - 0.04 tr^2, det / tr, det / tr^2, the smallest eigenvalue of the normals' "
                        "tensor, or the surface variation of the positions (needs no normals)")
    p.add_argument("--harris-threshold", type=float, default=0.0, metavar="T", help="harris: the smallest response kept (not negative)")
    p.add_argument("--harris-non-max-radius", type=float, default=None, metavar="R", help="harris: suppression radius (default --keypoint-size)")
    p.add_argument("--min-n-neighbors", type=int, default=None)
    p.add_argument("--proportion", type=float, default=0.5, help="share of points kept by --keypoints random")
    p.add_argument("--descriptor", default="shot_single_scale", choices=["fpfh", "shot_single_scale", "shot_bi_scale", "shot_multiscale", "usc", "pfh", "spin"],
                   help="usc: Unique Shape Context at --radius, 14 x 14 x 10 bins, no normals used; "
                        "pfh: Point Feature Histograms at --radius, every pair of a ball's points (quadratic in the ball size); "
                        "spin: spin images about each keypoint's normal at --radius, no local reference frame")
    p.add_argument("--usc-min-radius", type=float, default=None, metavar="R0", help="--descriptor usc: the first radial edge (default --radius / 10)")
    p.add_argument("--usc-density-radius", type=float, default=None, metavar="RD",
                   help="--descriptor usc: the ball whose population weighs a neighbour down (default --radius / 5)")
    p.add_argument("--radius", type=float, required=True)
    p.add_argument("--fpfh-bins", type=int, default=5)
    p.add_argument("--pfh-bins", type=int, default=5, metavar="S", help="--descriptor pfh: bins per angle, 1 .. 16 (rows of S^3)")
    p.add_argument("--spin-width", type=int, default=8, metavar="W", help="--descriptor spin: bins per image side, 1 .. 44")
    p.add_argument("--spin-signed", action="store_true",
                   help="--descriptor spin: keep the sign of the height along the normal (rows of (W + 1)(2 W + 1); needs consistently "
                        "oriented normals).  Default: the image folded over the tangent plane, (W + 1)^2, blind to the normals' signs")
    p.add_argument("--phi", type=float, default=3.0), p.add_argument("--rho", type=float, default=10.0)
    p.add_argument("--n-scales", type=int, default=2)
    p.add_argument("--no-support-subsampling", action="store_true")
    p.add_argument("--min-neighborhood-size", type=int, default=100)
    p.add_argument("--matching", default="simple", choices=["simple", "double", "threshold", "ratio"])
    p.add_argument("--reject-threshold", type=float, default=0.8), p.add_argument("--threshold-multiplier", type=float, default=10)
    consistency = p.add_mutually_exclusive_group()
    consistency.add_argument("--consistency", type=float, default=None, metavar="EPS",
                             help="keep only the matches whose pairwise lengths agree within EPS on both sides before the registration (default: off)")
    consistency.add_argument("--consistency-sc2", type=float, default=None, metavar="EPS",
                             help="the same test, the group chosen by second-order consistency (triangles of the compatibility graph): "
                                  "for sets with a few per cent of true matches, at most 32768 of them (default: off)")
    p.add_argument("--ransac-draws", type=int, default=10000), p.add_argument("--ransac-draw-size", type=int, default=None,
                                                                            help="default 4 (reference), 3 (prerejective)")
    p.add_argument("--ransac", default="reference", choices=["reference", "prerejective", "fgr", "sc2"],
                   help="prerejective: drop draws whose edge lengths disagree before scoring, refit the winner over its inliers; "
                        "fgr: fast global registration, no draws (--ransac-draws and --ransac-draw-size are ignored); "
                        "sc2: one fit per second-order seed, ranked by inliers, at most 32768 matches (no draws either; may be "
                        "combined with --consistency or --consistency-sc2, which then thin the matches first)")
    p.add_argument("--sc2-seeds", type=int, default=256, metavar="N", help="--ransac sc2: the number of seeds, 1 .. 1024")
    p.add_argument("--ransac-edge-similarity", type=float, default=0.9), p.add_argument("--ransac-refit", type=int, default=2)
    p.add_argument("--ransac-threshold", type=float, default=1.0)
    p.add_argument("--fgr-iterations", type=int, default=64), p.add_argument("--fgr-tuples", type=int, default=0)
    p.add_argument("--icp", default="point_to_plane", choices=["point_to_point", "point_to_plane", "generalized", "symmetric", "none"],
                   help="generalized: plane-to-plane ICP, every pair weighted by the local surface of both clouds; "
                        "symmetric: point-to-plane along the mean of both clouds' normals")
    p.add_argument("--gicp-neighbors", type=int, default=20, metavar="K",
                   help="--icp generalized, symmetric: neighbours of a normal that the clouds do not bring along")
    p.add_argument("--gicp-epsilon", type=float, default=1e-3, metavar="EPS",
                   help="--icp generalized: a point's covariance along its normal, in (0, 1]")
    p.add_argument("--icp-loss", default=None, choices=["none", "huber", "cauchy", "geman_mcclure", "tukey"],
                   help="robust loss of the ICP stage: pairs within --icp-dmax are weighted by their residual (needs --icp-loss-scale)")
    p.add_argument("--icp-loss-scale", type=float, default=None, metavar="K",
                   help="--icp-loss: the loss's scale in the residual's unit, a few sigma of the noise")
    p.add_argument("--icp-loss-scale-start", type=float, default=None, metavar="K0",
                   help="--icp-loss: the scale of the first iteration, divided by 1.4 per iteration down to K (default: --icp-dmax)")
    p.add_argument("--icp-overlap", type=float, default=None, metavar="X",
                   help="trimmed ICP: fit only the best-fitting share X, in (0, 1], of the pairs within --icp-dmax -- roughly how much "
                        "of the scan the reference also sees (combines with --icp-loss)")
    p.add_argument("--icp-overlap-anneal", type=int, default=10, metavar="N",
                   help="--icp-overlap: the share comes down from 1 to X over the first N iterations (0: X throughout)")
    p.add_argument("--icp-dmax", type=float, default=0.5), p.add_argument("--icp-voxel", type=float, default=0.2)
    p.add_argument("--icp-max-iter", type=int, default=50), p.add_argument("--icp-rms", type=float, default=1e-3)
    p.add_argument("--metric-threshold", type=float, default=0.1)
    p.add_argument("--write", default=None, help="basename for the aligned clouds (<name>_ransac.ply, <name>_icp.ply)")
    args = p.parse_args(argv)
    if args.outliers == "radius" and args.outlier_radius is None:
        p.error("--outliers radius needs --outlier-radius")
    if args.descriptor != "usc" and (args.usc_min_radius is not None or args.usc_density_radius is not None):
        p.error("--usc-min-radius and --usc-density-radius need --descriptor usc")
    if args.harris_threshold < 0.0:
        p.error("--harris-threshold must not be negative")
    if args.icp_loss is not None and args.icp_loss_scale is None:
        p.error("--icp-loss needs --icp-loss-scale")
    if args.icp_loss is None and (args.icp_loss_scale is not None or args.icp_loss_scale_start is not None):
        p.error("--icp-loss-scale and --icp-loss-scale-start need --icp-loss")
    if args.icp_overlap is not None and not 0.0 < args.icp_overlap <= 1.0:
        p.error("--icp-overlap must lie in (0, 1]")
    if args.icp_overlap_anneal < 0:
        p.error("--icp-overlap-anneal must not be negative")
    return args


def load_filtered(path: str, args: argparse.Namespace):
    """(points, normals, kept) of a PLY cloud with --outliers on: what get_data does, with the filter between the file and the
    normals -- the stored normals of the kept points are used as they are (--keep-stored-normals) or orient the ones
    computed on the filtered cloud."""
    data = read_ply(path)
    points = np.vstack((data["x"], data["y"], data["z"])).T
    stored = next((names for names in (("nx", "ny", "nz"), ("n_x", "n_y", "n_z")) if names[0] in data.dtype.fields), None)
    if args.outliers == "statistical":
        kept = remove_statistical_outliers(points, args.outlier_neighbors, args.outlier_std_ratio)
    else:
        kept = remove_radius_outliers(points, args.outlier_radius, args.outlier_min_neighbors)
    logging.info(f"{kept.shape[0]} points kept out of {points.shape[0]} in {path} (--outliers {args.outliers})")
    points = np.ascontiguousarray(points[kept])
    pre = None if stored is None else np.vstack([data[name] for name in stored]).T[kept]
    if pre is not None and args.keep_stored_normals:
        return points, pre, kept
    extra = {} if pre is None else {"pre_computed_normals": pre}
    return points, compute_normals(points, points, k=args.normals_k, radius=None, **extra), kept


def main(argv=None) -> int:
    args = parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    t0 = time.perf_counter()
    if args.outliers == "none":
        load = dict(recompute_normals=not args.keep_stored_normals, k=args.normals_k, normals_computation_callback=compute_normals)
        scan, scan_normals = get_data(args.scan, **load)
        ref, ref_normals = get_data(args.ref, **load)
        pipe = RegistrationPipeline(scan=scan, scan_normals=scan_normals, ref=ref, ref_normals=ref_normals)
    else:
        scan, scan_normals, scan_kept = load_filtered(args.scan, args)
        ref, ref_normals, ref_kept = load_filtered(args.ref, args)
        pipe = RegistrationPipeline(scan=scan, scan_normals=scan_normals, ref=ref, ref_normals=ref_normals, scan_kept=scan_kept,
                                    ref_kept=ref_kept)
    pipe.select_keypoints(args.keypoints, neighborhood_size=args.keypoint_size, min_n_neighbors=args.min_n_neighbors,
                          proportion_picked=args.proportion, iss_non_max_radius=args.iss_non_max_radius,
                          iss_gamma_21=args.iss_gamma21, iss_gamma_32=args.iss_gamma32, harris_method=args.harris_method,
                          harris_threshold=args.harris_threshold, harris_non_max_radius=args.harris_non_max_radius)
    if args.descriptor == "usc":
        pipe.compute_usc_descriptor(args.radius, min_radius=args.usc_min_radius, density_radius=args.usc_density_radius)
    else:
        pipe.compute_descriptors(radius=args.radius, descriptor_choice=args.descriptor, fpfh_n_bins=args.fpfh_bins, pfh_n_bins=args.pfh_bins,
                                 spin_width=args.spin_width, spin_signed=args.spin_signed,
                                 phi=args.phi, rho=args.rho, n_scales=args.n_scales, subsample_support=not args.no_support_subsampling,
                                 min_neighborhood_size=args.min_neighborhood_size, disable_progress_bars=True, verbose=False)
    pipe.find_descriptors_matches(args.matching, reject_threshold=args.reject_threshold,
                                  threshold_multiplier=args.threshold_multiplier)
    logging.info(f"{pipe.matches[0].shape[0]} matches")
    if args.consistency is not None:
        pipe.filter_matches_by_consistency(args.consistency)
    if args.consistency_sc2 is not None:
        pipe.filter_matches_by_second_order_consistency(args.consistency_sc2)
    draw_size = args.ransac_draw_size or (3 if args.ransac == "prerejective" else 4)
    transformation, inliers_ratio = pipe.run_ransac(n_draws=args.ransac_draws, draw_size=draw_size,
                                                    max_inliers_distance=args.ransac_threshold, disable_progress_bar=True,
                                                    method=args.ransac, edge_similarity=args.ransac_edge_similarity,
                                                    refit_iterations=args.ransac_refit, fgr_iterations=args.fgr_iterations,
                                                    fgr_tuple_count=args.fgr_tuples, sc2_seeds=args.sc2_seeds)
    logging.info(f"RANSAC inlier ratio {inliers_ratio:.3f}\n{transformation}")
    outputs = [(f"{args.write}_ransac.ply", transformation)] if args.write else []
    if args.icp != "none":
        transformation, rms, converged = pipe.run_icp(args.icp, transformation, d_max=args.icp_dmax, voxel_size=args.icp_voxel,
                                                       max_iter=args.icp_max_iter, rms_threshold=args.icp_rms,
                                                       disable_progress_bar=True, gicp_neighbors=args.gicp_neighbors,
                                                       gicp_epsilon=args.gicp_epsilon, robust_loss=args.icp_loss,
                                                       robust_scale=args.icp_loss_scale, robust_scale_start=args.icp_loss_scale_start,
                                                       trim_overlap=args.icp_overlap,
                                                       trim_anneal_iterations=args.icp_overlap_anneal)
        logging.info(f"ICP rms {rms:.3e}, converged: {bool(converged)}\n{transformation}")
        if args.write:
            outputs.append((f"{args.write}_icp.ply", transformation))
    overlap, keypoint_inliers = pipe.compute_metrics_post_icp(transformation, args.metric_threshold)
    logging.info(f"overlap {overlap:.3f}, keypoint inlier ratio {keypoint_inliers:.3f}, total {time.perf_counter() - t0:.2f} s")
    if outputs:
        pipe.write_alignments(*outputs)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
