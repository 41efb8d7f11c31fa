"""GPU drop-ins for shot_fpfh.descriptors (reference descriptors/__init__.py:1-17): the three hot-path
exports (compute_fpfh_descriptor, compute_normals, ShotMultiprocessor), the PCA feature helpers that
share kernel K3 with the normals, Unique Shape Context (compute_usc_descriptor, K21), Point Feature Histograms
(compute_pfh_descriptor, K22) and spin images (compute_spin_image_descriptor, K24): none of the three is in the reference."""
from .fpfh import compute_fpfh_descriptor
from .normals import compute_normals
from .pca_features import (
    compute_local_pca_with_moments,
    compute_pca_based_basic_features,
    compute_pca_based_features,
    compute_sphericity,
)
from .pfh import compute_pfh_descriptor
from .shot import ShotMultiprocessor
from .spin import compute_spin_image_descriptor
from .usc import compute_usc_descriptor

__all__ = [
    "compute_fpfh_descriptor",
    "compute_normals",
    "compute_pca_based_basic_features",
    "compute_pca_based_features",
    "compute_sphericity",
    "compute_local_pca_with_moments",
    "ShotMultiprocessor",
    "compute_usc_descriptor",
    "compute_pfh_descriptor",
    "compute_spin_image_descriptor",
]
