"""GPU drop-ins for shot_fpfh.matching (reference matching/__init__.py:1-19)."""
from .consistency import ConsistencyRecord, geometric_consistency_filter
from .filters import FilterFunction, left_median_filter, quantile_filter, threshold_filter
from .fgr import FgrRecord, fast_global_registration
from .match import basic_matching, double_matching_with_rejects, match_descriptors, match_two_nearest, ratio_test_matching
from .ransac import RansacRecord, ransac_on_matches, ransac_prerejective
from .sc2 import SecondOrderRecord, second_order_consistency_filter
from .sc2_registration import Sc2RegistrationRecord, sc2_registration

__all__ = [
    "FilterFunction",
    "threshold_filter",
    "quantile_filter",
    "left_median_filter",
    "match_descriptors",
    "basic_matching",
    "double_matching_with_rejects",
    "match_two_nearest",
    "ratio_test_matching",
    "ransac_on_matches",
    "ransac_prerejective",
    "RansacRecord",
    "fast_global_registration",
    "FgrRecord",
    "geometric_consistency_filter",
    "ConsistencyRecord",
    "second_order_consistency_filter",
    "SecondOrderRecord",
    "sc2_registration",
    "Sc2RegistrationRecord",
]
