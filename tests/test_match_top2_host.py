"""The ratio test's host layer (shot_fpfh_amd.matching: match_two_nearest, ratio_test_matching) on a NumPy stand-in for the
engine's top-2 matcher, and the C ABI declaration of sf_match_top2.  No GPU: tests/test_hip_match_top2.py holds the kernels."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT


def top2_reference(a, b):
    """The two nearest rows of b for each row of a, ranked by (distance, row): the float64 sum of (a - b)^2 taken left to
    right over the descriptor dimension, then sqrt (scipy's loop)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    acc = np.zeros((a.shape[0], b.shape[0]))
    for t in range(a.shape[1]):
        df = a[:, t, None] - b[None, :, t]
        acc += df * df
    dist = np.sqrt(acc)
    order = np.argsort(dist, axis=1, kind="stable")[:, :2]
    idx = np.full((a.shape[0], 2), -1, dtype=np.int64)
    d = np.full((a.shape[0], 2), np.inf)
    idx[:, : order.shape[1]] = order
    d[:, : order.shape[1]] = np.take_along_axis(dist, order, axis=1)
    return idx, d


class StubEngine:
    """Engine.match_top2's contract in NumPy; `canned` replaces the result (for exact boundary values)."""

    def __init__(self, canned=None):
        self.canned, self.calls = canned, 0

    def match_top2(self, a, b):
        self.calls += 1
        if a.shape[0] and not b.shape[0]:
            raise ValueError("empty reference set")
        if self.canned is not None:
            return self.canned[0], self.canned[1], 0
        idx, d = top2_reference(a, b)
        return idx, d, a.shape[0]


def test_two_nearest_skips_zero_rows_and_keeps_original_numbering():
    from shot_fpfh_amd.matching import match_two_nearest

    rng = np.random.default_rng(3)
    scan, ref = rng.random((40, 7)), rng.random((30, 7))
    scan[[0, 5, 39]] = 0.0
    ref[[1, 2, 17, 29]] = 0.0
    rows, idx, dist = match_two_nearest(scan, ref, engine=StubEngine())
    keep_s, keep_r = np.flatnonzero(scan.any(axis=1)), np.flatnonzero(ref.any(axis=1))
    assert np.array_equal(rows, keep_s)
    exp_idx, exp_d = top2_reference(scan[keep_s], ref[keep_r])
    assert np.array_equal(idx, keep_r[exp_idx]) and np.array_equal(dist, exp_d)
    assert not np.isin(idx, [1, 2, 17, 29]).any()


def test_single_reference_row_keeps_minus_one_and_is_kept():
    from shot_fpfh_amd.matching import match_two_nearest, ratio_test_matching

    rng = np.random.default_rng(4)
    scan, ref = rng.random((6, 5)), np.zeros((4, 5))
    ref[2] = rng.random(5)
    rows, idx, dist = match_two_nearest(scan, ref, engine=StubEngine())
    assert np.array_equal(idx[:, 0], np.full(6, 2)) and np.array_equal(idx[:, 1], np.full(6, -1))
    assert np.isinf(dist[:, 1]).all()
    s, r = ratio_test_matching(scan, ref, 0.1, verbose=False, engine=StubEngine())  # d2 = inf keeps every row
    assert np.array_equal(s, np.arange(6)) and np.array_equal(r, np.full(6, 2))


def test_ratio_is_a_strict_float64_less_than():
    from shot_fpfh_amd.matching import ratio_test_matching

    scan, ref = np.ones((4, 3)), np.ones((3, 3))
    idx = np.array([[0, 1], [1, 2], [2, 0], [0, -1]], dtype=np.int64)
    dist = np.array([[0.5, 1.0], [0.5, np.nextafter(1.0, 2.0)], [0.0, 0.0], [3.0, np.inf]])
    s, r = ratio_test_matching(scan, ref, 0.5, verbose=False, engine=StubEngine((idx, dist)))
    # row 0: 0.5 < 0.5 * 1.0 fails; row 1: 0.5 < 0.5 * (1 + ulp) holds; row 2: 0 < 0 fails; row 3: d2 = inf keeps
    assert np.array_equal(s, [1, 3]) and np.array_equal(r, [1, 0])
    s, r = ratio_test_matching(scan, ref, 1.0, verbose=False, engine=StubEngine((idx, dist)))
    assert np.array_equal(s, [0, 1, 3])  # ratio 1 drops exactly the tie


@pytest.mark.parametrize("ratio", [0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")])
def test_invalid_ratio_raises_before_any_work(ratio):
    from shot_fpfh_amd.matching import ratio_test_matching

    eng = StubEngine()
    with pytest.raises(ValueError):
        ratio_test_matching(np.ones((3, 2)), np.ones((3, 2)), ratio, verbose=False, engine=eng)
    assert eng.calls == 0


def test_ratio_logs_the_count(caplog):
    import logging

    from shot_fpfh_amd.matching import ratio_test_matching

    rng = np.random.default_rng(5)
    scan, ref = rng.random((20, 4)), rng.random((25, 4))
    with caplog.at_level(logging.INFO):
        s, _ = ratio_test_matching(scan, ref, 0.8, engine=StubEngine())
    assert f"Kept {s.shape[0]} matches out of 20 descriptors." in caplog.text


def test_pipeline_accepts_ratio(monkeypatch):
    import shot_fpfh_amd.matching.match as match_module
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    monkeypatch.setattr(match_module, "default_engine", lambda: StubEngine())
    rng = np.random.default_rng(6)
    pts = rng.random((10, 3))
    pipe = RegistrationPipeline(scan=pts, scan_normals=pts, ref=pts, ref_normals=pts)
    pipe.scan_descriptors, pipe.ref_descriptors = rng.random((30, 8)), rng.random((40, 8))
    pipe.find_descriptors_matches("ratio", reject_threshold=0.9, threshold_multiplier=10)
    idx, d = top2_reference(pipe.scan_descriptors, pipe.ref_descriptors)
    keep = d[:, 0] < 0.9 * d[:, 1]
    assert np.array_equal(pipe.matches[0], np.flatnonzero(keep)) and np.array_equal(pipe.matches[1], idx[keep, 0])


def test_cli_offers_ratio_matching():
    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    args = mod.parse_args(["scan.ply", "ref.ply", "--radius", "0.1", "--matching", "ratio"])
    assert args.matching == "ratio" and args.reject_threshold == 0.8


def test_sf_match_top2_is_declared_and_exported():
    from shot_fpfh_amd import _ffi

    header = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    assert "int sf_match_top2(sf_ctx *ctx," in header
    assert "sf_match_top2" in _ffi.SIGNATURES
    assert hasattr(_ffi.load(), "sf_match_top2")
