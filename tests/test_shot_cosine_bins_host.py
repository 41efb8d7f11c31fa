"""CPU side of the serial SHOT with any number of cosine bins (no GPU needed): the argument checks of
compute_shot_descriptor happen before any device work, the C ABI constants agree with the Python layer, and the fixture
tools/gen_golden_shot_bins.py wrote is consistent with itself."""
import os
import re

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_engine(monkeypatch):
    """Fails the test if anything asks for a device engine."""
    import shot_fpfh_amd.descriptors.shot as shot

    def refuse(*a, **k):
        raise AssertionError("a device engine was requested before the arguments were checked")

    monkeypatch.setattr(shot, "default_engine", refuse)
    return shot


def _call(shot, n, **kw):
    p = np.zeros((4, 3))
    return shot.compute_shot_descriptor(p[:2], p, p, 0.1, n_cosine_bins=n, **kw)


@pytest.mark.parametrize("n", [11.0, 8.5, "8", None, np.float64(4.0)])
def test_a_non_integer_count_raises_type_error(no_engine, n):
    with pytest.raises(TypeError):
        _call(no_engine, n)


@pytest.mark.parametrize("n", [-1, -64, np.int64(-3)])
def test_a_negative_count_raises_value_error(no_engine, n):
    with pytest.raises(ValueError):
        _call(no_engine, n)


@pytest.mark.parametrize("n", [65, 128, 10**6])
def test_a_count_above_the_limit_names_the_limit(no_engine, n):
    with pytest.raises(NotImplementedError, match="64"):
        _call(no_engine, n)


def test_the_other_bin_counts_still_assert(no_engine):
    with pytest.raises(AssertionError):
        _call(no_engine, 8, n_azimuth_bins=4)
    with pytest.raises(AssertionError):
        _call(no_engine, 8, n_radial_bins=3)


@pytest.mark.parametrize("n", [0, 1, 2, 11, 16, 64, np.int32(5)])
def test_a_count_in_range_reaches_the_device(no_engine, n):
    """An accepted count goes on to ask for the engine (refused here): nothing in 0 .. 64 is rejected on the host."""
    with pytest.raises(AssertionError, match="device engine"):
        _call(no_engine, n)


def test_the_header_constants_agree_with_the_python_layer():
    from shot_fpfh_amd import _ffi

    with open(os.path.join(ROOT, "include", "shotfpfh.h")) as f:
        h = f.read()
    assert int(re.search(r"#define SF_SHOT_MAX_COSINE_BINS (\d+)", h).group(1)) == _ffi.MAX_COSINE_BINS == 64
    assert int(re.search(r"#define SF_ERR_BIN_RANGE \((-\d+)\)", h).group(1)) == _ffi.SF_ERR_BIN_RANGE
    codes = [int(c) for c in re.findall(r"#define SF_ERR_\w+ \((-\d+)\)", h)]
    assert len(codes) == len(set(codes))
    assert "sf_shot_serial_bins" in _ffi.SIGNATURES


def test_the_fixture_is_consistent():
    g = load_golden("shot_cosine_bins.npz")
    for case in ("random", "dups", "cluster", "plane_x", "plane_z"):
        kp = g[f"{case}_kp"]
        for n in g[f"{case}_ns"]:
            n = int(n)
            if f"{case}_rows_{n}" in g.files:
                rows, sel = g[f"{case}_rows_{n}"], g[f"{case}_sel_{n}"]
                assert rows.shape == (len(sel), 32 * n) and sel.max() < len(kp)
                norms = np.linalg.norm(rows, axis=1)
                assert np.all((norms == 0) | (np.abs(norms - 1) < 1e-12))
            else:
                assert str(g[f"{case}_raises_{n}"]) in ("IndexError", "ValueError")
    # the reference's IndexError on the +z plane is exactly the even counts (and 0)
    raised = sorted(int(n) for n in g["plane_z_ns"] if f"plane_z_raises_{int(n)}" in g.files)
    assert raised == sorted(n for n in (int(n) for n in g["plane_z_ns"]) if n <= 0 or n % 2 == 0)
    assert g["cluster_counts"].max() > 3072
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "shot_cosine_bins.npz")) < 1 << 20
