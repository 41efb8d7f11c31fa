"""Spin images (K24) without a GPU: the statement tests/spin_numpy.py against closed forms and the unquantised bilinear image,
sf_spin_scale (host only) against its formula, the public function's argument checks, the names, the header, the registers."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import spin_numpy as S
from shot_fpfh_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


# ---- the scale --------------------------------------------------------------------------------------------------------------------
def test_scale_equals_its_formula_bit_for_bit():
    radii = [0.03, 0.1, 1.0, 1.0 / 3.0, 2.5e-4, 7.0, 1e6, np.sqrt(2.0), 8 * np.sqrt(2.0) / 256, np.nextafter(1.0, 2.0), 5e-324, 1e300]
    for R in radii:
        for W in range(1, S.MAX_WIDTH + 1):
            with np.errstate(over="ignore"):  # (the subnormal radius: inf on both sides)
                want = (np.float64(W) * np.sqrt(np.float64(2.0))) / np.float64(R)
            assert bits(S.scale(R, W)) == bits(want), (R, W)
    for k in (0, 3, 10):  # the edge tests' radii: a power of two exactly
        assert S.scale((8 * np.sqrt(2.0)) / 2 ** k, 8) == 2.0 ** k


def test_scale_refuses_bad_widths_and_radii():
    lib = _ffi.load()
    out = C.c_double(-7.0)
    for R, W in [(0.1, 0), (0.1, 45), (0.1, -1), (0.0, 8), (-1.0, 8), (float("nan"), 8), (float("inf"), 8)]:
        assert lib.sf_spin_scale(R, W, C.byref(out)) == -1, (R, W)
        assert _ffi.last_error().startswith("sf_spin_scale:"), _ffi.last_error()
        assert out.value == -7.0
    assert lib.sf_spin_scale(0.1, 8, None) == -1 and _ffi.last_error().startswith("sf_spin_scale:")
    assert lib.sf_spin_scale(0.1, 44, C.byref(out)) == 0 and lib.sf_spin_scale(0.1, 1, C.byref(out)) == 0
    assert _ffi.SPIN_MAX_WIDTH == S.MAX_WIDTH == 44


# ---- the weights --------------------------------------------------------------------------------------------------------------------
def test_every_entrys_four_weights_sum_to_two_to_the_32():
    rng = np.random.default_rng(1)
    W = 8
    u = np.r_[rng.random(5000) * W, np.arange(W + 1.0), np.nextafter(np.arange(1.0, W + 1), 0), np.nextafter(np.arange(W + 0.0), 99),
              np.arange(0, 4) / 65536.0, 3 + 65535 / 65536.0]
    v = np.r_[rng.random(u.size - 9) * 2 * W, np.arange(9.0) * 2]
    iu, iv, w = S.entry_weights(u, v)
    assert (w.sum(axis=1) == 1 << 32).all() and (w >= 0).all() and (w[:, 0] > 0).all()
    assert (iu == np.floor(u)).all() and (iv == np.floor(v)).all()
    on_node = u == np.floor(u)
    assert on_node.sum() >= W + 1 and (w[on_node][:, [1, 3]] == 0).all()  # (no weight leaves a node along u: iu + 1 is not addressed)


def _random_case(seed, n, k, R=0.25):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3))
    nrm = _unit(rng.standard_normal((n, 3)))
    kp = rng.choice(n, k, replace=False)
    lists = [np.flatnonzero(((pts - pts[i]) ** 2).sum(axis=1) <= R * R) for i in kp]
    return pts, nrm, kp, lists, R


@pytest.mark.parametrize("signed_beta", [True, False])
def test_unnormalised_rows_sum_to_exactly_the_contributing_count(signed_beta):
    """A node holds a multiple of 2^-32 and a list shorter than 2^21 entries keeps every partial sum below 2^21: 53 bits, so the
    float64 sum of a row is exact in any order."""
    pts, nrm, kp, lists, R = _random_case(2, 3000, 40)
    for W, min_cos in ((8, None), (3, 0.25), (44, None)):
        rows, cs = S.rows(pts, nrm, pts[kp], nrm[kp], lists, R, W, signed_beta, min_cos, return_counts=True)
        assert rows.shape == (40, S.shape(W, signed_beta)[1]) and (cs > 5).all() and (cs < [len(a) for a in lists]).all()
        assert np.array_equal(rows.sum(axis=1), cs.astype(np.float64)) and np.array_equal(rows[:, ::-1].sum(axis=1), cs.astype(np.float64))
        norm = S.rows(pts, nrm, pts[kp], nrm[kp], lists, R, W, signed_beta, min_cos, normalize=True)
        assert np.abs(norm.sum(axis=1) - 1.0).max() < 1e-13
    gated = S.rows(pts, nrm, pts[kp], nrm[kp], lists, R, 8, signed_beta, min_neighborhood_size=int(np.median(cs)))
    assert 0 < np.count_nonzero(gated.any(axis=1)) < 40


def test_the_keypoint_itself_duplicates_and_nan_take_no_part():
    p, n = np.array([0.5, 0.25, 0.125]), np.array([0.0, 0.0, 1.0])
    x = np.array([p, p, p + [0.01, 0, 0.01], [np.nan, 0, 0], p + [0, 0, 10.0], p + [10.0, 0, 0]])
    f = S.entry_coords(p, n, x, np.zeros((6, 3)), S.scale(0.1, 8), 8)
    assert f["keep"].tolist() == [False, False, True, False, False, False]
    f = S.entry_coords(p, n, x[2:3], np.array([[np.nan, 0, 0]]), S.scale(0.1, 8), 8, min_cos=-1.0)
    assert not f["keep"].any()


def test_unsigned_rows_do_not_see_a_sign():
    pts, nrm, kp, lists, R = _random_case(3, 2000, 20)
    flip = np.where(np.random.default_rng(4).random(2000) < 0.5, -1.0, 1.0)[:, None]
    a = S.rows(pts, nrm, pts[kp], nrm[kp], lists, R, 8, False, 0.3, return_counts=True)
    b = S.rows(pts, nrm * flip, pts[kp], (nrm * flip)[kp], lists, R, 8, False, 0.3, return_counts=True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and a[0].any()
    c = S.rows(pts, nrm * flip, pts[kp], (nrm * flip)[kp], lists, R, 8, True, 0.3)
    d = S.rows(pts, nrm, pts[kp], nrm[kp], lists, R, 8, True, 0.3)
    assert not np.array_equal(bits(c), bits(d))  # (the signed image does)


def test_quantised_rows_lie_within_c_2_to_the_minus_15_of_the_unquantised_image():
    """One entry with fractions (fu, fv) is quantised to (fu', fv') = (qu, qv) / 65536, du = fu - fu' and dv = fv - fv' in
    [0, 2^-16).  The four weights change by  -du (1 - fv') - dv (1 - fu') + du dv,  du (1 - fv') - fu' dv - du dv,
    dv (1 - fu') - fv' du - du dv,  fu' dv + fv' du + du dv:  mass du moves one node down along u and mass dv one node down along
    v, so the mass an entry moves is below du + dv < 2^-15, and its L1 distance -- the moved mass counted where it leaves and
    where it arrives -- below 2 (du + dv) < 2^-14.  Summed over a row's c entries: L1 < c 2^-14.  THAT is the guaranteed bound; it
    is asserted below for the row and for every entry on its own.
    The c 2^-15 that is also asserted is the figure the feature's specification sets for 10^4 random entries.  It is NOT a bound
    for arbitrary data, only what random data must stay within: fractions of independent entries average du = dv = 2^-17, which
    makes 2 (du + dv) = 2^-15 the MEAN per entry, and since every entry moves its mass the same way (down), what a node loses to
    its lower neighbours it regains from its upper ones wherever the neighbouring cells hold entries too, so a row of many spread
    entries lies well inside it (measured here: 0.13 and 0.16 of c 2^-15).  Entries that all sit just below a quantisation step
    in one cell could reach c 2^-14.  The float64 rounding of the unquantised image itself (c adds per node, each within 2^-53 of
    a value below c) is below c^2 2^-52 and does not show."""
    rng = np.random.default_rng(5)
    k, W, R = 10_000, 8, 0.5
    p, n = np.array([0.1, 0.2, 0.3]), _unit(rng.standard_normal((1, 3)))[0]
    x = p + (rng.random((k, 3)) - 0.5) * (2 * R / np.sqrt(2.0))
    m = np.zeros((k, 3))
    for signed_beta in (True, False):
        inv_bin = S.scale(R, W)
        cnt, c = S.counts(p, n, x, m, inv_bin, W, signed_beta)
        img, c2 = S.bilinear_float(p, n, x, m, inv_bin, W, signed_beta)
        assert c == c2 and c > 3000
        l1 = np.abs(S.to_row(cnt, c) - img).sum()
        print("signed" if signed_beta else "unsigned", "c =", c, "L1 =", l1, "bound", c * 2.0 ** -15, "ratio", l1 / (c * 2.0 ** -15))
        assert l1 < c * 2.0 ** -14  # (the guarantee)
        assert l1 <= c * 2.0 ** -15  # (the specification's figure for random entries)
        assert abs(img.sum() - c) < 1e-9 and S.to_row(cnt, c).sum() == c
        # every entry on its own: below 2^-14
        f = S.entry_coords(p, n, x, m, inv_bin, W, signed_beta)
        u, v = f["u"][f["keep"]], f["v"][f["keep"]]
        _, _, w = S.entry_weights(u, v)
        fu, fv = u - np.floor(u), v - np.floor(v)
        wf = np.stack([(1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv], axis=1)
        each = np.abs(w / S.TWO32 - wf).sum(axis=1)
        assert each.max() < 2.0 ** -14 and each.max() > 2.0 ** -16


# ---- the public function ------------------------------------------------------------------------------------------------------------
def test_compute_spin_image_descriptor_argument_errors_need_no_device():
    from shot_fpfh_amd.descriptors import compute_spin_image_descriptor

    pts = np.random.default_rng(5).random((20, 3))
    nr = _unit(np.random.default_rng(6).standard_normal((20, 3)))
    kp = np.arange(5)
    for W in (0, 45, -1):
        with pytest.raises(ValueError):
            compute_spin_image_descriptor(kp, pts, nr, 0.1, W)
    with pytest.raises(TypeError):
        compute_spin_image_descriptor(kp, pts, nr, 0.1, 8.5)
    for radius in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            compute_spin_image_descriptor(kp, pts, nr, radius)
    for mc in (1.5, -1.01, float("nan")):
        with pytest.raises(ValueError):
            compute_spin_image_descriptor(kp, pts, nr, 0.1, min_cos=mc)
    with pytest.raises(ValueError):
        compute_spin_image_descriptor(kp, pts, nr[:-1], 0.1)
    with pytest.raises(ValueError):
        compute_spin_image_descriptor(kp, pts[:, :2], nr[:, :2], 0.1)
    with pytest.raises(ValueError):
        compute_spin_image_descriptor(np.array([0, 20]), pts, nr, 0.1)
    with pytest.raises(ValueError):
        compute_spin_image_descriptor(np.array([-21]), pts, nr, 0.1)
    with pytest.raises(ValueError):
        compute_spin_image_descriptor(np.ones(19, dtype=bool), pts, nr, 0.1)
    bad = nr.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        compute_spin_image_descriptor(kp, pts, bad, 0.1)


def test_empty_inputs_give_zeros_of_the_right_shape():
    from shot_fpfh_amd.descriptors import compute_spin_image_descriptor

    pts = np.random.default_rng(5).random((20, 3))
    nr = _unit(np.random.default_rng(6).standard_normal((20, 3)))
    none = np.zeros(0, dtype=np.int64)
    assert compute_spin_image_descriptor(none, pts, nr, 0.1).shape == (0, 153)
    assert compute_spin_image_descriptor(none, pts, nr, 0.1, signed_beta=False).shape == (0, 81)
    assert compute_spin_image_descriptor(np.zeros(20, dtype=bool), pts, nr, 0.1, 3).shape == (0, 28)
    assert compute_spin_image_descriptor(none, np.zeros((0, 3)), np.zeros((0, 3)), 0.1, image_width=44).shape == (0, 4005)
    assert compute_spin_image_descriptor(none, pts, nr, 0.1, 1, signed_beta=False, normalize=True, min_cos=0.5).shape == (0, 4)


def test_names_are_exported():
    import shot_fpfh_amd
    from shot_fpfh_amd import descriptors
    from shot_fpfh_amd.descriptors import spin
    from shot_fpfh_amd.engine import Neighbors
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    assert "compute_spin_image_descriptor" in descriptors.__all__ and "compute_spin_image_descriptor" in shot_fpfh_amd.__all__
    assert spin.__all__ == ["compute_spin_image_descriptor"]
    assert shot_fpfh_amd.compute_spin_image_descriptor is spin.compute_spin_image_descriptor
    assert callable(Neighbors.spin_images) and callable(RegistrationPipeline.compute_spin_image_descriptor)
    lib = _ffi.load()
    assert lib.sf_spin_images and lib.sf_spin_scale


def test_header_declares_both_functions():
    text = open(os.path.join(ROOT, "include", "shotfpfh.h")).read()
    assert re.search(r"^int sf_spin_scale\(double radius, int64_t image_width, double \*inv_bin\);", text, re.M)
    assert re.search(r"^int sf_spin_images\(sf_ctx \*ctx, sf_cloud \*cloud, sf_nbrs \*nbrs, const double \*axes", text, re.M)
    assert re.search(r"^#define SF_SPIN_MAX_WIDTH 44\b", text, re.M)
    assert "spin.hip" in open(os.path.join(ROOT, "shot_fpfh_amd", "csrc", "Makefile")).read()


def test_the_script_takes_the_spin_options():
    text = open(os.path.join(ROOT, "scripts", "register_point_clouds.py")).read()
    assert '"spin"' in text and "--spin-width" in text and "--spin-signed" in text


# ---- the kernel's registers -------------------------------------------------------------------------------------------------------
def test_spin_kernel_does_not_spill():
    """From the compiler's resource remarks of csrc/spin.hip (written by every build): k_spin keeps every register -- a spill
    would sit inside the list walk -- and uses no scratch."""
    path = os.path.join(ROOT, "shot_fpfh_amd", "csrc", "build", "spin.remarks")
    assert os.path.exists(path), "no build/spin.remarks: the library is built by its Makefile, which writes it"
    res, cur = {}, None
    for ln in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    kernels = {k: v for k, v in res.items() if "k_spin" in k}
    assert len(kernels) == 1, list(res)
    for name, r in kernels.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)  # eight waves per SIMD by registers
