"""Trimmed ICP without a GPU: the order statistic and the rank of the NumPy statement (tests/icp_trimmed_numpy.py), its pass against
the statement without a trim, the conditions the GPU tests (tests/test_hip_icp_trimmed.py) place on their inputs, the accuracy the
trimming is for -- and what it costs without annealing -- and the argument checks of shot_fpfh_amd.icp.icp_trimmed,
RegistrationPipeline.run_icp and the script's parser."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import gicp_numpy as G
import icp_robust_numpy as S
import icp_trimmed_numpy as TR
import test_hip_icp_robust as H
import test_hip_icp_sums as T
import test_hip_icp_trimmed as HT
from conftest import ROOT
from test_hip_gicp import one_pass_set


# ---- 1. the order statistic ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", TR.SELECT_FAMILIES)
def test_select_statement_is_the_sorted_order_of_the_cleared_patterns(family):
    """np.partition's pick equals the rank-th of the keys sorted as unsigned 63-bit patterns (what the radix selection walks), and
    the two counts bracket the rank."""
    for n in (1, 2, 65, 4097):
        x = TR.select_keys(family, n)
        bits = np.sort(x.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF))
        for rank in TR.select_ranks(x):
            v, below, at_or_below = TR.select_kth(x, rank)
            assert np.float64(v).view(np.uint64) == bits[rank - 1], (family, n, rank)
            assert below < rank <= at_or_below
            assert not (v == 0.0 and math.copysign(1.0, v) < 0)  # a zero comes back as +0.0


def test_select_families_are_what_their_names_say():
    n = 4097
    assert np.unique(TR.select_keys("all_equal", n)).size == 1 and np.unique(TR.select_keys("two_values", n)).size == 2
    assert np.unique(TR.select_keys("seven_values", n)).size == 7
    low = TR.select_keys("low_bits", n).view(np.uint64)
    assert np.unique(low >> np.uint64(11)).size == 1 and np.unique(low & np.uint64(0x7FF)).size > 1000
    exps = np.unique(TR.select_keys("exponents", n))
    assert exps.size == 6 and np.unique(exps.view(np.uint64) >> np.uint64(52)).size >= 4  # 0 and 5e-324 share the zero exponent
    assert np.all((exps.view(np.uint64) & np.uint64((1 << 52) - 1))[[0, 2, 3, 4, 5]] == 0)
    z = TR.select_keys("signed_zeros", n)
    assert np.count_nonzero(np.signbit(z) & (z == 0)) > 1000 and np.count_nonzero(~np.signbit(z) & (z == 0)) > 1000
    v, below, at_or_below = TR.select_kth(z, 5)
    assert v == 0.0 and not np.signbit(v) and below == 0 and at_or_below == np.count_nonzero(z == 0)
    nan = TR.select_keys("nans", n)
    assert 0 < np.count_nonzero(np.isnan(nan)) < n and max(TR.select_ranks(nan)) == np.count_nonzero(~np.isnan(nan))
    assert not np.isnan(TR.select_keys("nans", 1)).any()
    for family in TR.SELECT_FAMILIES:
        for size in TR.SELECT_SIZES:
            if size <= 65537:
                x = TR.select_keys(family, size)
                assert x.shape == (size,) and x.dtype == np.float64 and 1 <= len(TR.select_ranks(x)) <= 64


def test_rank_formula():
    assert [TR.trim_rank(0.5, n) for n in (1, 2, 3, 4, 5)] == [1, 1, 2, 2, 3]
    assert TR.trim_rank(1e-9, 1000) == 1 and TR.trim_rank(1.0, 1000) == 1000 and TR.trim_rank(0.999999, 5) == 5
    assert TR.trim_rank(103 / 512, 512) == 103 and TR.trim_rank(104 / 512, 512) == 104
    assert TR.trim_rank(0.8, 1875) == 1500 and TR.trim_rank(0.3, 7) == 3  # 0.3 * 7 = 2.1 (and the product is rounded as a double)
    assert TR.used_pairs(np.zeros(0), 0.5)[:3] == (0, 0, 0.0) and TR.used_pairs(np.zeros(0), 0.5)[3].shape == (0,)
    n0, rank, cut, used = TR.used_pairs(np.array([3.0, 1.0, -0.0, 1.0, 2.0]), 0.4)
    assert (n0, rank, cut, used.tolist()) == (5, 2, 1.0, [False, True, True, True, False])  # the tie at the cut is used: 3 > rank
    n0, rank, cut, used = TR.used_pairs(np.array([3.0, 1.0, -0.0]), 0.2)
    assert (rank, cut, used.tolist()) == (1, 0.0, [False, False, True]) and not np.signbit(cut)


def test_trimmed_overlap_schedule():
    from shot_fpfh_amd.icp import trimmed_overlap

    got = [trimmed_overlap(0.8, 10, i) for i in range(14)]
    assert got[0] == 1.0 and got[1] == 1.0 - (1.0 - 0.8) * 1 / 10 and got[10:] == [0.8] * 4
    assert all(x >= y for x, y in zip(got, got[1:])) and got[9] > 0.8
    assert got == [TR.trimmed_overlap(0.8, 10, i) for i in range(14)]
    assert [trimmed_overlap(0.6, 0, i) for i in range(3)] == [0.6] * 3 == [TR.trimmed_overlap(0.6, 0, i) for i in range(3)]
    assert trimmed_overlap(1.0, 10, 3) == 1.0


# ---- 2. one pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", H.MODE_IDS)
def test_trim_one_is_the_statement_without_a_trim_and_a_trim_keeps_the_smallest_residuals(mode):
    s = one_pass_set()
    label, R, t = s["states"][1]
    a, na = s["scan"][:400], s["na"][:400]
    loss, k = S.LOSSES["cauchy"], H.K_ONE[mode]
    full = S.sums(mode, loss, k, a, na, s["ref"], s["nref"], R, t, H.D_MAX, tree=s["tree"])
    one = TR.sums(mode, loss, k, 1.0, a, na, s["ref"], s["nref"], R, t, H.D_MAX, tree=s["tree"])
    same = [c for c in range(48) if c not in (37, 38, 47)]
    assert np.array_equal(one["vec"][same], full["vec"][same]) and np.array_equal(one["abs"], full["abs"])
    assert one["vec"][37] == one["vec"][38] == one["vec"][0] == full["count"] and one["vec"][47] == 0.0
    r2 = TR.keys(mode, a, na, s["ref"], s["nref"], R, t, H.D_MAX, tree=s["tree"])
    assert r2.shape[0] == full["count"] and np.all(r2 >= 0)
    for trim in HT.TRIMS[:-1]:
        got = TR.sums(mode, loss, k, trim, a, na, s["ref"], s["nref"], R, t, H.D_MAX, tree=s["tree"])
        assert got["n0"] == full["count"] and got["rank"] == TR.trim_rank(trim, got["n0"]) == got["count"]  # no ties in this set
        assert got["cut"] == np.sort(r2)[got["rank"] - 1] and got["vec"][0] == got["count"]
        assert not got["vec"][TR.UNUSED[mode]].any()
        w = S.weight(loss, np.sort(r2)[:got["rank"]], k)
        assert math.isclose(got["vec"][7], math.fsum(w), rel_tol=1e-15) and math.isclose(got["vec"][46], math.fsum(w * np.sort(r2)[:got["rank"]]), rel_tol=1e-14)


# ---- 3. the conditions the GPU tests place on their inputs -----------------------------------------------------------------------------
def test_one_pass_trims_select_different_ranks_at_every_size():
    """At every size of the one-pass test with at least five pairs the five trims ask for five different ranks, the smallest for
    rank 1 and the largest for no selection; at the true motion no two kept pairs share a residual, so `used == rank` there."""
    s = one_pass_set()
    assert HT.TRIMS[0] * T.M_SIZES[-1] < 1 and HT.TRIMS[-1] == 1.0 and HT.TRIMS == sorted(HT.TRIMS)
    label, R, t = s["states"][1]
    for m in T.M_SIZES:
        for mode in H.MODE_IDS:
            r2 = TR.keys(mode, s["scan"][:m], s["na"][:m], s["ref"], s["nref"], R, t, H.D_MAX, tree=s["tree"])
            n0 = r2.shape[0]
            ranks = [TR.trim_rank(trim, n0) for trim in HT.TRIMS]
            assert ranks[0] == 1 and ranks[-1] == n0 >= 1
            if n0 >= 5:
                assert len(set(ranks)) == 5 and np.unique(r2).size == n0


def test_lattice_ties_are_what_the_gpu_test_expects():
    L = T.lattice_set()
    r2 = TR.keys(S.POINT, L["mixed"], None, L["ref"], None, None, None, T.LATTICE_R, tree=L["tree"])
    assert r2.shape == (512,) and np.count_nonzero(r2 == 0) == 103 == L["on_lattice"] and np.count_nonzero(r2 == 25 * 2.0**-14) == 409
    assert TR.used_pairs(r2, 103 / 512)[:3] == (512, 103, 0.0) and TR.used_pairs(r2, 103 / 512)[3].sum() == 103
    assert TR.used_pairs(r2, 104 / 512)[:3] == (512, 104, 25 * 2.0**-14) and TR.used_pairs(r2, 104 / 512)[3].sum() == 512
    below = float(np.nextafter(T.LATTICE_R, 0.0))
    r2 = TR.keys(S.POINT, L["mixed"], None, L["ref"], None, None, None, below, tree=L["tree"])
    assert r2.shape == (103,) and not r2.any()
    for trim in HT.TRIMS:
        n0, rank, cut, used = TR.used_pairs(r2, trim)
        assert (n0, cut, int(used.sum())) == (103, 0.0, 103)


def test_whole_run_inputs():
    """Every share of the schedule is reached inside the run, the run set keeps all its rows (tests/test_icp_robust_host.py asserts
    RUN_VOXEL does), and the clutter is the 20 % the overlap names."""
    scan, na, ref, nref, r0, t0 = H.clutter_run_set()
    assert 5 * S.CLUTTER == scan.shape[0] and TR.OVERLAP == 0.8  # a fifth of the scan is clutter
    assert TR.trimmed_overlap(TR.OVERLAP, TR.ANNEAL, HT.RUN_ITERATIONS - 5) == TR.OVERLAP < TR.trimmed_overlap(TR.OVERLAP, TR.ANNEAL, 5)


# ---- 4. what it is for --------------------------------------------------------------------------------------------------------------------
_rows = {}


def accuracy_row(seed):
    """|R - R0| of point-to-plane on clutter_set(seed) after 60 iterations of the statement with NumPy's pairwise sums: without a trim,
    with overlap 0.8 annealed over 10 iterations, with overlap 0.8 from iteration 0"""
    if seed not in _rows:
        scan, ref, r0, t0 = S.clutter_set(seed)
        nref = G.knn_normals(ref)
        row = {}
        for name, overlap, anneal in (("none", 1.0, 0), ("annealed", TR.OVERLAP, TR.ANNEAL), ("fixed", TR.OVERLAP, 0)):
            r = TR.refine(scan, None, ref, nref, S.PLANE, S.D_MAX, overlap, anneal, max_iter=TR.ITERATIONS, rms_threshold=0.0,
                          step_tolerance=0.0, how="np")
            row[name] = G.rotation_error(r["R"], r0)
        _rows[seed] = row
    return _rows[seed]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_annealed_trimming_removes_the_clutter_from_point_to_plane(seed):
    """25 % of the scan is a patch the reference does not have, inside d_max; overlap 0.8 annealed over 10 iterations leaves less than
    a fifth of the untrimmed run's rotation error (ratios of 9 to 30 when this was written)."""
    row = accuracy_row(seed)
    print(f"seed {seed}: " + ", ".join(f"{name} {err:.2e}" for name, err in row.items()))
    assert row["annealed"] < 0.2 * row["none"], row


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_fixed_overlap_from_a_coarse_start_is_worse_than_no_trimming(seed):
    """0.12 rad off, the clutter fits better than the true pairs: the share used from iteration 0 keeps it and drops them.  This is
    why the annealing is the default."""
    row = accuracy_row(seed)
    assert row["fixed"] > row["none"], row


def test_overlap_one_is_the_untrimmed_statement():
    scan, ref, r0, t0 = G.corner_set(0, n=300)
    nref = G.knn_normals(ref)
    got = TR.refine(scan, None, ref, nref, S.PLANE, 0.15, 1.0, 10, max_iter=5, rms_threshold=0.0, step_tolerance=0.0)
    want = S.refine(scan, None, ref, nref, S.PLANE, S.LOSSES["none"], 0.15, 1.0, 1.0, max_iter=5, rms_threshold=0.0, step_tolerance=0.0)
    assert np.array_equal(got["R"], want["R"]) and np.array_equal(got["t"], want["t"]) and got["rms_trace"] == want["rms_trace"]
    assert got["selections"] == [(c, c, c) for c in want["counts"]]


# ---- 5. arguments --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_upload(monkeypatch):
    import shot_fpfh_amd.icp as icp
    from shot_fpfh_amd.core import RigidTransform

    assert "icp_trimmed" in icp.__all__

    def no_device(*a, **kw):
        raise AssertionError("reached the device")

    monkeypatch.setattr(icp, "_Registration", no_device)
    monkeypatch.setattr(icp, "grid_subsampling", no_device)
    monkeypatch.setattr(icp, "compute_normals", no_device)
    pts = np.random.default_rng(1).random((50, 3))
    ok = dict(overlap=0.8, mode="point_to_plane", ref_normals=pts)
    for kw, word in ((dict(overlap=0.0), "overlap"), (dict(overlap=-0.1), "overlap"), (dict(overlap=1.0001), "overlap"),
                     (dict(overlap=float("nan")), "overlap"), (dict(overlap=None), "overlap"), (dict(anneal_iterations=-1), "anneal_iterations"),
                     (dict(anneal_iterations=2.5), "anneal_iterations"), (dict(mode="plane"), "mode"), (dict(loss="l2"), "loss"),
                     (dict(loss="cauchy"), "scale"), (dict(loss="cauchy", scale=0.0), "scale"),
                     (dict(loss="tukey", scale=0.01, scale_start=0.0), "scale_start"),
                     (dict(loss="tukey", scale=0.01, division_factor=1.0), "division_factor"), (dict(epsilon=0.0), "epsilon"),
                     (dict(step_tolerance=-1.0), "step_tolerance"), (dict(ref_normals=None), "ref_normals"),
                     (dict(mode="generalized", ref_normals=None, k_normals=2), "k_normals")):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            icp.icp_trimmed(pts, pts, RigidTransform(), 0.1, **args)
    with pytest.raises(ValueError, match="scan"):
        icp.icp_trimmed(pts[:, :2], pts, RigidTransform(), 0.1, **ok)
    with pytest.raises(TypeError):
        icp.icp_trimmed(pts, pts, RigidTransform(), 0.1, mode="point_to_point")  # overlap has no default
    # without a loss the scale is not looked at: the call gets as far as the device
    with pytest.raises(AssertionError, match="reached the device"):
        icp.icp_trimmed(pts, pts, RigidTransform(), 0.1, overlap=0.5, mode="point_to_point", scale=-1.0)


def test_pipeline_and_script_take_the_overlap():
    from shot_fpfh_amd.core import RigidTransform
    from shot_fpfh_amd.pipeline import RegistrationPipeline

    pts = np.random.default_rng(2).random((50, 3))
    pipe = RegistrationPipeline(scan=pts, scan_normals=None, ref=pts, ref_normals=pts)
    for bad in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match="overlap"):
            pipe.run_icp("point_to_plane", RigidTransform(), d_max=0.1, trim_overlap=bad)
    with pytest.raises(ValueError, match="anneal_iterations"):
        pipe.run_icp("point_to_plane", RigidTransform(), d_max=0.1, trim_overlap=0.8, trim_anneal_iterations=-2)
    with pytest.raises(ValueError, match="robust_scale"):
        pipe.run_icp("point_to_plane", RigidTransform(), d_max=0.1, trim_overlap=0.8, robust_loss="cauchy")
    with pytest.raises(ValueError, match="robust_loss"):
        pipe.run_icp("point_to_plane", RigidTransform(), d_max=0.1, trim_overlap=0.8, robust_scale=0.01)
    with pytest.raises(TypeError):
        pipe.run_icp("point_to_plane", RigidTransform(), 0.1, 0.2, 30, 1e-2, False, 20, 1e-3, None, None, None, 0.8)  # keyword-only
    spec = importlib.util.spec_from_file_location("register_point_clouds", os.path.join(ROOT, "scripts", "register_point_clouds.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    base = ["scan.ply", "ref.ply", "--radius", "0.2"]
    args = script.parse_args(base)
    assert (args.icp_overlap, args.icp_overlap_anneal) == (None, 10)
    args = script.parse_args(base + ["--icp-overlap", "0.8", "--icp-overlap-anneal", "0"])
    assert (args.icp_overlap, args.icp_overlap_anneal, args.icp_loss) == (0.8, 0, None)
    args = script.parse_args(base + ["--icp-overlap", "0.7", "--icp-loss", "tukey", "--icp-loss-scale", "0.012"])
    assert (args.icp_overlap, args.icp_overlap_anneal, args.icp_loss, args.icp_loss_scale) == (0.7, 10, "tukey", 0.012)
    for bad in (["--icp-overlap", "0"], ["--icp-overlap", "1.2"], ["--icp-overlap", "0.8", "--icp-overlap-anneal", "-1"],
                ["--icp-overlap", "0.8", "--icp-loss", "cauchy"], ["--icp-overlap", "x"]):
        with pytest.raises(SystemExit):
            script.parse_args(base + bad)


def test_layout_of_the_header_the_binding_and_the_reader():
    """include/shotfpfh.h declares the two calls the binding makes, and `_PairSums` reads the slots the statement writes."""
    from shot_fpfh_amd import _ffi
    from shot_fpfh_amd.icp import _PairSums

    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shotfpfh.h")).read(), flags=re.S)
    for name, want in (("sf_icp_accumulate_trimmed", ["ctx", "ref", "pts_dev", "nrm_dev", "sel_dev", "m", "Rt", "d_max", "mode", "epsilon",
                                                      "loss", "scale", "trim", "sums"]),
                       ("sf_select_kth", ["ctx", "keys_dev", "n", "rank", "out"])):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"include/shotfpfh.h does not declare {name}"
        params = [p.strip() for p in m.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == want and len(_ffi.SIGNATURES[name][1]) == len(want)
    s = one_pass_set()
    label, R, t = s["states"][1]
    v = TR.sums(S.PLANE, S.LOSSES["cauchy"], 0.02, 0.5, s["scan"][:400], s["na"][:400], s["ref"], s["nref"], R, t, H.D_MAX, tree=s["tree"])
    got = _PairSums(v["vec"], S.PLANE)
    assert (got.count, got.inside, got.rank, got.cut) == (v["count"], v["n0"], v["rank"], v["cut"]) and got.inside > got.count > 0
