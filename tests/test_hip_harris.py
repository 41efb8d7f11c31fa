"""Harris 3D keypoints on the MI355X (K23) against the NumPy statement of the definition (tests/harris_numpy.py: float64,
KDTree.query_radius balls, math.fsum sums, numpy.linalg.eigvalsh).

As for ISS, the check is split where the definition leaves a choice to the implementation: the order of a float64 sum.  Ball
sizes are compared exactly, the tensor and the responses under bounds derived below, accept / reject decisions everywhere but
at points the statement itself flags as near a threshold, and the suppression EXACTLY, on the device's own response array,
where it is nothing but comparisons of identical float64 values and exact ball membership.

The bounds (u = 2^-53, k the ball size, tr the trace, A_ab = sum |n_a n_b| / k):

Tensor entry, |C_dev - C| <= 1.01 (k + 2) u A_ab.  Both sides round every product once and identically; the device then rounds
at most k - 1 times in its sum whatever the order (adding the zeros of idle lanes is exact), fsum once, and either side once in
the division: k + 2 roundings of at most u A_ab each, the second order inside the 1.01.

det C, |det_dev - det| <= (k + 5) u tr^3.  To first order the difference is sum over the nine entries of adj(C)_ab dC_ab.  The
adjugate of a positive semi-definite C is positive semi-definite with eigenvalues l2 l3, l1 l3, l1 l2, each at most (tr / 2)^2,
so every |adj_ab| <= tr^2 / 4; the nine A_ab add up to sum_j (|n_x| + |n_y| + |n_z|)^2 / k <= 3 sum_j |n_j|^2 / k = 3 tr.  With
the entry bound that is (tr^2 / 4) (3 tr) 1.01 (k + 2) u = 0.76 (k + 2) u tr^3, rounded up to (k + 2) u tr^3 for the higher
orders.  The evaluation itself: six triple products, each at most tr^3 / 27 (|C_ab|^2 <= C_aa C_bb and the arithmetic-geometric
mean), each under five roundings (two multiplications, a difference, two sums), on either side: 2 x 6 x 5 / 27 = 2.3 -> 3 u tr^3.
(A looser count, 4 (k + 8) u tr^3, comes from bounding every A_ab by tr / 2 and every cofactor by tr^2 / 2; the one above is
sharper and is the one asserted.)

tr, |tr_dev - tr| <= (1.01 (k + 2) + 4) u tr: the three diagonal entries (A_aa = C_aa, they add up to tr) and two additions a side.
noble det / tr: the det bound over tr, plus (det / tr) <= tr^2 / 27 times the relative error of tr and one division a side:
  (k + 5) u tr^2 + (k + 9) / 27 u tr^2.
lowe det / tr^2: the det bound over tr^2, plus tr / 27 times twice the relative error of tr, one multiplication and one
  division a side: (k + 5) u tr + (2 k + 17) / 27 u tr.
harris 0.04 + det - 0.04 tr^2: the det bound, 0.04 tr^2 times twice the relative error of tr (0.08 (k + 7) u tr^2), and a side's
  evaluation -- 0.04 + det, the two multiplications of 0.04 (tr tr), the final difference: u (0.08 + 2 det + 0.12 tr^2) -- twice:
  ((k + 5.15) tr^3 + (0.08 (k + 7) + 0.24) tr^2 + 0.16) u.
tomasi: 1e-9 tr, curvature: 1e-9 absolute -- ISS's bound, for ISS's reason (Weyl on the entry bound gives ~1e-13; the
eigensolver is pinned elsewhere, tests/test_eigh3_host.py).

The position covariance behind "curvature" is the covariance sweep's own (the very launch ISS and sf_normals_radius make).  No
call hands that matrix out, so it is held bit for bit through what the library computes from it: for EVERY point, the device's
eigenvector of the smallest eigenvalue of the returned matrix (sf_eigh3) equals the normal sf_normals_radius returns -- a
function of all six entries; its smallest eigenvalue equals sf_iss_saliency's at gamma = 1 where that accepts the point; the six
entries repeat bit for bit after an unrelated search; and the response equals the same expression evaluated in NumPy on the
device's eigenvalues of the returned matrix."""
import numpy as np
import pytest

import harris_numpy as H
from conftest import config1_cloud, family, synth_cloud
from shot_fpfh_amd import ShotFpfhError
from shot_fpfh_amd.keypoint_selection import harris_response, select_keypoints_harris

N = H.N
pytestmark = pytest.mark.gpu


def _family(name, n=5000):
    return family(name, n, np.random.default_rng(1))[:2]


def _bumpy():
    from shot_fpfh_amd.descriptors import compute_normals

    p = N.bumpy_sphere(30000, 5)
    return p, compute_normals(p, p, radius=0.03)  # (PCA normals, arbitrary signs: computed once, handed to both sides)


def _one_normal_plane():
    p = _family("plane")[0]
    return p, np.tile(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), (p.shape[0], 1))


def _nonunit():
    p, nr, rng = synth_cloud(20000, 7)
    return p, nr * rng.uniform(0.5, 2.0, (p.shape[0], 1))


# name -> (points and normals, r, r_n)
CLOUDS = {
    "uniform": (lambda: synth_cloud(20000, 7)[:2], 0.06, 0.06),
    "sphere": (lambda: config1_cloud(35947, 1), 0.03, 0.03),
    "bumpy": (_bumpy, 0.03, 0.03),
    "lattice": (lambda: _family("lattice", 4096), 0.13, 0.13),
    "duplicates": (lambda: _family("duplicates"), 0.1, 0.1),
    "plane": (lambda: _family("plane"), 0.05, 0.05),
    "plane_one_normal": (_one_normal_plane, 0.05, 0.05),
    "rough_plane": (lambda: _family("rough_plane"), 0.05, 0.05),
    "slab": (lambda: _family("slab"), 0.05, 0.05),
    "far_origin": (lambda: _family("far_origin"), 0.1, 0.1),
    "clustered": (lambda: _family("clustered"), 0.05, 0.05),
    "nonunit_normals": (_nonunit, 0.06, 0.06),
    "uniform_rn_3r": (lambda: synth_cloud(20000, 7)[:2], 0.03, 0.09),  # the suppression needs another grid
    "uniform_r_3rn": (lambda: synth_cloud(20000, 7)[:2], 0.09, 0.03),  # the tensor grid is too coarse to keep
    # a wave serves four points: last waves of one, two and three, balls of several hundred points over many 128-candidate steps
    "last_wave_of_1": (lambda: synth_cloud(2001, 7)[:2], 0.4, 0.4),
    "last_wave_of_2": (lambda: synth_cloud(2002, 7)[:2], 0.15, 0.15),
    "last_wave_of_3": (lambda: synth_cloud(2003, 7)[:2], 0.15, 0.15),
    "three_points": (lambda: synth_cloud(3, 7)[:2], 2.0, 2.0),  # ... and a wave that is the whole launch
}
MIN_NB = {"three_points": 1}  # (three points: the default of 5 would reject them all)

_cache = {}


def _case(name, engine):
    """one cloud: points, normals, radii, the statement's side (counts, C, A, position eigenvalues) and the device's (per method:
    response, counts, matrices), computed once"""
    if name not in _cache:
        make, r, r_n = CLOUDS[name]
        p, nr = make()
        counts, C, A = H.tensor(p, nr, r)
        counts_e, e = N.ball_eigenvalues(p, r)
        assert np.array_equal(counts, counts_e)
        dev = {}
        cloud = engine.cloud(p, nr)
        try:
            for method in H.METHODS:
                dev[method] = cloud.harris_response(r, method, min_neighbors=MIN_NB.get(name, 5), return_counts=True, return_tensor=True)
            iss_e3 = cloud.iss_saliency(r, 1.0, 1.0, 1)
        finally:
            cloud.free()
        cloud = engine.cloud(p)  # (a cloud of its own: sf_normals_radius on the grid it builds for r itself)
        try:
            cov_normals = cloud.normals_radius(p, r)
        finally:
            cloud.free()
        _cache[name] = dict(cov_normals=cov_normals, p=p, nr=nr, r=r, r_n=r_n, counts=counts, C=C, A=A, e=e, dev=dev, iss_e3=iss_e3, min_nb=MIN_NB.get(name, 5))
    return _cache[name]


@pytest.fixture(scope="module")
def engine():
    from shot_fpfh_amd import default_engine

    return default_engine()


@pytest.mark.parametrize("name", list(CLOUDS))
def test_tensor_and_response_against_the_statement(name, engine):
    c = _case(name, engine)
    p, counts, C, A, e = c["p"], c["counts"], c["C"], c["A"], c["e"]
    n = p.shape[0]
    tr = H.trace(C)
    for method in H.METHODS:
        res, cnt, ten = c["dev"][method]
        assert res.dtype == np.float64 and res.shape == (n,) and ten.shape == (n, 6)
        assert np.array_equal(cnt, counts), "ball sizes differ"  # the project's neighbour-set rule: 100 %
        if method == "curvature":
            w = engine.eigh3(H.full(ten))[0]  # (ascending: the device's own eigenvalues of the matrix it returned)
            took = c["iss_e3"] > 0
            assert np.array_equal(w[took, 0], c["iss_e3"][took]), "not the covariance sweep's matrix"
            # ... and every point, all six entries: the eigenvector of the smallest eigenvalue is sf_normals_radius' normal
            assert np.array_equal(engine.eigh3(H.full(ten))[1][:, :, 0], c["cov_normals"]), "not the covariance sweep's matrix"
            assert took.sum() >= (0.9 * n if name in ("uniform", "sphere", "bumpy") else 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                value = w[:, 0] / ((w[:, 2] + w[:, 1]) + w[:, 0])
            assert np.array_equal(res[res > 0], value[res > 0])
            worst_t = float((np.abs(np.linalg.eigvalsh(H.full(ten))[:, ::-1] - e).max(axis=1) / np.maximum(e[:, 0], 1e-300))[e[:, 0] > 0].max(initial=0.0)) / 1e-9
            ref = H.response_from(method, counts, e=e, min_neighbors=c["min_nb"])
            near = H.near_a_threshold(method, e=e)
            scale_tr = np.ones(n)
        else:
            assert np.array_equal(ten, c["dev"]["harris"][2]), "the tensor depends on the method"
            bound_t = H.tensor_bound(counts, A)
            gap_t = np.abs(ten - C)
            assert np.all(gap_t[bound_t == 0] == 0)
            worst_t = float((gap_t[bound_t > 0] / bound_t[bound_t > 0]).max(initial=0.0))
            ref = H.response_from(method, counts, C=C, min_neighbors=c["min_nb"])
            near = H.near_a_threshold(method, C=C)
            scale_tr = tr
        both = (res > 0) & (ref > 0)
        bound_r = H.response_bound(method, counts[both].astype(np.float64), scale_tr[both])
        worst_r = float((np.abs(res[both] - ref[both]) / bound_r).max(initial=0.0))
        differ = (res > 0) != (ref > 0)
        excepted = differ & near
        print(f"HARRIS_PARITY {name} {method} n={n} r={c['r']} max_ball={int(counts.max())} accepted_numpy={int((ref > 0).sum())} "
              f"accepted_device={int((res > 0).sum())} tensor_over_bound={worst_t:.3e} response_over_bound={worst_r:.3e} "
              f"decisions_differ={int(differ.sum())} near_threshold={int(near.sum())}")
        assert np.all((res > 0) | (res == -1.0))
        assert worst_t <= 1.0
        assert worst_r <= 1.0
        assert not np.any(differ & ~excepted), np.flatnonzero(differ & ~excepted)[:10]
        assert excepted.sum() <= 1e-3 * n


@pytest.mark.parametrize("name", list(CLOUDS))
def test_suppression_is_exact_on_the_devices_own_response(name, engine):
    c = _case(name, engine)
    p, r_n = c["p"], c["r_n"]
    cloud = engine.cloud(p)
    try:
        for method in H.METHODS:
            res = c["dev"][method][0]
            got, want = cloud.iss_select(res, r_n, c["min_nb"]), N.select(p, res, r_n, c["min_nb"])
            print(f"HARRIS_SELECT {name} {method} r_n={r_n} keypoints={want.size}")
            assert got.dtype == np.int64 and np.array_equal(got, want), method
    finally:
        cloud.free()


@pytest.mark.parametrize("name", ["uniform", "sphere", "lattice", "duplicates", "nonunit_normals", "uniform_rn_3r", "uniform_r_3rn", "last_wave_of_3"])
def test_end_to_end(name, engine):
    c = _case(name, engine)
    p, nr, r, r_n = c["p"], c["nr"], c["r"], c["r_n"]
    flip = np.where(np.random.default_rng(2).random(p.shape[0]) < 0.5, -1.0, 1.0)[:, None]
    for method in ("harris", "tomasi", "curvature") if name != "uniform" else H.METHODS:
        res = c["dev"][method][0]
        kp, r2 = select_keypoints_harris(p, nr, r, r_n, method=method, return_response=True)
        assert kp.dtype == np.int64 and np.all(np.diff(kp) > 0)
        assert np.array_equal(r2, res) and np.array_equal(harris_response(p, nr, r, method=method), res)  # bit for bit
        cloud = engine.cloud(p, nr)
        try:
            assert np.array_equal(kp, cloud.iss_select(cloud.harris_response(r, method), r_n))
            assert np.array_equal(kp, cloud.harris_keypoints(r, r_n, method))  # a second call on the same cloud repeats
        finally:
            cloud.free()
        if r_n == r:
            assert np.array_equal(kp, select_keypoints_harris(p, nr, r, method=method))  # one radius by default
        for other in (1.7 * r, 0.8 * r_n):  # the same Cloud, searched at another radius first: a grid the passes must not trust
            cloud = engine.cloud(p, nr)
            try:
                cloud.radius_search(p[:64], other)
                k3, r3 = cloud.harris_keypoints(r, r_n, method, return_response=True)
                assert np.array_equal(r3, res) and np.array_equal(k3, kp)
                cloud.radius_search(p[:64], other)
                r5, c5, t5 = cloud.harris_response(r, method, return_counts=True, return_tensor=True)  # all six entries, every point
                assert np.array_equal(t5, c["dev"][method][2]) and np.array_equal(c5, c["counts"]) and np.array_equal(r5, res)
            finally:
                cloud.free()
        cloud = engine.cloud(p, nr * flip)  # the sign PCA normals come with does not matter, to the bit
        try:
            r4, _, t4 = cloud.harris_response(r, method, return_counts=True, return_tensor=True)
            assert np.array_equal(t4, c["dev"][method][2]) and np.array_equal(r4, res)
            assert np.array_equal(cloud.harris_keypoints(r, r_n, method), kp)
        finally:
            cloud.free()


def test_a_plane_with_one_common_normal_has_no_keypoints(engine):
    c = _case("plane_one_normal", engine)
    for method in H.TENSOR_METHODS:
        assert np.all(c["dev"][method][0] == -1.0), method
        kp, res = select_keypoints_harris(c["p"], c["nr"], c["r"], method=method, return_response=True)
        assert kp.dtype == np.int64 and kp.size == 0 and np.all(res == -1.0)


def test_refused_inputs_and_a_cloud_without_normals(engine):
    p, nr, _ = synth_cloud(3000, 7)
    cloud = engine.cloud(p)  # no normals
    try:
        for method in H.TENSOR_METHODS:
            with pytest.raises(ShotFpfhError, match="normals"):
                cloud.harris_response(0.1, method)
            with pytest.raises(ShotFpfhError, match="normals"):
                cloud.harris_keypoints(0.1, 0.1, method)
        res = cloud.harris_response(0.1, "curvature")
        assert np.array_equal(res, harris_response(p, None, 0.1, method="curvature")) and (res > 0).sum() > 2000
        assert np.array_equal(cloud.harris_keypoints(0.1, method="curvature"), select_keypoints_harris(p, None, 0.1, method="curvature"))
        for bad in (dict(threshold=-1e-9), dict(threshold=float("nan")), dict(min_neighbors=0)):
            with pytest.raises(ShotFpfhError):
                cloud.harris_response(0.1, "curvature", **bad)
            with pytest.raises(ShotFpfhError):
                cloud.harris_keypoints(0.1, 0.1, "curvature", **bad)
        for bad_radius in (0.0, -1.0, float("inf")):
            with pytest.raises(ShotFpfhError):
                cloud.harris_response(bad_radius, "curvature")
            with pytest.raises(ShotFpfhError):
                cloud.harris_keypoints(0.1, bad_radius, "curvature")
        with pytest.raises(ValueError):
            cloud.harris_response(0.1, "shi")
    finally:
        cloud.free()
    lib, h = engine.lib, engine.h
    cloud = engine.cloud(p, nr)
    try:
        out = np.zeros(3000)
        assert lib.sf_harris_response(h, cloud.h, 0.1, 5, 0.0, 5, out.ctypes.data, None, None, 0) != 0  # (method out of the enum)
        assert lib.sf_harris_response(h, cloud.h, 0.1, -1, 0.0, 5, out.ctypes.data, None, None, 0) != 0
    finally:
        cloud.free()


def test_device_resident_outputs_equal_the_host_ones(engine):
    """SF_OUT_DEVICE: response, count, tensor and selected are device pointers, as in the ISS calls; *n_selected stays on the host"""
    import ctypes

    from shot_fpfh_amd._ffi import SF_OUT_DEVICE, check

    c = _case("uniform_rn_3r", engine)
    p, nr, r, r_n = c["p"], c["nr"], c["r"], c["r_n"]
    n, lib, h = p.shape[0], engine.lib, engine.h
    cloud = engine.cloud(p, nr)
    res, cnt, ten, sel = engine.empty((n,)), engine.empty((n,), np.int32), engine.empty((n, 6)), engine.empty((n,), np.int64)
    try:
        for method in ("harris", "tomasi", "curvature"):
            mid = H.METHODS.index(method)
            want_res, want_cnt, want_ten = c["dev"][method]
            want_kp = cloud.harris_keypoints(r, r_n, method)
            for buf in (res, ten):
                buf.from_host(np.full(buf.shape, np.nan))
            check(lib.sf_harris_response(h, cloud.h, r, mid, 0.0, 5, res.ptr, cnt.ptr, ten.ptr, SF_OUT_DEVICE), "sf_harris_response")
            assert np.array_equal(res.to_host(), want_res) and np.array_equal(cnt.to_host(), want_cnt) and np.array_equal(ten.to_host(), want_ten)
            res.from_host(np.full(n, np.nan))
            check(lib.sf_harris_response(h, cloud.h, r, mid, 0.0, 5, res.ptr, None, None, SF_OUT_DEVICE), "sf_harris_response")
            assert np.array_equal(res.to_host(), want_res)
            for response in (res, None):
                res.from_host(np.full(n, np.nan))
                sel.from_host(np.full(n, -1, dtype=np.int64))
                k = ctypes.c_int64(-1)
                check(lib.sf_harris_keypoints(h, cloud.h, r, r_n, mid, 0.0, 5, None if response is None else response.ptr, sel.ptr,
                                              ctypes.byref(k), SF_OUT_DEVICE), "sf_harris_keypoints")
                assert k.value == want_kp.size and np.array_equal(sel.to_host()[: k.value], want_kp)
                if response is not None:
                    assert np.array_equal(res.to_host(), want_res)
    finally:
        for buf in (res, cnt, ten, sel):
            buf.free()
        cloud.free()


@pytest.mark.parametrize("method", H.METHODS)
def test_a_threshold_at_the_median_halves_the_accepted_set_as_the_statement_does(method, engine):
    c = _case("uniform", engine)
    p, nr, r, counts = c["p"], c["nr"], c["r"], c["counts"]
    kw = dict(e=c["e"]) if method == "curvature" else dict(C=c["C"])
    ref0 = H.response_from(method, counts, **kw)
    med = float(np.median(ref0[ref0 > 0]))
    ref = H.response_from(method, counts, threshold=med, **kw)
    res = harris_response(p, nr, r, method=method, threshold=med)
    assert abs(2 * int((ref > 0).sum()) - int((ref0 > 0).sum())) <= 1
    differ = (res > 0) != (ref > 0)
    near = H.near_a_threshold(method, threshold=med, **kw)
    print(f"HARRIS_THRESHOLD {method} median={med:.6e} accepted={int((res > 0).sum())} of {int((ref0 > 0).sum())} differ={int(differ.sum())}")
    assert not np.any(differ & ~near) and (differ & near).sum() <= 1e-3 * p.shape[0]
    assert np.array_equal(res[res > 0], c["dev"][method][0][res > 0])  # the survivors keep their values


def test_pipeline_feeds_fpfh_and_shot(engine):
    from shot_fpfh_amd import RegistrationPipeline

    p, d = config1_cloud(35947, 1)
    q, dq = config1_cloud(20000, 2)
    pipe = RegistrationPipeline(scan=p, scan_normals=d, ref=q, ref_normals=dq)
    pipe.select_keypoints("harris", neighborhood_size=0.03)
    assert np.array_equal(pipe.scan_keypoints, select_keypoints_harris(p, d, 0.03))
    assert np.array_equal(pipe.ref_keypoints, select_keypoints_harris(q, dq, 0.03))
    assert pipe.scan_keypoints.dtype == np.int64 and 0 < pipe.scan_keypoints.size < p.shape[0] // 4
    pipe.compute_descriptors(radius=0.06, descriptor_choice="fpfh", disable_progress_bars=True, verbose=False)
    assert pipe.scan_descriptors.shape == (pipe.scan_keypoints.size, 125) and np.isfinite(pipe.scan_descriptors).all()
    pipe.compute_descriptors(radius=0.06, descriptor_choice="shot_single_scale", subsample_support=False, min_neighborhood_size=10,
                             disable_progress_bars=True, verbose=False, force_recompute=True)
    assert pipe.ref_descriptors.shape == (pipe.ref_keypoints.size, 352) and np.isfinite(pipe.ref_descriptors).all()
    pipe.select_keypoints("harris", neighborhood_size=0.03, harris_method="tomasi", harris_non_max_radius=0.05, min_n_neighbors=8,
                          force_recompute=True)
    assert np.array_equal(pipe.ref_keypoints, select_keypoints_harris(q, dq, 0.03, 0.05, method="tomasi", min_neighbors=8))
